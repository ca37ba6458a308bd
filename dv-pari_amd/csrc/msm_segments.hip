// Many independent MSMs in one call: out[j] = sum over seg_ptr[j] <= i < seg_ptr[j+1] of k_i P_i, the reference's multi_scalar_mul
// (src/curve.rs:141-158: a map of point_scalar_mul, then an add tree) over consecutive slices of one scalar and one point vector.
//
//   stage 1   points_mul_dev (points_mul.hip) as it stands: the n affine products and their infinity flags, into d_work
//   stage 2   a segmented reduction of those products, level after level (k_seg_reduce):
//               level 0      every segment is cut into pieces of at most P consecutive products; one lane sums a piece into a
//                            Lopez-Dahab accumulator with the complete mixed addition (madd_complete: equal, opposite and O operands)
//               level l > 0  the piece sums of a segment are cut into pieces of at most P again and summed with the complete full
//                            addition (ld_add_nodbl, the doubling from a copy read back)
//               last level   reached when no segment holds more than P operands: one lane per SEGMENT sums what is left, inverts
//                            once (gf_inv_fast) and stores the affine sum; O for a segment without operands
//
// A piece never crosses a segment boundary and the pieces of a level are numbered segment by segment, so the operands of piece q of
// segment j at level l are off_l[j] + q P ... and its sum is operand off_(l+1)[j] + q of the next level.  The offset arrays off_l
// (n_seg + 1 words each, off_0 = seg_ptr) are computed on the host, where seg_ptr lives, and uploaded with one copy; a lane of a
// level before the last finds its segment by bisection in off_(l+1).  Nothing is accumulated with atomics and every output has one
// writer: the same inputs give the same bytes.
//
// Dependent chain behind stage 1: P mixed additions, then P - 1 full additions per further level, one inversion -- at most
// P ceil(log_P(longest segment)) additions whatever the cut: one segment of n points and n segments of one point both run as
// cdiv(tasks, 256) workgroups of full lanes per level.  Extra work: n mixed additions and fewer than n / (P - 1) full ones.
//
// Out of scope: gathered bases (a column index per term), a per-segment bucket method in LDS, fusing the reduction into k_points_mul,
// a device-resident seg_ptr, and use of this entry inside the prover.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "common.h"
#include "k233.cuh"
#include "host_api.h"

namespace dvp {


constexpr int SEG_TPB = 256;
constexpr unsigned SEG_LDS = (SEG_TPB / 64) * GF_LDSK_BYTES_PER_WAVE;
constexpr long long SEG_PIECE_DEFAULT = 4, SEG_PIECE_MAX = 64;

// the segment of task t: the largest j with off[j] <= t (off[0] = 0 <= t < off[n_seg]; empty segments repeat an offset and are
// passed over)
__device__ __forceinline__ uint32_t seg_find(const uint32_t* __restrict__ off, uint32_t n_seg, uint32_t t) {
  uint32_t lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// One level.  AFF: the operands are the affine products and flags of stage 1, else the Lopez-Dahab sums of the level before.
// FINAL: one task per segment (no search), affine out; else one task per piece, its sum to out[task].
template <bool AFF, bool FINAL>
__global__ void __launch_bounds__(SEG_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_seg_reduce(const Aff* __restrict__ prod, const uint8_t* __restrict__ flags, const Ld* __restrict__ in, const uint32_t* __restrict__ off_in,
             const uint32_t* __restrict__ off_out, uint32_t n_seg, uint32_t n_tasks, uint32_t P, GfSqrTables T, Ld* __restrict__ out,
             Aff* __restrict__ out_xy, uint8_t* __restrict__ out_inf) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  uint32_t start, len;
  if (FINAL) {
    start = off_in[t];
    len = off_in[t + 1] - start;
  } else {
    const uint32_t j = seg_find(off_out, n_seg, t);
    start = off_in[j] + (t - off_out[j]) * P;
    len = min(P, off_in[j + 1] - start);
  }
  Ld acc = ld_infinity();
  if (AFF) {
#pragma unroll 1
    for (uint32_t k = 0; k < len; ++k) {
      if (flags[start + k]) continue;
      const Aff q = prod[start + k];
      madd_complete(acc, q, L);
    }
  } else {
    if (len) acc = in[start];
#pragma unroll 1
    for (uint32_t k = 1; k < len; ++k) {
      if (!ld_add_nodbl(acc, in[start + k], L)) {  // acc == the operand: double a copy read back
        acc = in[start + k];
        acc = ld_dbl(acc, L);
      }
    }
  }
  if (!FINAL) {
    out[t] = acc;
    return;
  }
  Aff a;
  a.x = gf_zero();
  a.y = gf_zero();
  const bool fin = !ld_is_inf(acc);
  if (fin) {
    const Gf zi = gf_inv_fast(acc.Z, T, L);
    a.x = gf_mul(acc.X, zi, L);
    a.y = gf_mul(acc.Y, gf_sqr(zi), L);
  }
  out_xy[t] = a;
  out_inf[t] = fin ? 0 : 1;
}

static uint32_t seg_piece() {
  const long long p = tune().msm_seg_piece;
  return (uint32_t)((p >= 2 && p <= SEG_PIECE_MAX) ? p : SEG_PIECE_DEFAULT);
}

// ---- d_work: products | flags | piece sums of the even levels | piece sums of the odd levels | offsets ----
// Level 0 leaves sum of ceil(len_j / P) <= (n + non-empty segments) / 2 sums for P >= 2, the next level at most as many of those
// again, and from there on every level fits the buffer two levels back.  Offsets: one array per level; P = 2 needs the most,
// ceil(log2 n) of them (a level runs while some segment holds more than P operands).
struct SegLayout {
  size_t prod, flags, buf[2], cap[2], geo, geo_levels, total;
};
static SegLayout seg_layout(size_t n, size_t n_seg) {
  SegLayout w;
  w.cap[0] = (n + std::min(n, n_seg)) / 2;
  w.cap[1] = (w.cap[0] + std::min(w.cap[0], n_seg)) / 2;
  size_t lg = 1;
  while (lg < 40 && ((size_t)1 << lg) < n) ++lg;
  w.geo_levels = lg + 1;
  Carver c;
  w.prod = c.take(n * sizeof(Aff));
  w.flags = c.take(n);
  w.buf[0] = c.take(w.cap[0] * sizeof(Ld));
  w.buf[1] = c.take(w.cap[1] * sizeof(Ld));
  w.geo = c.take(w.geo_levels * (n_seg + 1) * sizeof(uint32_t));
  w.total = c.o;
  return w;
}

// seg_ptr[0] == 0, non-decreasing, seg_ptr[n_seg] == n; else the first offending segment
static bool seg_ptr_ok(const uint64_t* seg_ptr, size_t n, size_t n_seg, int64_t* bad) {
  if (seg_ptr[0] != 0) {
    *bad = 0;
    return false;
  }
  for (size_t j = 0; j < n_seg; ++j)
    if (seg_ptr[j] > seg_ptr[j + 1] || seg_ptr[j + 1] > n) {
      *bad = (int64_t)j;
      return false;
    }
  if (seg_ptr[n_seg] != n) {
    *bad = (int64_t)n_seg - 1;
    return false;
  }
  return true;
}

// what every flavour decides before any device call
static int seg_check_sizes(size_t n, const uint64_t* seg_ptr, size_t n_seg) {
  if (!seg_ptr || n >= ((size_t)1 << 32) || n_seg >= ((size_t)1 << 32)) return DVP_EINVAL;
  int64_t bad;
  if (!seg_ptr_ok(seg_ptr, n, n_seg, &bad)) {
    g_last_error_index = bad;
    return DVP_EINVAL;
  }
  return DVP_OK;
}

// ---- pinned staging for the offsets: a ring of slots, each guarded by an event recorded behind its copy ----
struct SegStage {
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  int dev = -1;
  bool pending = false;
};
constexpr int SEG_RING = 4;
static std::mutex g_seg_mu;
static SegStage g_seg_ring[SEG_RING];
static unsigned g_seg_next = 0;

static int seg_stage_acquire(size_t bytes, SegStage** out) {
  SegStage& s = g_seg_ring[g_seg_next++ % SEG_RING];
  int dev;
  DVP_HIP(hipGetDevice(&dev));
  if (s.pending) {
    DVP_HIP(hipEventSynchronize(s.ev));
    s.pending = false;
  }
  if (s.ev && s.dev != dev) {
    DVP_HIP(hipEventDestroy(s.ev));
    s.ev = nullptr;
  }
  if (!s.ev) {
    DVP_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    s.dev = dev;
  }
  if (s.cap < bytes) {
    if (s.p) DVP_HIP(hipHostFree(s.p));
    s.p = nullptr;
    s.cap = 0;
    size_t cap = 1 << 16;
    while (cap < bytes) cap <<= 1;
    DVP_HIP(hipHostMalloc(&s.p, cap, hipHostMallocPortable));
    s.cap = cap;
  }
  *out = &s;
  return DVP_OK;
}

template <bool AFF, bool FINAL>
static void seg_launch(const SegLayout& w, char* work, int level, uint32_t n_seg, uint32_t n_tasks, uint32_t P, const GfSqrTables& T, void* d_out_xy,
                       void* d_out_inf, hipStream_t st) {
  const uint32_t* geo = (const uint32_t*)(work + w.geo);
  const uint32_t* off_in = geo + (size_t)level * (n_seg + 1);
  const uint32_t* off_out = off_in + (n_seg + 1);  // not read by the last level
  const Ld* in = level ? (const Ld*)(work + w.buf[(level - 1) & 1]) : nullptr;
  Ld* out = (Ld*)(work + w.buf[level & 1]);
  DVP_LAUNCH((k_seg_reduce<AFF, FINAL>), dim3(cdiv(n_tasks, SEG_TPB)), dim3(SEG_TPB), SEG_LDS, st, (const Aff*)(work + w.prod),
                     (const uint8_t*)(work + w.flags), in, off_in, off_out, n_seg, n_tasks, P, T, out, (Aff*)d_out_xy, (uint8_t*)d_out_inf);
}

// enqueue only; the arguments have been checked (n < 2^32, 0 < n_seg < 2^32, seg_ptr sound, work_bytes enough)
static int msm_segments_dev(const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, const uint64_t* seg_ptr, size_t n_seg, void* d_out_xy,
                            void* d_out_inf, void* d_work, void* d_summary, hipStream_t st) {
  if (!n) {  // n_seg times O; the summary as an empty dvp_points_mul_dev leaves it
    DVP_TRY(points_mul_dev(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, d_summary, st));
    DVP_HIP(hipMemsetAsync(d_out_xy, 0, n_seg * sizeof(Aff), st));
    DVP_HIP(hipMemsetAsync(d_out_inf, 1, n_seg, st));
    return DVP_OK;
  }
  const SegLayout w = seg_layout(n, n_seg);
  char* work = (char*)d_work;
  const uint32_t P = seg_piece();
  uint64_t longest = 0;
  for (size_t j = 0; j < n_seg; ++j) longest = std::max<uint64_t>(longest, seg_ptr[j + 1] - seg_ptr[j]);
  size_t levels = 1;  // offset arrays = kernel launches
  for (uint64_t c = longest; c > P; c = (c + P - 1) / P) ++levels;
  if (levels > w.geo_levels) return DVP_EINVAL;  // cannot happen: geo_levels covers P = 2
  const size_t row = n_seg + 1, geo_bytes = levels * row * sizeof(uint32_t);
  uint32_t tasks[64];
  {
    std::lock_guard<std::mutex> g(g_seg_mu);
    SegStage* s;
    DVP_TRY(seg_stage_acquire(geo_bytes, &s));
    uint32_t* off = (uint32_t*)s->p;
    for (size_t j = 0; j < row; ++j) off[j] = (uint32_t)seg_ptr[j];
    for (size_t l = 1; l < levels; ++l) {
      const uint32_t* a = off + (l - 1) * row;
      uint32_t* b = off + l * row;
      uint32_t run = 0;
      for (size_t j = 0; j < n_seg; ++j) {
        b[j] = run;
        run += (a[j + 1] - a[j] + P - 1) / P;
      }
      b[n_seg] = run;
      tasks[l - 1] = run;
      if (run > w.cap[(l - 1) & 1]) return DVP_EINVAL;  // cannot happen: seg_layout's bounds
    }
    DVP_HIP(hipMemcpyAsync(work + w.geo, s->p, geo_bytes, hipMemcpyHostToDevice, st));
    DVP_HIP(hipEventRecord(s->ev, st));
    s->pending = true;
  }
  DVP_TRY(points_mul_dev(d_scalars, n, d_xy, d_inf, n, work + w.prod, work + w.flags, d_summary, st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  for (size_t l = 0; l + 1 < levels; ++l) {
    if (l == 0) seg_launch<true, false>(w, work, 0, (uint32_t)n_seg, tasks[0], P, T, d_out_xy, d_out_inf, st);
    else seg_launch<false, false>(w, work, (int)l, (uint32_t)n_seg, tasks[l], P, T, d_out_xy, d_out_inf, st);
  }
  if (levels == 1) seg_launch<true, true>(w, work, 0, (uint32_t)n_seg, (uint32_t)n_seg, P, T, d_out_xy, d_out_inf, st);
  else seg_launch<false, true>(w, work, (int)levels - 1, (uint32_t)n_seg, (uint32_t)n_seg, P, T, d_out_xy, d_out_inf, st);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}


}  // namespace dvp

using namespace dvp;

extern "C" size_t dvp_msm_segments_work_bytes(size_t n, size_t n_seg) {
  if (n >= ((size_t)1 << 32) || n_seg >= ((size_t)1 << 32)) return 0;
  return seg_layout(n, n_seg).total;
}

extern "C" int dvp_msm_segments_dev(const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, const uint64_t* seg_ptr, size_t n_seg,
                                    void* d_out_xy, void* d_out_inf, void* d_work, size_t work_bytes, void* d_summary, void* stream) {
  if (!n_seg) return DVP_OK;
  if (!d_out_xy || !d_out_inf || !d_summary) return DVP_EINVAL;
  if (n && (!d_scalars || !d_xy || !d_work)) return DVP_EINVAL;
  DVP_TRY(seg_check_sizes(n, seg_ptr, n_seg));
  if (n && work_bytes < seg_layout(n, n_seg).total) return DVP_EINVAL;
  return msm_segments_dev(d_scalars, d_xy, d_inf, n, seg_ptr, n_seg, d_out_xy, d_out_inf, d_work, d_summary, (hipStream_t)stream);
}

extern "C" int dvp_msm_segments(const uint64_t* scalars, const uint64_t* xy, const uint8_t* inf, size_t n, const uint64_t* seg_ptr, size_t n_seg,
                                uint64_t* out_xy, uint8_t* out_inf) {
  if (!n_seg) return DVP_OK;
  if (!out_xy || !out_inf || (n && (!scalars || !xy))) return DVP_EINVAL;
  DVP_TRY(seg_check_sizes(n, seg_ptr, n_seg));
  if (!n) {
    memset(out_xy, 0, n_seg * 64);
    memset(out_inf, 1, n_seg);
    return DVP_OK;
  }
  const size_t work_bytes = seg_layout(n, n_seg).total;
  DevBuf ds, dp, di, dox, doi, dw, dsum;
  DVP_TRY(dp.up(xy, n * 64));
  DVP_TRY(di.up_opt(inf, n));
  DVP_TRY(dox.alloc(n_seg * 64));
  DVP_TRY(doi.alloc(n_seg));
  DVP_TRY(dw.alloc(work_bytes));
  DVP_TRY(dsum.alloc(16));
  DVP_TRY(points_check_strict(dp.p, di.p, n, 0));  // the points before the scalars, which go up only once both have passed
  DVP_TRY(scalars_in_range(scalars, n));
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(msm_segments_dev(ds.p, dp.p, di.p, n, seg_ptr, n_seg, dox.p, doi.p, dw.p, dsum.p, 0));
  DVP_TRY(dox.down(out_xy, n_seg * 64));
  return doi.down(out_inf, n_seg);
}

extern "C" int dvp_msm_segments_xsk233(const uint8_t* scalars, const uint8_t* enc, size_t n, const uint64_t* seg_ptr, size_t n_seg, uint8_t* out_enc) {
  if (!n_seg) return DVP_OK;
  if (!out_enc || (n && (!scalars || !enc))) return DVP_EINVAL;
  DVP_TRY(seg_check_sizes(n, seg_ptr, n_seg));
  if (!n) {  // the neutral element encodes as 30 zero bytes under every codec rule (codec.hip: k_encode)
    memset(out_enc, 0, n_seg * 30);
    return DVP_OK;
  }
  const size_t work_bytes = seg_layout(n, n_seg).total;
  DevBuf ds, dp, di, dox, doi, de, doe, dw, dsum;
  DVP_TRY(dp.alloc(n * 64));
  DVP_TRY(di.alloc(n));
  DVP_TRY(de.up(enc, n * 30));
  DVP_TRY(dox.alloc(n_seg * 64));
  DVP_TRY(doi.alloc(n_seg));
  DVP_TRY(doe.alloc(n_seg * 30));
  DVP_TRY(dw.alloc(work_bytes));
  DVP_TRY(dsum.alloc(16));
  DVP_TRY(decode_dev(de.as<uint8_t>(), n, dp.as<Aff>(), di.as<uint8_t>(), 0));
  // 32 little-endian bytes are the four limbs on the hosts this library runs on; the check reads each through a copy, whatever the alignment
  DVP_TRY(scalars_in_range(scalars, n));
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(msm_segments_dev(ds.p, dp.p, di.p, n, seg_ptr, n_seg, dox.p, doi.p, dw.p, dsum.p, 0));
  DVP_TRY(encode_dev(dox.as<Aff>(), doi.as<uint8_t>(), n_seg, doe.as<uint8_t>(), 0));
  return doe.down(out_enc, n_seg * 30);
}
