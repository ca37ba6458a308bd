// "Are these points the given multiples of G?" -- dvp_points_check_dlog*, the primitive behind dvp_srs_check_cache_dir (setup.hip).
// The claim P_i = s_i G for every i is linear in the group, so n claims fold into ONE multi-scalar multiplication of n + 1 points:
//     sum_i r_i P_i + (p - sum_i r_i s_i) G == O          <=>          sum_i r_i (P_i - s_i G) == O,
// with coefficients r_i that are fixed only after the points are (include/dvpari.h states the derivation and the error bound).
//   points_check_dev     every point reduced, on the curve, in E[r] (codec.hip); a bad point ends the call: the MSM never sees one
//   b3_leaves / _reduce  h = BLAKE3(xy bytes || infinity bytes) of the call's own copy of the points (blake3_tree.hip)
//   k_dlog_key           k = BLAKE3(key || h), one lane
//   k_dlog_rlc_prep      one lane per element: r_i = BLAKE3(k || LE64(i))[0..16) | 2^127 as MSM scalar i, block partials of sum r_i s_i
//   k_dlog_rlc_final     one block: MSM scalar n = p - sum r_i s_i, MSM base n = G (generator table, window 0, digit 1)
//   msm_affine_dev       the one-shot MSM, deferred completion
//   mulgen_dev + k_points_first_diff   only after a failed combination, or alone under DVP_DLOG_CHECK_EXACT: s_i G in batches of at
//                        most 2^20, compared with P_i; the smallest differing index by atomicMin
// The scalars may be the discrete logs of an SRS (trapdoor material): what held s_i, r_i s_i or their sums is zeroed on every exit.
#include <algorithm>

#include "blake3.h"
#include "blake3_dev.cuh"
#include "common.h"
#include "fr_block.cuh"
#include "host_api.h"
#include "k233.cuh"

namespace dvp {

namespace {
constexpr uint32_t DLOG_TPB = FR_SUM_LANES;
constexpr size_t DLOG_LOCATE_BATCH = (size_t)1 << 20;
constexpr size_t DLOG_MAX_N = ((size_t)1 << 27) - 1;  // n + 1 entries of the one-shot MSM
static_assert(DLOG_TPB == 256, "block_sum256");

// k = BLAKE3(key || h): 64 bytes, one compression
__global__ void __launch_bounds__(64) k_dlog_key(b3d::Words8 key, const uint32_t* __restrict__ h, uint32_t* __restrict__ k) {
  if (threadIdx.x != 0) return;
  constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  uint32_t cv[8], m[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    cv[i] = IV[i];
    m[i] = key.w[i];
    m[8 + i] = h[i];
  }
  b3d::compress(cv, m, 64u, 1u | 2u | 8u);  // CHUNK_START | CHUNK_END | ROOT
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = cv[i];
}

// r_i: the first 16 bytes of BLAKE3(k || LE64(i)) read little-endian, bit 127 set (non-zero, 127 hashed bits, below p).  40 bytes in:
// one compression.
__device__ __forceinline__ Fr dlog_coeff(const uint32_t k[8], uint64_t i) {
  constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  uint32_t cv[8], m[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cv[j] = IV[j];
    m[j] = k[j];
    m[8 + j] = 0;
  }
  m[8] = (uint32_t)i;
  m[9] = (uint32_t)(i >> 32);
  b3d::compress(cv, m, 40u, 1u | 2u | 8u);
  Fr r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r.v[j] = cv[j];
  r.v[3] |= 0x80000000u;
#pragma unroll
  for (int j = 4; j < 8; ++j) r.v[j] = 0;
  return r;
}

// level 1: block b takes elements b, b + B, b + 2B, ... in strides of the whole grid.  A scalar that is not below p is reported (err:
// the smallest such index) and taken as zero.
__global__ void __launch_bounds__(DLOG_TPB)
k_dlog_rlc_prep(const Fr* __restrict__ s, size_t n, const uint32_t* __restrict__ k, Fr* __restrict__ sc, Fr* __restrict__ part,
                unsigned long long* __restrict__ err) {
  __shared__ Fr sh[DLOG_TPB];
  uint32_t kw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) kw[j] = k[j];
  Fr acc = fr_zero();
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * DLOG_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * DLOG_TPB) {
    Fr si = s[i];
    if (!fr_is_canonical(si)) {
      atomicMin(err, (unsigned long long)i);
      si = fr_zero();
    }
    const Fr r = dlog_coeff(kw, (uint64_t)i);
    sc[i] = r;
    acc = fr_add(acc, fr_mul(fr_to_mont(r), si));  // Montgomery x canonical = the canonical product
  }
  const Fr total = block_sum256(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// level 2 (one block): the G entry of the MSM -- scalar p - sum r_i s_i, base G = tab[window 0, digit 1]
__global__ void __launch_bounds__(DLOG_TPB)
k_dlog_rlc_final(const Fr* __restrict__ part, uint32_t nparts, const Aff* __restrict__ tab, Fr* __restrict__ g_sc, Aff* __restrict__ g_base,
                 uint8_t* __restrict__ g_inf) {
  __shared__ Fr sh[DLOG_TPB];
  Fr acc = fr_zero();
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < nparts; i += DLOG_TPB) acc = fr_add(acc, part[i]);
  const Fr total = block_sum256(acc, sh);
  if (threadIdx.x == 0) {
    *g_sc = fr_neg(total);
    *g_base = tab[1];
    *g_inf = 0;
  }
}

// two affine vectors with infinity flags (either mask may be NULL = no point at infinity): *first = min(*first, base + i) over the
// i < n at which they differ.  Two points at infinity are equal whatever their coordinates hold.  Only the lowest differing lane of a
// wave touches memory, so equal vectors pay for no atomic.
__global__ void __launch_bounds__(256)
k_points_first_diff(const Aff* __restrict__ a, const uint8_t* __restrict__ ainf, const Aff* __restrict__ b, const uint8_t* __restrict__ binf,
                    size_t n, unsigned long long base, unsigned long long* __restrict__ first) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool diff = false;
  if (i < n) {
    const bool ai = ainf && ainf[i], bi = binf && binf[i];
    diff = ai != bi;
    if (!ai && !bi) {
      const Aff p = a[i], q = b[i];
      diff = !gf_eq(p.x, q.x) || !gf_eq(p.y, q.y);
    }
  }
  const unsigned long long bad = __ballot(diff);
  if (bad && (threadIdx.x & 63) == (unsigned)__ffsll((long long)bad) - 1) atomicMin(first, base + (unsigned long long)i);
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------------
// pts holds the call's copy of the points, [n x 64 xy | n infinity bytes]: first the stream h is the hash of, then -- the hash is done
// by then, in stream order -- the MSM's n + 1 bases, G written over the first bytes behind the xy.
struct DlogLayout {
  size_t sc, pts, minf, cls, cvs, cvs_tmp, part, loc_xy, loc_inf, ctrl, total;
  size_t hash_len, nchunks;
};
DlogLayout dlog_layout(size_t n) {
  const size_t N = n + 1;
  Carver c;
  DlogLayout l;
  l.hash_len = 65 * n;
  l.nchunks = (l.hash_len + 1023) / 1024;
  l.sc = c.take(32 * N);
  l.pts = c.take(std::max(64 * N, l.hash_len));
  l.minf = c.take(N);
  l.cls = c.take(n);
  l.cvs = c.take(32 * l.nchunks);
  l.cvs_tmp = c.take(b3_reduce_tmp_bytes(l.nchunks));
  l.part = c.take(32 * (size_t)FR_SUM_BLOCKS);
  const size_t batch = std::min(n, DLOG_LOCATE_BATCH);
  l.loc_xy = c.take(64 * batch);
  l.loc_inf = c.take(batch);
  // MSM x, y [0, 64) | MSM infinity u32 [64] | MSM scalar-range word u64 [72] | point summary 2 x u64 [80] | scalar word u64 [96] |
  // first difference u64 [104] | h [128, 160) | k [160, 192)
  l.ctrl = c.take(192);
  l.total = c.o;
  return l;
}
constexpr size_t CTRL_MSM_INF = 64, CTRL_MSM_ERR = 72, CTRL_SUMMARY = 80, CTRL_SC_ERR = 96, CTRL_DIFF = 104, CTRL_H = 128, CTRL_K = 160;

// zeroes what held scalars, products or their sums and waits for it, on every exit
struct DlogWipe {
  char* ws;
  const DlogLayout& l;
  size_t n;
  hipStream_t st;
  ~DlogWipe() {
    (void)hipMemsetAsync(ws + l.sc, 0, 32 * (n + 1), st);
    (void)hipMemsetAsync(ws + l.part, 0, 32 * (size_t)FR_SUM_BLOCKS, st);
    (void)hipStreamSynchronize(st);
  }
};

// step 5: s_i G against P_i, batch by batch in index order; *first_bad = the first index that differs, or -1.  DVP_EINVAL with the
// index of a scalar that is not below p.
int dlog_locate(const Fr* d_s, const Aff* d_xy, const uint8_t* d_inf, size_t n, char* ws, const DlogLayout& l, int64_t* first_bad,
                hipStream_t st) {
  Aff* loc_xy = (Aff*)(ws + l.loc_xy);
  uint8_t* loc_inf = (uint8_t*)(ws + l.loc_inf);
  unsigned long long* d_first = (unsigned long long*)(ws + CTRL_DIFF + l.ctrl);
  *first_bad = -1;
  for (size_t base = 0; base < n; base += DLOG_LOCATE_BATCH) {
    const size_t cnt = std::min(DLOG_LOCATE_BATCH, n - base);
    const int rc = mulgen_dev(d_s + base, cnt, loc_xy, loc_inf, st);  // waits; the index it reports counts from the batch's start
    if (rc == DVP_EINVAL) g_last_error_index += (int64_t)base;
    DVP_TRY(rc);
    DVP_HIP(hipMemsetAsync(d_first, 0xff, 8, st));
    DVP_LAUNCH(k_points_first_diff, dim3(cdiv(cnt, 256)), dim3(256), 0, st, (const Aff*)loc_xy, (const uint8_t*)loc_inf, d_xy + base,
               d_inf ? d_inf + base : (const uint8_t*)nullptr, cnt, (unsigned long long)base, d_first);
    DVP_HIP(hipGetLastError());
    unsigned long long first = ~0ull;
    DVP_HIP(hipMemcpyAsync(&first, d_first, 8, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipStreamSynchronize(st));
    if (first != ~0ull) {
      *first_bad = (int64_t)first;
      return DVP_OK;
    }
  }
  return DVP_OK;
}
}  // namespace

size_t dlog_check_work_bytes(size_t n) { return n && n <= DLOG_MAX_N ? dlog_layout(n).total : 0; }

// the primitive on device buffers; key = the 32 bytes k is derived from (the caller has resolved seed == NULL); d_work holds
// dlog_check_work_bytes(n) bytes
int dlog_check_dev(const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, const uint8_t key[32], uint32_t flags, void* d_work,
                   dvp_dlog_report* rep, hipStream_t st) {
  rep->verdict = 0;
  rep->path = (flags & DVP_DLOG_CHECK_EXACT) ? DVP_DLOG_PATH_EXACT : DVP_DLOG_PATH_COMBINED;
  rep->first_bad = -1;
  rep->point_class = 0;
  if (!n) return DVP_OK;
  if (n > DLOG_MAX_N) return DVP_EINVAL;
  const DlogLayout l = dlog_layout(n);
  char* ws = (char*)d_work;
  char* ctrl = ws + l.ctrl;
  const Fr* s = (const Fr*)d_scalars;
  const Aff* xy = (const Aff*)d_xy;
  const uint8_t* inf = (const uint8_t*)d_inf;
  // ---- step 1: well-formed points, or nothing further ----
  uint8_t* cls = (uint8_t*)(ws + l.cls);
  DVP_TRY(points_check_dev(xy, inf, n, cls, ctrl + CTRL_SUMMARY, st));
  unsigned long long summary[2] = {~0ull, 0};
  DVP_HIP(hipMemcpyAsync(summary, ctrl + CTRL_SUMMARY, 16, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  if (summary[0] != ~0ull) {
    rep->verdict = DVP_DLOG_BAD_POINT;
    rep->first_bad = (int64_t)summary[0];
    DVP_HIP(hipMemcpy(&rep->point_class, cls + summary[0], 1, hipMemcpyDeviceToHost));
    return DVP_OK;
  }
  DlogWipe wipe{ws, l, n, st};
  if (!(flags & DVP_DLOG_CHECK_EXACT)) {
    // ---- step 2: h, then k ----
    char* pts = ws + l.pts;
    uint8_t* minf = (uint8_t*)(ws + l.minf);
    DVP_HIP(hipMemcpyAsync(pts, xy, 64 * n, hipMemcpyDeviceToDevice, st));
    if (inf) {
      DVP_HIP(hipMemcpyAsync(pts + 64 * n, inf, n, hipMemcpyDeviceToDevice, st));
      DVP_HIP(hipMemcpyAsync(minf, inf, n, hipMemcpyDeviceToDevice, st));
    } else {
      DVP_HIP(hipMemsetAsync(pts + 64 * n, 0, n, st));
      DVP_HIP(hipMemsetAsync(minf, 0, n, st));
    }
    uint32_t* h = (uint32_t*)(ctrl + CTRL_H);
    uint32_t* k = (uint32_t*)(ctrl + CTRL_K);
    if (l.nchunks == 1) {
      DVP_TRY(b3_single_chunk_dev((const uint8_t*)pts, l.hash_len, h, st));
    } else {
      uint32_t* cvs = (uint32_t*)(ws + l.cvs);
      DVP_TRY(b3_leaves_dev((const uint8_t*)pts, l.hash_len, 0, cvs, st));
      DVP_TRY(b3_reduce_dev(cvs, l.nchunks, (uint32_t*)(ws + l.cvs_tmp), h, st));
    }
    b3d::Words8 kw;
    memcpy(kw.w, key, 32);
    DVP_LAUNCH(k_dlog_key, dim3(1), dim3(64), 0, st, kw, (const uint32_t*)h, k);
    // ---- step 3: coefficients, sum r_i s_i, the G entry ----
    const Aff* tab;
    DVP_TRY(gen_table(&tab, st));
    Fr* sc = (Fr*)(ws + l.sc);
    Fr* part = (Fr*)(ws + l.part);
    unsigned long long* sc_err = (unsigned long long*)(ctrl + CTRL_SC_ERR);
    DVP_HIP(hipMemsetAsync(sc_err, 0xff, 8, st));
    const uint32_t nparts = std::min<uint32_t>(cdiv(n, DLOG_TPB), FR_SUM_BLOCKS);
    DVP_LAUNCH(k_dlog_rlc_prep, dim3(nparts), dim3(DLOG_TPB), 0, st, s, n, (const uint32_t*)k, sc, part, sc_err);
    DVP_LAUNCH(k_dlog_rlc_final, dim3(1), dim3(DLOG_TPB), 0, st, (const Fr*)part, nparts, tab, sc + n, (Aff*)pts + n, minf + n);
    DVP_HIP(hipGetLastError());
    // ---- step 4: the MSM over n + 1 points ----
    uint32_t* out_inf = (uint32_t*)(ctrl + CTRL_MSM_INF);
    unsigned long long* msm_err = (unsigned long long*)(ctrl + CTRL_MSM_ERR);
    DVP_TRY(msm_affine_dev(sc, pts, minf, n + 1, MsmOut{ctrl, out_inf, nullptr, nullptr, nullptr, 0, msm_err}, st));
    uint32_t res[12];  // the control block from the MSM's infinity flag to the scalar word
    DVP_HIP(hipMemcpyAsync(res, ctrl + CTRL_MSM_INF, sizeof res, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipStreamSynchronize(st));
    unsigned long long bad_scalar, bad_msm;
    memcpy(&bad_scalar, (char*)res + (CTRL_SC_ERR - CTRL_MSM_INF), 8);
    memcpy(&bad_msm, (char*)res + (CTRL_MSM_ERR - CTRL_MSM_INF), 8);
    if (bad_scalar != ~0ull) {
      g_last_error_index = (int64_t)bad_scalar;
      return DVP_EINVAL;
    }
    if (bad_msm != ~0ull) return DVP_EHIP;  // every MSM scalar was written below p by the two kernels above
    if (res[0] == 1u) return DVP_OK;        // the combination is O
    rep->path = DVP_DLOG_PATH_LOCATED;
  }
  // ---- step 5: locate ----
  DVP_TRY(dlog_locate(s, xy, inf, n, ws, l, &rep->first_bad, st));
  if (rep->first_bad >= 0) rep->verdict = DVP_DLOG_WRONG;
  // (a combination that is not O over vectors that agree entry for entry cannot happen: both say what sum r_i (P_i - s_i G) is)
  else if (rep->path == DVP_DLOG_PATH_LOCATED) return DVP_EHIP;
  return DVP_OK;
}

// key of a call without a seed
static void dlog_default_key(uint8_t key[32]) {
  static const char tag[] = "dv-pari dlog check v1";
  b3::hash((const uint8_t*)tag, sizeof(tag) - 1, key);
}

}  // namespace dvp

using namespace dvp;

extern "C" size_t dvp_points_check_dlog_work_bytes(size_t n) { return dlog_check_work_bytes(n); }

extern "C" int dvp_points_check_dlog_dev(const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, const uint8_t* seed, uint32_t flags,
                                         void* d_work, size_t work_bytes, dvp_dlog_report* report, void* stream) {
  if (!report || (flags & ~DVP_DLOG_CHECK_EXACT)) return DVP_EINVAL;
  if (n && (!d_scalars || !d_xy || !d_work || n > DLOG_MAX_N || work_bytes < dlog_check_work_bytes(n) || ((uintptr_t)d_work & 255))) return DVP_EINVAL;
  uint8_t key[32];
  if (seed) memcpy(key, seed, 32);
  else dlog_default_key(key);
  return dlog_check_dev(d_scalars, d_xy, d_inf, n, key, flags, d_work, report, (hipStream_t)stream);
}

extern "C" int dvp_points_check_dlog(const uint64_t* scalars, const uint64_t* xy, const uint8_t* inf, size_t n, const uint8_t* seed, uint32_t flags,
                                     dvp_dlog_report* report) {
  if (!report || (flags & ~DVP_DLOG_CHECK_EXACT)) return DVP_EINVAL;
  if (n && (!scalars || !xy || n > DLOG_MAX_N)) return DVP_EINVAL;
  if (!n) return dvp_points_check_dlog_dev(nullptr, nullptr, nullptr, 0, seed, flags, nullptr, 0, report, nullptr);
  DVP_TRY(scalars_in_range(scalars, n));
  DevBuf ds, dp, di, work;
  // the device copy of the scalars is zeroed before it goes back to the allocator, on every exit
  struct Wipe {
    DevBuf& b;
    ~Wipe() {
      if (b.p) (void)hipMemset(b.p, 0, b.bytes);
      (void)hipDeviceSynchronize();
    }
  } wipe{ds};
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(dp.up(xy, n * 64));
  DVP_TRY(di.up_opt(inf, n));
  const size_t wb = dlog_check_work_bytes(n);
  DVP_TRY(work.alloc(wb));
  return dvp_points_check_dlog_dev(ds.p, dp.p, di.p, n, seed, flags, work.p, wb, report, nullptr);
}
