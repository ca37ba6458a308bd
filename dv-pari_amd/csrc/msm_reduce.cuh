// MSM bucket reducers behind the pair rounds: the block shape of the EC kernels (EC_TPB, EC_LDS*), MergeMul, the fan-in-K reducer
// (k_accum_affine, k_accum_affine_fast, k_accum_affine_rest, k_accum_proj), the per-bucket leftovers (k_bucket_pairs, k_bucket_rest) and the
// multi-squaring tables of the fast inversion (k_build_sqr_tables, gf_sqr_tables).  Part of msm.hip's translation unit: msm.hip
// includes it, and its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include <mutex>

#include "common.h"
#include "k233.cuh"

namespace dvp {

// EC kernels on the Karatsuba LDS multiplier: 256-thread blocks, 4 x 8 KB of half tables; the quad-cooperative
// flavours (latency-bound stages) keep the 16 KB comb tables
constexpr int EC_TPB = 256;
constexpr unsigned EC_LDS = (EC_TPB / 64) * GF_LDSK_BYTES_PER_WAVE;
constexpr unsigned EC_LDS_Q = (EC_TPB / 64) * GF_LDS_BYTES_PER_WAVE;
constexpr uint32_t MERGE_HEX_MAX = 8192;    // additions per level up to which 16 lanes per addition win: one chip-full of rows at two waves per SIMD (measured: 0 / 4096 / 8192 -> 21.01 / 20.94 / 20.87 ms per proof)
constexpr uint32_t MERGE_QUAD_MAX = 16384;  // additions per level up to which 4 lanes per addition win (measured: 35 us vs 41 us at 16384)

// the multiplier flavours behind one name: init, and which lane of a group stores
template <class LT> struct MergeMul;
template <> struct MergeMul<GfLdsK> { static __device__ __forceinline__ GfLdsK init(char* l) { return gf_ldsk_init(l); } static __device__ __forceinline__ bool lead(const GfLdsK&) { return true; } };
template <> struct MergeMul<GfLdsQ> { static __device__ __forceinline__ GfLdsQ init(char* l) { return gf_ldsq_init(l); } static __device__ __forceinline__ bool lead(const GfLdsQ& c) { return c.r == 0; } };
template <> struct MergeMul<GfLdsH> { static __device__ __forceinline__ GfLdsH init(char* l) { return gf_ldsh_init(l); } static __device__ __forceinline__ bool lead(const GfLdsH& c) { return c.r == 0; } };
// ---- segmented reduction by fan-in K ----------------------------------------------------------------
// largest key with toff[key] <= tid (toff has nkeys+1 entries, toff[nkeys] = total > tid)
__device__ __forceinline__ uint32_t find_key(const uint32_t* __restrict__ toff, uint32_t nkeys, uint32_t tid) {
  uint32_t lo = 0, hi = nkeys;  // invariant: toff[lo] <= tid < toff[hi]
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (toff[mid] <= tid) lo = mid; else hi = mid;
  }
  return lo;
}

// QUAD: one task per quad of lanes (quad-cooperative products, gf233.cuh).  A small MSM -- config #2's 2^16 points, the shard
// of one rank of an 8-way split -- has fewer reducer tasks than the chip has lanes and its fan-in-K chains are pure
// latency: 2.2x shorter per addition this way (the same trade k_merge<true> makes for the deep merge levels).
constexpr uint32_t ACCUM_QUAD_MAX = 49152;  // tasks: 4 lanes each = one chip-full of 3 blocks per CU
constexpr uint32_t ACCUM_HEX_MAX = 32768;   // tasks of the reducer's last level up to which 16 lanes per task win
template <bool INDIRECT, bool QUAD>
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_accum_affine(const Aff* __restrict__ bases, const uint32_t* __restrict__ items, const uint32_t* __restrict__ cnt,
               const uint32_t* __restrict__ off, const uint32_t* __restrict__ toff, uint32_t nkeys, uint32_t K,
               Ld* __restrict__ out, uint32_t sign_mask) {
  extern __shared__ char lds_raw[];
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (QUAD) tid >>= 2;
  if (tid >= toff[nkeys]) return;
  uint32_t key = find_key(toff, nkeys, tid);
  uint32_t j = tid - toff[key];
  uint32_t start = off[key] + j * K;
  uint32_t len = min(K, cnt[key] - j * K);
  // INDIRECT: bases gathered through the sorted index list; otherwise `bases` is the compacted output of
  // the affine rounds, where x == 0 marks infinity
  auto item_point = [&](uint32_t v) -> Aff {  // table entry named by a sorted item; bit 31 (signed flavours) = subtract it
    Aff q = bases[v & ~sign_mask];
    if (v & sign_mask) q.y = gf_add(q.y, q.x);
    return q;
  };
  Aff first = INDIRECT ? item_point(items[start]) : bases[start];
  Ld acc = (!INDIRECT && gf_is_zero(first.x)) ? ld_infinity() : ld_from_aff(first);
  if (QUAD) {
    GfLdsQ L = gf_ldsq_init(lds_raw);
#pragma unroll 1
    for (uint32_t t = 1; t < len; ++t) {
      Aff q = INDIRECT ? item_point(items[start + t]) : bases[start + t];
      if (!INDIRECT && gf_is_zero(q.x)) continue;
      ld_madd_ip(acc, q, L);
    }
    if (L.r == 0) out[tid] = acc;
  } else {
    GfLdsK L = gf_ldsk_init(lds_raw);
#pragma unroll 1
    for (uint32_t t = 1; t < len; ++t) {
      Aff q = INDIRECT ? item_point(items[start + t]) : bases[start + t];
      if (!INDIRECT && gf_is_zero(q.x)) continue;
      ld_madd_ip(acc, q, L);
    }
    out[tid] = acc;
  }
}

// The same tasks without the exceptional branches (round 6; what k_bucket_pairs does for the fixed-base sizes): the first two entries
// are two AFFINE points (ld_add_aff_aff: Z1 = 1, 5M + 3S instead of 8M + 5S), the others go through ld_madd_fast; a task that meets
// an exceptional pair -- an infinity marker first, equal x -- goes on a list that k_accum_affine_rest redoes with the general
// formulas.  The general kernel kept the accumulator's exceptional paths alive on every lane: 253 VGPRs and 312-444 B of scratch
// per lane at two waves per SIMD.
template <bool INDIRECT, bool QUAD>
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_accum_affine_fast(const Aff* __restrict__ bases, const uint32_t* __restrict__ items, const uint32_t* __restrict__ cnt,
                    const uint32_t* __restrict__ off, const uint32_t* __restrict__ toff, uint32_t nkeys, uint32_t K,
                    Ld* __restrict__ out, uint32_t sign_mask, uint32_t* __restrict__ rest_n, uint32_t* __restrict__ rest) {
  extern __shared__ char lds_raw[];
  using LT = typename std::conditional<QUAD, GfLdsQ, GfLdsK>::type;
  LT L = MergeMul<LT>::init(lds_raw);
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (QUAD) tid >>= 2;
  if (tid >= toff[nkeys]) return;
  const uint32_t key = find_key(toff, nkeys, tid);
  const uint32_t j = tid - toff[key];
  const uint32_t start = off[key] + j * K;
  const uint32_t len = min(K, cnt[key] - j * K);
  auto point = [&](uint32_t t) -> Aff {
    if (!INDIRECT) return bases[start + t];
    const uint32_t v = items[start + t];
    Aff q = bases[v & ~sign_mask];
    if (v & sign_mask) q.y = gf_add(q.y, q.x);
    return q;
  };
  const Aff first = point(0);
  bool ok = INDIRECT || !gf_is_zero(first.x);
  Ld acc = ld_from_aff(first);
  if (ok && len > 1) {
    const Aff q = point(1);
    ok = (INDIRECT || !gf_is_zero(q.x)) && !gf_eq(first.x, q.x);
    if (ok) ld_add_aff_aff(first, q, acc, L);
  }
#pragma unroll 1
  for (uint32_t t = 2; t < len && ok; ++t) {
    const Aff q = point(t);
    if (!INDIRECT && gf_is_zero(q.x)) continue;
    ok = ld_madd_fast(acc, q, L);
  }
  if (!MergeMul<LT>::lead(L)) return;
  if (ok)
    out[tid] = acc;
  else
    rest[atomicAdd(rest_n, 1u)] = tid;
}
// the listed tasks again, general formulas (one thread per task)
template <bool INDIRECT>
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_accum_affine_rest(const Aff* __restrict__ bases, const uint32_t* __restrict__ items, const uint32_t* __restrict__ cnt,
                    const uint32_t* __restrict__ off, const uint32_t* __restrict__ toff, uint32_t nkeys, uint32_t K,
                    Ld* __restrict__ out, uint32_t sign_mask, const uint32_t* __restrict__ rest_n, const uint32_t* __restrict__ rest) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= *rest_n) return;
  const uint32_t tid = rest[r];
  const uint32_t key = find_key(toff, nkeys, tid);
  const uint32_t j = tid - toff[key];
  const uint32_t start = off[key] + j * K;
  const uint32_t len = min(K, cnt[key] - j * K);
  auto point = [&](uint32_t t) -> Aff {
    if (!INDIRECT) return bases[start + t];
    const uint32_t v = items[start + t];
    Aff q = bases[v & ~sign_mask];
    if (v & sign_mask) q.y = gf_add(q.y, q.x);
    return q;
  };
  const Aff first = point(0);
  Ld acc = (!INDIRECT && gf_is_zero(first.x)) ? ld_infinity() : ld_from_aff(first);
#pragma unroll 1
  for (uint32_t t = 1; t < len; ++t) {
    const Aff q = point(t);
    if (!INDIRECT && gf_is_zero(q.x)) continue;
    ld_madd_ip(acc, q, L);
  }
  out[tid] = acc;
}

// GROUP = lanes per task: 1, 4 (a quad) or 16 (a DPP row: the last level of a small MSM -- one or two additions per bucket, fewer
// tasks than the chip has rows -- is pure latency, and the sixteen-lane product is ~290 instructions against the quad's ~450)
template <int GROUP>
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_accum_proj(const Ld* __restrict__ in, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
             const uint32_t* __restrict__ toff, uint32_t nkeys, uint32_t K, Ld* __restrict__ out) {
  extern __shared__ char lds_raw[];
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  tid /= (uint32_t)GROUP;
  if (tid >= toff[nkeys]) return;
  uint32_t key = find_key(toff, nkeys, tid);
  uint32_t j = tid - toff[key];
  uint32_t start = off[key] + j * K;
  uint32_t len = min(K, cnt[key] - j * K);
  Ld acc = in[start];
  using LT = typename std::conditional<GROUP == 16, GfLdsH, typename std::conditional<GROUP == 4, GfLdsQ, GfLdsK>::type>::type;
  LT L = MergeMul<LT>::init(lds_raw);
#pragma unroll 1
  for (uint32_t t = 1; t < len; ++t) {
    if (!ld_add_nodbl(acc, in[start + t], L)) {  // acc == the entry: double a copy read back
      acc = in[start + t];
      acc = ld_dbl(acc, L);
    }
  }
  if (MergeMul<LT>::lead(L)) out[tid] = acc;
}

// ---- what the pair rounds leave, one thread per BUCKET (fixed-base sizes: the rounds stop with 1-4 points per bucket) ----
// k_accum_affine gives every chunk of K entries a task and runs it as a serial chain of general mixed additions at two waves
// per SIMD (253 VGPRs: the exceptional branches of ld_madd_ip), behind a scan and a binary search per task and in front of a
// gather into the bucket array.  With the signed windows the load is bimodal -- the narrow windows reach only the lower half of
// the keys, which end the rounds with three points per bucket where the upper half has one -- so contiguous keys do the same
// work and a thread per bucket diverges no more than a thread per task did.  Here: the first two entries are two AFFINE
// points, so the mixed addition's Z1 = 1 and three of its eight products vanish (ld_add_aff_aff, 5M + 3S); further entries go
// through the mixed addition stripped of its exceptional branches (ld_madd_fast), straight into the bucket array (two waves
// per SIMD: 222 VGPRs; at three the loop spills 240 B per lane and the heavy half of the keys -- 1 024 workgroups -- is 1.33
// chip-fulls instead of exactly two: measured equal).  A bucket that meets an exceptional pair (an infinity marker first, equal x) goes on a list that k_bucket_rest
// redoes from its first entry with the general formulas.  No task scan, no search, no gather.
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_bucket_pairs(const Aff* __restrict__ pts, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, uint32_t nkeys,
               Ld* __restrict__ A, uint32_t* __restrict__ rest_n, uint32_t* __restrict__ rest) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= nkeys) return;
  const uint32_t c = cnt[key];
  if (c == 0) {
    A[key] = ld_infinity();
    return;
  }
  const uint32_t o = off[key];
  const Aff p = pts[o];
  if (c == 1) {
    A[key] = gf_is_zero(p.x) ? ld_infinity() : ld_from_aff(p);  // x == 0 marks infinity
    return;
  }
  Aff q = pts[o + 1];
  bool ok = !(gf_is_zero(p.x) || gf_is_zero(q.x) || gf_eq(p.x, q.x));
  Ld r;
  if (ok) {
    ld_add_aff_aff(p, q, r, L);
#pragma unroll 1
    for (uint32_t t = 2; t < c && ok; ++t) {
      q = pts[o + t];
      if (gf_is_zero(q.x)) continue;
      ok = ld_madd_fast(r, q, L);
    }
  }
  if (ok)
    A[key] = r;
  else
    rest[atomicAdd(rest_n, 1u)] = key;
}
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_bucket_rest(const Aff* __restrict__ pts, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
              const uint32_t* __restrict__ rest_n, const uint32_t* __restrict__ rest, Ld* __restrict__ A) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= *rest_n) return;
  const uint32_t key = rest[tid];
  const uint32_t c = cnt[key], o = off[key];
  const Aff first = pts[o];
  Ld acc = gf_is_zero(first.x) ? ld_infinity() : ld_from_aff(first);
#pragma unroll 1
  for (uint32_t t = 1; t < c; ++t) {
    const Aff q = pts[o + t];
    if (gf_is_zero(q.x)) continue;
    ld_madd_ip(acc, q, L);
  }
  A[key] = acc;
}

// ---- multi-squaring tables for the fast inversion (gf233.cuh) ----------------------------------------
__global__ void __launch_bounds__(256)
k_build_sqr_tables(Gf* __restrict__ tabs /* t29 | t58 | t116 | th | t14 | t7, 30 x 256 entries each */) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= 6 * 30 * 256) return;
  uint32_t which = tid / (30 * 256), e = tid - which * 30 * 256, pos = e >> 8, byte = e & 255;
  Gf v = gf_zero();
  v.w[pos >> 2] = byte << (8 * (pos & 3));
  if (pos == 29) v.w[7] &= 0x1FFu;  // bits >= 233 never occur in a reduced element
  if (which == 3) {
    tabs[tid] = gf_halftrace(v);
    return;
  }
  const int k = which == 0 ? 29 : which == 1 ? 58 : which == 2 ? 116 : which == 4 ? 14 : 7;
  tabs[tid] = gf_sqr_n(v, k);
}
static PerDevice<Gf> g_sqr_tab;
int gf_sqr_tables(GfSqrTables* out, hipStream_t st) {
  Gf* tab;
  DVP_TRY(g_sqr_tab.get(&tab, [&](Gf** t) -> int {
    DVP_HIP(hipMalloc((void**)t, (size_t)6 * 30 * 256 * sizeof(Gf)));
    DVP_LAUNCH(k_build_sqr_tables, dim3(cdiv(6 * 30 * 256, 256)), dim3(256), 0, st, *t);
    DVP_HIP(hipGetLastError());
    DVP_HIP(hipStreamSynchronize(st));
    return DVP_OK;
  }));
  out->t29 = tab;
  out->t58 = tab + 30 * 256;
  out->t116 = tab + 2 * 30 * 256;
  out->th = tab + 3 * 30 * 256;
  const long long tabs = tune().gf_inv_tabs;  // 0: the three long runs only (rounds 1-5), 1: + the run of 14, 2: + the run of 7
  out->t14 = tabs >= 1 ? tab + 4 * 30 * 256 : nullptr;
  out->t7 = tabs >= 2 ? tab + 5 * 30 * 256 : nullptr;
  return DVP_OK;
}

}  // namespace dvp
