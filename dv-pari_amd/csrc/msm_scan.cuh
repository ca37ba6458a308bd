// MSM: exclusive scans of u32 arrays (k_scan_*; scan_exclusive_pad2 for the sorts' bucket offsets, scan_exclusive_div for the
// per-round bookkeeping of the bucket reducers) and the block-level scan the sorts share (block_scan_waves).  Part of msm.hip's
// translation unit: msm.hip includes it, and its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include "common.h"

namespace dvp {

// ---- exclusive scan of u32 (3 kernels; up to 4096*1024 elements) ---------------------------------
constexpr int SCAN_TPB = 256, SCAN_EPT = 4, SCAN_BLK = SCAN_TPB * SCAN_EPT;

// Exclusive scan of one value per thread over a block of NW waves (<= 16): wave-level inclusive scans by shuffles, the wave totals
// scanned by the first wave, two barriers (+ one so that `sh` can be reused at once).  The first version was Hillis-Steele over the
// whole block in LDS -- two barriers per doubling step, 16-20 barriers of 16 waves for a 1024-thread block -- and those barriers
// were most of the 19 us a staged-scatter block took.  sh: >= 32 words.
template <int NW>
__device__ __forceinline__ uint32_t block_scan_waves(uint32_t v, uint32_t* total, uint32_t* sh) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[w] = x;
  __syncthreads();
  if (w == 0) {
    uint32_t z = lane < NW ? sh[lane] : 0u;
#pragma unroll
    for (int o = 1; o < NW; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)z, o);
      if (lane >= o) z += y;
    }
    if (lane < NW) sh[16 + lane] = z;
  }
  __syncthreads();
  const uint32_t base = w ? sh[16 + w - 1] : 0u;
  *total = sh[16 + NW - 1];
  __syncthreads();
  return base + x - v;
}
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total, uint32_t* sh) {
  return block_scan_waves<SCAN_TPB / 64>(v, total, sh);  // sh: 256 entries
}

// every count is rounded up to even first (both sorts: buckets then start at even positions of the sorted
// item list, so the list read as uint2 pairs IS the first pair round's descriptor array, see k_post_sort)
__global__ void __launch_bounds__(SCAN_TPB) k_scan_local(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                         uint32_t* __restrict__ bsum, uint32_t m) {
  __shared__ uint32_t sh[SCAN_TPB];
  uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_EPT;
  uint32_t v[SCAN_EPT], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k) {
    v[k] = (base + k < m) ? in[base + k] : 0;
    v[k] = (v[k] + 1u) & ~1u;
    s += v[k];
  }
  uint32_t tot;
  uint32_t ex = block_exclusive_scan(s, &tot, sh);
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k) {
    if (base + k < m) out[base + k] = ex;
    ex += v[k];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// the same with a division fused in: v = ceil(in / K) (outputs per bucket of a pair round, tasks per bucket of the
// fan-in-K reducer) is written to vout and scanned
__global__ void __launch_bounds__(SCAN_TPB) k_scan_local_div(const uint32_t* __restrict__ in, uint32_t K, uint32_t* __restrict__ vout,
                                                             uint32_t* __restrict__ out, uint32_t* __restrict__ bsum, uint32_t m) {
  __shared__ uint32_t sh[SCAN_TPB];
  uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_EPT;
  uint32_t v[SCAN_EPT], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k) {
    v[k] = (base + k < m) ? (in[base + k] + K - 1) / K : 0;
    if (base + k < m) vout[base + k] = v[k];
    s += v[k];
  }
  uint32_t tot;
  uint32_t ex = block_exclusive_scan(s, &tot, sh);
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k) {
    if (base + k < m) out[base + k] = ex;
    ex += v[k];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(SCAN_TPB) k_scan_bsums(uint32_t* __restrict__ bsum, uint32_t nb, uint32_t* total_out) {
  __shared__ uint32_t sh[SCAN_TPB];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += SCAN_TPB) {
    uint32_t idx = base + threadIdx.x;
    uint32_t v = idx < nb ? bsum[idx] : 0;
    uint32_t tot;
    uint32_t ex = block_exclusive_scan(v, &tot, sh);
    if (idx < nb) bsum[idx] = ex + carry;
    carry += tot;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(SCAN_TPB) k_scan_add(uint32_t* __restrict__ out, const uint32_t* __restrict__ bsum, uint32_t m) {
  uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_EPT;
  uint32_t add = bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k)
    if (base + k < m) out[base + k] += add;
}

// Short inputs (<= SCAN_FOLD_NB blocks of 1 024 values: the bucket arrays of a small MSM) fold the scan of the block sums into the last
// launch: every block adds up the raw sums of the blocks in front of it itself (a uniform loop over <= 64 words) -- two dependent
// launches per scan instead of three (round 6: a one-shot MSM of 2^16 points scans its 24 576 counts four times)
constexpr uint32_t SCAN_FOLD_NB = 64;
__global__ void __launch_bounds__(SCAN_TPB) k_scan_add_fold(uint32_t* __restrict__ out, const uint32_t* __restrict__ bsum_raw, uint32_t m,
                                                           uint32_t* __restrict__ total_out) {
  uint32_t add = 0;
  for (uint32_t b = 0; b < blockIdx.x; ++b) add += bsum_raw[b];
  const uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_EPT;
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k)
    if (base + k < m) out[base + k] += add;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = add + bsum_raw[blockIdx.x];
}

// out[0..m) = exclusive scan of in[0..m) rounded up to even; out[m] = total
static int scan_exclusive_pad2(const uint32_t* in, uint32_t* out, uint32_t m, uint32_t* bsum, hipStream_t st) {
  uint32_t nb = cdiv(m, SCAN_BLK);
  DVP_LAUNCH(k_scan_local, dim3(nb), dim3(SCAN_TPB), 0, st, in, out, bsum, m);
  if (nb <= SCAN_FOLD_NB)
    DVP_LAUNCH(k_scan_add_fold, dim3(nb), dim3(SCAN_TPB), 0, st, out, bsum, m, out + m);
  else {
    DVP_LAUNCH(k_scan_bsums, dim3(1), dim3(SCAN_TPB), 0, st, bsum, nb, out + m);
    DVP_LAUNCH(k_scan_add, dim3(nb), dim3(SCAN_TPB), 0, st, out, bsum, m);
  }
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

// vout[i] = ceil(in[i] / K); out = exclusive scan of vout (out[m] = total): the per-round bookkeeping of the bucket reducers
static int scan_exclusive_div(const uint32_t* in, uint32_t K, uint32_t* vout, uint32_t* out, uint32_t m, uint32_t* bsum, hipStream_t st) {
  uint32_t nb = cdiv(m, SCAN_BLK);
  DVP_LAUNCH(k_scan_local_div, dim3(nb), dim3(SCAN_TPB), 0, st, in, K, vout, out, bsum, m);
  if (nb <= SCAN_FOLD_NB)
    DVP_LAUNCH(k_scan_add_fold, dim3(nb), dim3(SCAN_TPB), 0, st, out, bsum, m, out + m);
  else {
    DVP_LAUNCH(k_scan_bsums, dim3(1), dim3(SCAN_TPB), 0, st, bsum, nb, out + m);
    DVP_LAUNCH(k_scan_add, dim3(nb), dim3(SCAN_TPB), 0, st, out, bsum, m);
  }
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

}  // namespace dvp
