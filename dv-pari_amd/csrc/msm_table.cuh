// MSM fixed-base tables: k_frob_table (rows tau^(o_w) P, the tau-adic aligned windows) and k_dbl_table (rows 2^(o_w) P, the signed
// binary windows).  Built once per context by msm_fixed_build (msm.hip).  Part of msm.hip's translation unit: msm.hip includes it, and
// its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include "k233.cuh"

namespace dvp {

// pre-rotated base table for the fixed-base mode: T[w][i] = tau^(o_w)(P_i), o_w = first digit of window w
// (windows 0 .. n_narrow-1 are c-1 digits wide, the rest c)
__global__ void __launch_bounds__(256)
k_frob_table(const Aff* __restrict__ bases, uint32_t n, int FX_C, int FX_W, int n_narrow, Aff* __restrict__ table) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Aff p = bases[i];
  table[i] = p;
#pragma unroll 1
  for (int w = 1; w < FX_W; ++w) {
    int width = (w - 1) < n_narrow ? FX_C - 1 : FX_C;
    p.x = gf_sqr_n(p.x, width);
    p.y = gf_sqr_n(p.y, width);
    table[(size_t)w * n + i] = p;
  }
}

// signed aligned windows: T[w][i] = 2^(o_w) P_i, o_w = first bit of window w (the n_narrow low windows are c - 1 bits wide).
// The ~222 doublings of a base run in Lopez-Dahab coordinates (3M + 5S each) and the W - 1 row snapshots of the base share ONE
// inversion (Montgomery's trick over their Z's): ~0.9 k field products per base.  The first version doubled in affine
// coordinates, one table-driven inversion per doubling: 4.2 k products per base, 0.30 s per table at 2^20 constraints and 75 % of
// the profiled GPU time of a short run (prover open).  zs / pre: thread-private scratch in HBM, (W - 1) x n field elements each
// ([row][base]: coalesced), freed after the build.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_dbl_table(const Aff* __restrict__ bases, uint32_t n, int c, int W, int n_narrow, GfSqrTables T, Aff* __restrict__ table, Gf* __restrict__ zs,
            Gf* __restrict__ pre) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Aff p0 = bases[i];
  table[i] = p0;
  Ld p = ld_from_aff(p0);
  Gf run = gf_one();
#pragma unroll 1
  for (int w = 1; w < W; ++w) {
    const int width = (w - 1) < n_narrow ? c - 1 : c;  // row w starts where window w - 1 ends
#pragma unroll 1
    for (int k = 0; k < width; ++k) p = ld_dbl(p, L);
    Aff raw;
    raw.x = p.X;
    raw.y = p.Y;
    table[(size_t)w * n + i] = raw;  // normalised below
    zs[(size_t)(w - 1) * n + i] = p.Z;
    pre[(size_t)(w - 1) * n + i] = run;
    run = gf_mul(run, p.Z, L);
  }
  Gf inv = gf_inv_fast(run, T, L);  // a base of E[r] never doubles to infinity: every Z is non-zero
#pragma unroll 1
  for (int w = W - 1; w >= 1; --w) {
    const Gf z = zs[(size_t)(w - 1) * n + i];
    Gf zi, inv_next;
    gf_mul2(pre[(size_t)(w - 1) * n + i], z, inv, L, zi, inv_next);  // 1 / Z_w, and the running inverse stripped of Z_w
    inv = inv_next;
    Aff a = table[(size_t)w * n + i];
    a.x = gf_mul(a.x, zi, L);
    a.y = gf_mul(a.y, gf_sqr(zi), L);
    table[(size_t)w * n + i] = a;
  }
}

}  // namespace dvp
