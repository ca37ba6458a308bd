// MSM merge and tail: the lambda-projective sum-over-subsets tree (k_merge), the tails (k_tail_groups, k_tail), the
// sums of partial points (k_sum_points, k_join_points) and the multiplier microbenchmark kernel (k_ubench_mul).  Part of msm.hip's
// translation unit: msm.hip includes it, and its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include <type_traits>

#include "k233.cuh"
#include "tau.cuh"
#include "codec.cuh"
#include "msm_reduce.cuh"

namespace dvp {

// ---- pruned sum-over-subsets merge (see file header, step 4) ---------------------------------------
// level j: blocks of 2^(j+1) buckets; slot s <= j: A[base+s] += A[base+2^j+s]; slot j+1 <- T_right
// QUAD: the deep levels have far fewer additions than the chip has lanes and are pure latency; there the four lanes
// of a quad share one addition (gf233.cuh, quad-cooperative product), 2.2x shorter per level.
// Round 4: the tree runs in lambda-projective coordinates (k233.cuh: 11M + 2S per full addition against 13M + 5S).  Level 0
// reads every bucket exactly once (as the left or the right operand of its pair) and converts it on the way in -- (X, Y, Z) ->
// (X^2, X^2 + Y, X Z), 1M + 1S -- so the right operand, which stays in place as D_0 of its block, is written back converted;
// k_tail converts what it reads back to Lopez-Dahab (1M) for its doublings.
// GROUP = lanes per addition: 1 (wide levels, Karatsuba multiplier), 4 (a quad, <= MERGE_QUAD_MAX additions) or 16 (a DPP row,
// <= MERGE_HEX_MAX additions: the deepest levels are pure latency and a lone wave pays per instruction, gf233.cuh)
template <int GROUP, bool FIRST>
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(GROUP > 1 ? 1 : 2, 2))) k_merge(Ld* __restrict__ A, int j, uint32_t total /* nblocks*(j+1) */, Ld* __restrict__ save0 /* FIRST: where bucket 0 is kept as it was (or nullptr) */) {
  using LT = typename std::conditional<GROUP == 1, GfLdsK, typename std::conditional<GROUP == 4, GfLdsQ, GfLdsH>::type>::type;
  extern __shared__ char lds_raw[];
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  tid /= (uint32_t)GROUP;
  if (tid >= total) return;
  uint32_t blk = tid / (uint32_t)(j + 1), s = tid - blk * (uint32_t)(j + 1);
  size_t base = (size_t)blk << (j + 1);
  Ld l = A[base + s], r = A[base + ((size_t)1 << j) + s];
  LT L = MergeMul<LT>::init(lds_raw);
  const bool lead = MergeMul<LT>::lead(L);  // the lane of the group that stores
  if (FIRST) {  // j == 0
    // signed windows: bucket 0 (the digits of magnitude 2^(c-1)) is weighed separately by k_tail; the merge turns slot 0 into the total
    if (save0 && tid == 0 && lead) *save0 = l;
    lam_from_ld(l, L);
    lam_from_ld(r, L);
  }
  if (lead && s == 0 && j != 1) A[base + 1 + j] = r;  // j = 0: the converted right operand; j = 1: T_right is in place already
  if (!lam_add_ip(l, r, L)) {  // l == r (equal bucket sums: equal bases and scalars): double a copy read back
    l = A[base + s];
    if (FIRST) lam_from_ld(l, L);
    lam_dbl_ip(l, L);
  }
  if (lead) A[base + s] = l;
}

// Round 6, one-shot MSMs (W windows x c points = 240 at 2^16 points): the Frobenius powers and the first four levels of the add tree
// on MANY workgroups -- a workgroup takes 16 consecutive points, one row of 16 lanes each (the sixteen-lane product, ~290 instructions
// against the quad's ~450), and leaves their sum in part[blockIdx.x]; k_tail then adds the <= 16 group sums (n_narrow == -4) and
// converts.  The single-workgroup tail walked 120 + 60 + 30 + 15 additions in passes of 64 quads: 218 us of its own at 2^16 points.
// The sum is the same group element in another order: the affine result and its encoding are unchanged bit for bit.
__global__ void __launch_bounds__(EC_TPB) k_tail_groups(const Ld* __restrict__ A, int c, int W, int n_narrow, GfSqrTables T, Ld* __restrict__ buf /* 2 W c */,
                                                        Ld* __restrict__ part) {
  extern __shared__ char lds_raw[];
  GfLdsH H = gf_ldsh_init(lds_raw);
  const uint32_t cnt0 = (uint32_t)(W * c), g0 = blockIdx.x * 16u;
  const uint32_t cntl = min(16u, cnt0 - g0);
  Ld* in = buf + g0;
  Ld* out = buf + cnt0 + g0;
  {
    const uint32_t row = threadIdx.x >> 4;
    if (row < cntl) {  // whole rows together
      const uint32_t tid = g0 + row;
      const uint32_t w = tid / (uint32_t)c, t = tid - w * (uint32_t)c;
      const int k = (int)(w * (uint32_t)c) - min((int)w, n_narrow) + (int)t;
      Ld p = A[((size_t)w << c) + 1 + t];
      lam_to_ld(p, H);  // lambda-projective (the merge tree's output) -> Lopez-Dahab: Y = X (L + X)
      // the three coordinates' Frobenius powers side by side: the 16 lanes of the row hold the same point, lanes 0-4 / 5-9 / 10-15 take
      // X / Y / Z through the table passes (a serial chain of L2 round trips each) and the row gathers them again
      const uint32_t sel = H.r < 5u ? 0u : (H.r < 10u ? 1u : 2u);
      Gf v = sel == 0u ? p.X : (sel == 1u ? p.Y : p.Z);
      v = gf_sqr_n_fast(v, k, T);
      const int lane0 = (int)(threadIdx.x & 63u) - (int)H.r;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        p.X.w[q] = (uint32_t)__shfl((int)v.w[q], lane0);
        p.Y.w[q] = (uint32_t)__shfl((int)v.w[q], lane0 + 5);
        p.Z.w[q] = (uint32_t)__shfl((int)v.w[q], lane0 + 10);
      }
      if (H.r == 0) in[row] = p;
    }
  }
  __syncthreads();
  uint32_t cnt = cntl;
  while (cnt > 1) {
    const uint32_t half = (cnt + 1) / 2;
    const uint32_t i = threadIdx.x >> 4;
    if (i < half) {
      Ld a = in[2 * i];
      if (2 * i + 1 < cnt) ld_add_ip(a, in[2 * i + 1], H);
      if (H.r == 0) out[i] = a;
    }
    __syncthreads();
    Ld* t = in; in = out; out = t;
    cnt = half;
  }
  if (threadIdx.x == 0) part[blockIdx.x] = in[0];
}

// The whole Frobenius tail of an MSM in ONE single-workgroup launch: E[w*c+t] = tau^k(A[w*2^c + 1 + t]) with k = the first
// digit of window w plus t (window w starts at digit w*c - min(w, n_narrow): the first n_narrow windows are c-1 digits wide;
// up to 239 squarings per coordinate, done by table passes, not a serial chain), then the pairwise add tree (in[count]
// treated as infinity when count is odd), then the projective -> affine conversion.  Every step is pure latency -- 18..240
// points, log-depth -- so seven launches (each a ~5 us boundary plus a grid ramp) buy nothing over __syncthreads between
// the levels of one 256-thread block (64 quads, one addition per quad and pass).  buf: 2 * cnt Ld of scratch.
// n_narrow == -3: signed aligned windows over the binary digits (the default fixed-base flavour, W = 1): key = |digit|, so the
// result is sum_t 2^t A[1 + t], t < c - 1, plus 2^(c-1) x bucket 0 (doublings instead of Frobenius powers).
// out_enc (optional): the result's 30-byte encoding under `rule` as well (what k_encode_point would make of out_xy): the affine
// conversion and the encoding's 1 / x share ONE inversion, 1 / (X Z) -- a proof's two commitments are encoded right here instead
// of after a host round trip, a launch and a second 45 us inversion chain.
// HEX (round 4, the signed flavour's c points): a DPP row of 16 lanes per point instead of a quad -- the doublings, the add tree and the
// final inversion are one dependent chain of ~140 products, and a lone wave pays per instruction (gf233.cuh: ~290 against ~450 per
// product).  16 rows per workgroup: the points go out longest chain first, the few left over to the rows with the shortest ones.
template <bool HEX>
__global__ void __launch_bounds__(EC_TPB) k_tail(const Ld* __restrict__ A, int c, int W, int n_narrow, GfSqrTables T, Ld* __restrict__ buf,
                                                 uint32_t* __restrict__ out_xy, uint32_t* __restrict__ out_inf, uint8_t* __restrict__ out_enc, int rule,
                                                 unsigned long long* __restrict__ ctrl /* msm_core's control words: [0] err, [1] d_max | rest_n, [2] err_out, [3] last MSM's [1] */, unsigned long long* __restrict__ err_dst) {
  using LT = typename std::conditional<HEX, GfLdsH, GfLdsQ>::type;
  constexpr int GS = HEX ? 4 : 2;             // log2 lanes per point
  constexpr uint32_t NG = EC_TPB >> GS;       // points in flight per pass
  extern __shared__ char lds_raw[];
  LT L = MergeMul<LT>::init(lds_raw);
  const uint32_t grp = threadIdx.x >> GS;
  const uint32_t cnt0 = (uint32_t)(W * c);
  Ld* in = buf;
  Ld* out = buf + cnt0;
  if (n_narrow == -4) {
    // the cnt0 points are in buf already (the group sums of k_tail_groups, Frobenius powers applied): only the tree and the conversion
  } else if (n_narrow == -3) {
    // signed aligned windows: t doublings of A[1 + t], one point per quad of lanes (a serial chain of <= c - 1 doublings at
    // 3 products + 5 squarings each); the last point is bucket 0 (the digits of magnitude 2^(c-1); saved at buf[2 cnt0] before
    // the merge turned slot 0 into the total)
    for (uint32_t q = 0; q * NG < cnt0; ++q) {
      // point t needs t doublings: pass 0 hands the longest chains to groups 0, 1, ..; the next pass runs the other way round
      const uint32_t idx = q * NG + ((q & 1u) ? NG - 1 - grp : grp);
      if (idx >= cnt0) continue;  // whole groups skip together
      const uint32_t pt = cnt0 - 1 - idx;
      Ld p = pt + 1 < cnt0 ? A[1 + pt] : buf[2 * cnt0];
      if (pt + 1 < cnt0) lam_to_ld(p, L);  // the merge tree's lambda-projective output; bucket 0 was saved before the tree (Lopez-Dahab)
#pragma unroll 1
      for (uint32_t k = 0; k < pt; ++k) p = ld_dbl(p, L);
      if (L.r == 0) in[pt] = p;
    }
  } else {
    for (uint32_t tid = threadIdx.x; tid < cnt0; tid += EC_TPB) {
      uint32_t w = tid / (uint32_t)c, t = tid - w * (uint32_t)c;
      int k = (int)(w * (uint32_t)c) - min((int)w, n_narrow) + (int)t;
      Ld p = A[((size_t)w << c) + 1 + t];
      p.Y = gf_mul(p.X, gf_add(p.Y, p.X));  // lambda-projective (the merge tree's output) -> Lopez-Dahab: Y = X (L + X)
      p.X = gf_sqr_n_fast(p.X, k, T);
      p.Y = gf_sqr_n_fast(p.Y, k, T);
      p.Z = gf_sqr_n_fast(p.Z, k, T);
      in[tid] = p;
    }
  }
  __syncthreads();
  uint32_t cnt = cnt0;
  while (cnt > 1 && (HEX || (cnt + 1) / 2 > EC_TPB / 16)) {  // quad variant: while a level has more additions than the block has rows
    const uint32_t half = (cnt + 1) / 2;
    for (uint32_t i = grp; i < half; i += NG) {  // whole groups take the same trips
      Ld a = in[2 * i];
      if (2 * i + 1 < cnt) ld_add_ip(a, in[2 * i + 1], L);
      if (L.r == 0) out[i] = a;
    }
    __syncthreads();
    Ld* t = in; in = out; out = t;
    cnt = half;
  }
  // the last levels (<= 16 additions) and the conversion run on rows of 16 lanes in both variants (same LDS tables)
  GfLdsH H;
  H.l = L.l;
  H.r = threadIdx.x & 15u;
  while (cnt > 1) {
    const uint32_t half = (cnt + 1) / 2;
    for (uint32_t i = threadIdx.x >> 4; i < half; i += EC_TPB / 16) {
      Ld a = in[2 * i];
      if (2 * i + 1 < cnt) ld_add_ip(a, in[2 * i + 1], H);
      if (H.r == 0) out[i] = a;
    }
    __syncthreads();
    Ld* t = in; in = out; out = t;
    cnt = half;
  }
  if (threadIdx.x >= 16) return;  // one row: the inversion's products are a serial chain
  Aff a;
  Ld p = in[0];
  const bool fin = !ld_is_inf(p);
  a.x = gf_zero();
  a.y = gf_zero();
  Gf w = gf_zero();
  if (fin) {
    if (out_enc && !gf_is_zero(p.X)) {
      // x = X / Z, y = Y / Z^2, y / x = Y / (X Z): everything from inv = 1 / (X Z)
      const Gf inv = gf_inv_fast(gf_mul(p.X, p.Z, H), T, H);
      const Gf zi = gf_mul(inv, p.X, H);
      a.x = gf_mul(p.X, zi, H);
      a.y = gf_mul(p.Y, gf_sqr(zi), H);
      const Gf lam1 = gf_add(gf_add(a.x, gf_mul(p.Y, inv, H)), gf_one());
      w = gf_sqr_tab_wide(gf_sqr_tab_wide(lam1, T.t116), T.t116);
      if (rule) w = codec_present(w, rule, T);
    } else {
      Gf zi = gf_inv_fast(p.Z, T, H);
      a.x = gf_mul(p.X, zi, H);
      a.y = gf_mul(p.Y, gf_sqr(zi), H);
      if (out_enc) {  // x = 0 (the point of order two): the same formula as k_encode_point, where 1 / 0 reads 0
        const Gf lam1 = gf_add(gf_add(a.x, gf_mul(a.y, gf_inv_fast(a.x, T, H), H)), gf_one());
        w = gf_sqr_tab_wide(gf_sqr_tab_wide(lam1, T.t116), T.t116);
        if (rule) w = codec_present(w, rule, T);
      }
    }
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out_xy[k] = a.x.w[k];
    out_xy[8 + k] = a.y.w[k];
  }
  *out_inf = fin ? 0u : 1u;
  if (out_enc) store30(out_enc, w, rule);
  // the scalar-range word: to the caller's block (a deferred MSM, msm_core's d_err_defer) and to err_out, which the host copy of a
  // synchronous call reads; then the control words are left as the next MSM on this workspace expects them
  const unsigned long long e = ctrl[0];
  if (err_dst) *err_dst = e;
  ctrl[2] = e;
  ctrl[3] = ctrl[1];  // (d_max | rest_n) of this MSM, kept for dvp_debug_msm_rest_len
  ctrl[0] = ~0ull;
  ctrl[1] = 0ull;
}

// sum of n affine points (the partial MSM results of n GPUs or ranks) -> affine: one quad of lanes, n - 1 mixed
// additions + one inversion, all through the quad-cooperative multiplier (~15 us per point + ~50 us)
__global__ void __launch_bounds__(64) k_sum_points(const char* __restrict__ pts, uint32_t pt_stride_bytes, const uint32_t* __restrict__ inf, uint32_t n,
                                                  uint32_t inf_stride, GfSqrTables T, uint32_t* __restrict__ out_xy, uint32_t* __restrict__ out_inf) {
  extern __shared__ char lds_raw[];
  GfLdsQ L = gf_ldsq_init(lds_raw);
  if (threadIdx.x >= 4 || blockIdx.x != 0) return;
  Ld acc = ld_infinity();
#pragma unroll 1
  for (uint32_t i = 0; i < n; ++i) {
    if (inf[(size_t)i * inf_stride]) continue;
    Aff q = *(const Aff*)(pts + (size_t)i * pt_stride_bytes);
    ld_madd_ip(acc, q, L);
  }
  Aff a;
  a.x = gf_zero();
  a.y = gf_zero();
  const bool fin = !ld_is_inf(acc);
  if (fin) {
    Gf zi = gf_inv_fast(acc.Z, T, L);
    a.x = gf_mul(acc.X, zi, L);
    a.y = gf_mul(acc.Y, gf_sqr(zi), L);
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out_xy[k] = a.x.w[k];
    out_xy[8 + k] = a.y.w[k];
  }
  *out_inf = fin ? 0u : 1u;
}

// The join of a MIXED MSM (a prover whose table budget covers only a prefix of the bases: prove.hip): the fixed-base MSM over the
// prefix and the one-shot MSM over the suffix each left an affine partial point and a scalar-range word; this launch writes what the
// tail kernel of a single MSM would have written for the whole sum -- the affine sum (complete addition: either part neutral, P = Q,
// P = -Q), its 30-byte encoding under `rule` from the same shared inversion 1 / (X Z) as k_tail, and the merged range word: the
// prefix's word wins (its indices come first), the suffix's first bad index is rebased by `covered` to the whole vector.  One row of
// 16 lanes (the mixed addition and the inversion are one dependent chain of ~300 products); LDS: one wave's tables.
__global__ void __launch_bounds__(64) k_join_points(const Aff* __restrict__ pa, const uint32_t* __restrict__ inf_a, const unsigned long long* __restrict__ err_a,
                                                    const Aff* __restrict__ pb, const uint32_t* __restrict__ inf_b, const unsigned long long* __restrict__ err_b,
                                                    uint32_t covered, GfSqrTables T, uint32_t* __restrict__ out_xy, uint32_t* __restrict__ out_inf,
                                                    uint8_t* __restrict__ out_enc, int rule, unsigned long long* __restrict__ err_dst) {
  extern __shared__ char lds_raw[];
  GfLdsH H = gf_ldsh_init(lds_raw);
  if (threadIdx.x >= 16 || blockIdx.x != 0) return;
  Ld p = ld_infinity();
  if (!*inf_a) {
    const Aff q = *pa;
    p.X = q.x; p.Y = q.y; p.Z = gf_one();
  }
  if (!*inf_b) {
    const Aff q = *pb;
    ld_madd_ip(p, q, H);
  }
  Aff a;
  const bool fin = !ld_is_inf(p);
  a.x = gf_zero();
  a.y = gf_zero();
  Gf w = gf_zero();
  if (fin) {
    if (out_enc && !gf_is_zero(p.X)) {
      // x = X / Z, y = Y / Z^2, y / x = Y / (X Z): everything from inv = 1 / (X Z), as in k_tail
      const Gf inv = gf_inv_fast(gf_mul(p.X, p.Z, H), T, H);
      const Gf zi = gf_mul(inv, p.X, H);
      a.x = gf_mul(p.X, zi, H);
      a.y = gf_mul(p.Y, gf_sqr(zi), H);
      const Gf lam1 = gf_add(gf_add(a.x, gf_mul(p.Y, inv, H)), gf_one());
      w = gf_sqr_tab_wide(gf_sqr_tab_wide(lam1, T.t116), T.t116);
      if (rule) w = codec_present(w, rule, T);
    } else {
      Gf zi = gf_inv_fast(p.Z, T, H);
      a.x = gf_mul(p.X, zi, H);
      a.y = gf_mul(p.Y, gf_sqr(zi), H);
      if (out_enc) {  // x = 0 (the point of order two): the same formula as k_encode_point, where 1 / 0 reads 0
        const Gf lam1 = gf_add(gf_add(a.x, gf_mul(a.y, gf_inv_fast(a.x, T, H), H)), gf_one());
        w = gf_sqr_tab_wide(gf_sqr_tab_wide(lam1, T.t116), T.t116);
        if (rule) w = codec_present(w, rule, T);
      }
    }
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out_xy[k] = a.x.w[k];
    out_xy[8 + k] = a.y.w[k];
  }
  *out_inf = fin ? 0u : 1u;
  if (out_enc) store30(out_enc, w, rule);
  const unsigned long long ea = *err_a, eb = *err_b;
  *err_dst = ea != ~0ull ? ea : (eb != ~0ull ? eb + (unsigned long long)covered : ~0ull);
}

// multiplier microbenchmark (bench.py's roofline leg runs it OUTSIDE the timed loop): a dependent chain of products per
// lane through the Karatsuba LDS multiplier at the occupancy of k_affine_round (256-thread blocks, 3 waves per SIMD)
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(3, 3))) k_ubench_mul(Gf* __restrict__ out, int reps) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const uint32_t t = threadIdx.x + blockIdx.x * blockDim.x;
  Gf x, y;
#pragma unroll
  for (int i = 0; i < 8; ++i) { x.w[i] = t * 2654435761u + i; y.w[i] = t * 40503u + 7 * i; }
  x.w[7] &= 0x1ff; y.w[7] &= 0x1ff;
#pragma unroll 1
  for (int r = 0; r < reps; ++r) { x = gf_mul(x, y, L); y.w[0] ^= x.w[3]; }
  out[t] = x;
}

}  // namespace dvp
