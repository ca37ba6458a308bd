// The 30-byte presentation of an encoded point (shared by codec.hip's kernels and the MSM tail, which encodes its own result).
#pragma once
#include "k233.cuh"
#include "tau.cuh"

namespace dvp {

// ---- the encoding RULE as a run-time constant (dvp_codec_set_rule) -------------------------------------------------------
// What is settled (tools/pin_xsk233.py): a point travels as ONE field element of 30 bytes from which the
// decode equation x^2 + (w^2 + w + a) x + b = 0 recovers it, and w = y'/x on the N = (0,0) model satisfies it.  What one vector
// from xs233 would settle is which equivalent presentation of that element the bytes hold.  Every candidate tools/pin_xsk233.py
// enumerates (8 formulas x 2 views x 2 generator signs x "+1" x 2 byte orders) collapses -- on the curve sqrt(s/x) = y'/x =
// sqrt(lambda), s/x = lambda = (y'/x)^2, and w(Q + N) = w(-Q) = w(Q) + 1 -- into the classes below (the formulas y/x and
// "x alone" are not encodings of this family: their decode is a cubic / needs a sign bit).  rule =
//   bit 0      the element is w + 1  (= the E[r] representative's own value, = the negated generator's convention)
//   bit 1      bytes are big-endian
//   bits 2..3  0: w = sqrt(s/x) itself   1: w^2 (= s/x = lambda)   2: sqrt(w) (= sqrt(y'/x))
// Rule 0 is the candidate followed since round 1 (Pornin, ePrint 2022/1325, as recalled).  The neutral element is 30 zero bytes
// under every rule.  A vector from a machine with cargo turns into `dvp_codec_set_rule(k)` (or DVP_CODEC_RULE=k), not a port.
constexpr int CODEC_RULES = 12;
__device__ __forceinline__ Gf codec_present(Gf w, int rule, const GfSqrTables& T) {
  const int tr = (rule >> 2) & 3;
  if (tr == 1) w = gf_sqr(w);
  else if (tr == 2) w = gf_sqr_tab(gf_sqr_tab(w, T.t116), T.t116);  // sqrt = 232 squarings = two 116-step table passes
  if (rule & 1) w.w[0] ^= 1u;
  return w;
}
__device__ __forceinline__ Gf codec_absorb(Gf t, int rule, const GfSqrTables& T) {
  if (rule & 1) t.w[0] ^= 1u;
  const int tr = (rule >> 2) & 3;
  if (tr == 1) t = gf_sqr_tab(gf_sqr_tab(t, T.t116), T.t116);
  else if (tr == 2) t = gf_sqr(t);
  return t;
}
__device__ __forceinline__ void store30(uint8_t* dst, const Gf& w, int rule) {
  const bool be = (rule & 2) != 0;
#pragma unroll
  for (int b = 0; b < 30; ++b) dst[be ? 29 - b : b] = (uint8_t)(w.w[b >> 2] >> (8 * (b & 3)));
}
__device__ __forceinline__ Gf load30(const uint8_t* src, uint32_t* top_bits, int rule) {
  const bool be = (rule & 2) != 0;
  Gf w = gf_zero();
#pragma unroll
  for (int b = 0; b < 30; ++b) w.w[b >> 2] |= (uint32_t)src[be ? 29 - b : b] << (8 * (b & 3));
  *top_bits = w.w[7] >> 9;
  return w;
}

// P in E[r] (affine, x != 0)?  E[r] = 4E: Tr(x) = 0 and a half of P has Tr(x_half) = 0.
// half-trace through the byte table (30 lookups instead of 232 squarings)
__device__ __forceinline__ bool k233_in_subgroup(const Aff& p, const GfSqrTables& T, const GfLdsK& L) {
  if (gf_is_zero(p.x)) return false;
  if (gf_trace(p.x)) return false;
  Gf lam = gf_sqr_tab(p.x, T.th);                   // lam^2 + lam = x
  Gf u2 = gf_add(p.y, gf_mul(gf_add(lam, gf_one()), p.x, L));  // x_half^2
  return gf_trace(u2) == 0;
}

// One 30-byte encoding -> the E[r] representative (codec.hip's k_decode and verify.hip's k_verify).  Returns false for an
// invalid encoding (spare top bits set, no curve point, or no root in E[r]); then r = 0 and is_inf is left false.  A valid
// encoding decodes to the unique point whose encoding (k_encode) is these 30 bytes again.
__device__ __forceinline__ bool codec_decode(const uint8_t* enc, int rule, const GfSqrTables& T, const GfLdsK& L, Aff& r, bool& is_inf) {
  uint32_t top;
  Gf w = load30(enc, &top, rule);
  r.x = gf_zero();
  r.y = gf_zero();
  bool ok = (top == 0);
  is_inf = false;
  if (ok && gf_is_zero(w)) {
    is_inf = true;
  } else if (ok) {
    if (rule) w = codec_absorb(w, rule, T);
    Gf w2 = gf_sqr(w);
    Gf e = gf_add(w2, w);
    ok = !gf_is_zero(e);
    if (ok) {
      Gf einv = gf_inv_fast(e, T, L);
      Gf cst = gf_sqr(einv);  // 1/e^2
      ok = gf_trace(cst) == 0;
      if (ok) {
        Gf z = gf_sqr_tab(cst, T.th);   // half-trace: z^2 + z = 1/e^2
        Gf lam = gf_add(w2, gf_one());  // x + y/x
        Aff c0, c1;
        c0.x = gf_mul(e, z, L);
        c1.x = gf_add(c0.x, e);
        c0.y = gf_mul(c0.x, gf_add(lam, c0.x), L);
        c1.y = gf_mul(c1.x, gf_add(lam, c1.x), L);
        bool s0 = k233_in_subgroup(c0, T, L), s1 = k233_in_subgroup(c1, T, L);
        if (s0) r = c0; else if (s1) r = c1; else ok = false;
      }
    }
  }
  return ok;
}

// ---- fixed-base tables of the generator (codec.hip: gen_table): tab[w][d] = sum_t d_t tau^(c w + t)(G), affine ----------
constexpr int GEN_C = 16;  // 15 windows, 63 MB table (L2 / Infinity-Cache resident): 15 mixed additions per scalar
constexpr int GEN_W = TAU_DIGITS / GEN_C;  // 15

}  // namespace dvp
