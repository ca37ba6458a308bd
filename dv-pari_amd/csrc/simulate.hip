// The verifier's side as test vectors: accepted proofs made from the trapdoor alone (dvp_simulate_batch*), and the stage values of
// SRS::verify per proof (dvp_verify_trace_batch*).  One lane per proof, one launch per call once the generator table exists.
//
// k_simulate solves the verifier's equation v0 K + u0 G = P (src/srs.rs:418-424) for chosen discrete logs:
//   P = p G,  alpha = H(enc(P), pub),  v0 = (tau - alpha) eps,  pick b0 and a target t for u0:
//   K = ((p - t) / v0) G,   a0 = (t / eps - delta b0 + delta^2 i0) / (1 + delta^2 b0)   =>   v0 K + u0 G = (p - t) G + t G = P.
// p, b0 and t are drawn from BLAKE3(key || LE64(index_base + j) || tag); the DVP_SIM_* cases steer t (and p) into the exceptional
// branches of the verifier's addition chain.  Per lane: two generator-table multiplications (k_mulgen's loop with k_verify's complete
// addition), each encoded straight from Lopez-Dahab coordinates with ONE GF inversion -- lambda + 1 = (X^2 + Y + X Z) / (X Z), so the
// affine point is never formed --, the transcript, a Horner pass and one Fr inversion shared by 1 / v0 and 1 / (1 + delta^2 b0).
//
// k_verify_trace is SRS::verify with every stage written out: a third text beside k_verify and k_verify_rlc_prep (verify.hip), not a
// flag on k_verify, whose register allocation any sharing changes.  v0 K and u0 G go into two accumulators, are normalised with one
// shared GF inversion, added by the complete mixed addition, and the sum is normalised: the record holds all three points affine.
#include <cstring>

#include "blake3_dev.cuh"
#include "codec.cuh"
#include "common.h"
#include "fr.cuh"
#include "host_api.h"
#include "k233.cuh"
#include "tau.cuh"
#include "verify_front.cuh"

namespace dvp {

// draw(j, tag): the first 29 bytes of BLAKE3(key || LE64(index) || tag), little-endian, masked to 230 bits (< p = 2^231 + c)
__device__ __forceinline__ Fr sim_draw(const b3d::Words8& key, uint64_t index, uint32_t tag) {
  uint32_t m[16], out[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = key.w[k];
  m[8] = (uint32_t)index;
  m[9] = (uint32_t)(index >> 32);
  m[10] = tag;  // one byte
#pragma unroll
  for (int k = 11; k < 16; ++k) m[k] = 0;
  b3d::hash_chunk(m, 41, out);
  Fr r;
#pragma unroll
  for (int k = 0; k < 7; ++k) r.v[k] = out[k];
  r.v[7] = out[7] & 0x3fu;
  return r;
}

// a / 2 mod p for a canonical a: (a + p) / 2 when a is odd (a + p < 2^233)
__device__ __forceinline__ Fr sim_half(const Fr& a) {
  const bool odd = a.v[0] & 1u;
  uint32_t s[9];
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c += (uint64_t)a.v[k] + (odd ? fr_p_limb(k) : 0u);
    s[k] = (uint32_t)c;
    c >>= 32;
  }
  s[8] = (uint32_t)c;
  Fr r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = (s[k] >> 1) | (s[k + 1] << 31);
  return r;
}

__device__ __forceinline__ void store29(uint8_t* dst, const Fr& a) {
#pragma unroll
  for (int b = 0; b < 29; ++b) dst[b] = (uint8_t)(a.v[b >> 2] >> (8 * (b & 3)));
}

// enc(k G) -> dst[0..30): the table loop of k_mulgen, then k_encode's element from the projective point (one inversion, of X Z: a
// point of E[r] has x != 0); k = 0 gives the neutral element, 30 zero bytes
__device__ __forceinline__ void sim_mulgen_store(const Fr& k, const Aff* __restrict__ tab, const GfSqrTables& T, const GfLdsK& L, int rule,
                                                 uint8_t* dst) {
  uint32_t r0t[5], r1t[5];
  tau_partial_reduce(k.v, r0t, r1t);
  Ld acc = ld_infinity();
#pragma unroll 1
  for (int w = 0; w < GEN_W; ++w) {
    const uint32_t d = tau_step16(r0t, r1t);
    if (d) madd_complete(acc, tab[((size_t)w << GEN_C) + d], L);
  }
  Gf w = gf_zero();
  if (!ld_is_inf(acc)) {
    const Gf xz = gf_mul(acc.X, acc.Z, L);
    const Gf num = gf_add(gf_add(gf_sqr(acc.X), acc.Y), xz);
    const Gf lam1 = gf_mul(num, gf_inv_fast(xz, T, L), L);
    w = gf_sqr_tab(gf_sqr_tab(lam1, T.t116), T.t116);  // sqrt = 232 squarings = two 116-step table passes
    if (rule) w = codec_present(w, rule, T);
  }
  store30(dst, w, rule);
}

// status != 0: the proof is 118 zero bytes and both discrete logs are zero
__device__ __forceinline__ void sim_reject(uint8_t* pr, uint8_t* status, Fr* dlogs, size_t i, uint32_t st) {
#pragma unroll 1
  for (int b = 0; b < 118; ++b) pr[b] = 0;
  status[i] = (uint8_t)st;
  if (dlogs) {
    dlogs[2 * i] = fr_zero();
    dlogs[2 * i + 1] = fr_zero();
  }
}

// `proofs` is read back by the lane that wrote it (the transcript hashes the 30 bytes of enc(P) as stored): no __restrict__ on it
__global__ void __launch_bounds__(256, 2)
k_simulate(const Fr* __restrict__ pub, uint32_t npub, size_t n, VerifyConsts K, Fr eps_inv_m, b3d::Words8 key, uint64_t index_base,
           const uint8_t* __restrict__ cases, const Fr* __restrict__ b0_in, const Aff* __restrict__ tab, GfSqrTables T, int rule,
           uint8_t* proofs, uint8_t* __restrict__ status, Fr* __restrict__ dlogs) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t* pr = proofs + 118 * i;
  const Fr* pi = pub + (size_t)npub * i;
  const uint64_t index = index_base + (uint64_t)i;
  uint32_t bad = 0;
  const uint32_t cs = cases ? cases[i] : (uint32_t)DVP_SIM_GENERIC;
  if (cs > DVP_SIM_K_ZERO) bad |= DVP_SIM_BAD_CASE;
#pragma unroll 1
  for (uint32_t j = 0; j < npub; ++j)
    if (!fr_below_p(pi[j])) bad |= DVP_SIM_BAD_PUBLIC;
  Fr b0;
  if (b0_in) {
    b0 = b0_in[i];
    if (!fr_below_p(b0)) bad |= DVP_SIM_BAD_B0;
  } else {
    b0 = sim_draw(key, index, 2);
  }
  if (bad) {
    sim_reject(pr, status, dlogs, i, bad);
    return;
  }
  Fr p = sim_draw(key, index, 1);
  if (fr_is_zero(p)) p = fr_one_canon();
  Fr t = sim_draw(key, index, 3);
  if (cs == DVP_SIM_P_ZERO) p = fr_zero();
  if (cs == DVP_SIM_T_HALF) t = sim_half(p);
  if (cs == DVP_SIM_U0_ZERO) t = fr_zero();
  if (cs == DVP_SIM_K_ZERO) t = p;
  sim_mulgen_store(p, tab, T, L, rule, pr);  // stored now: the transcript reads the bytes, and no point is held across it
  uint32_t h_pi[8];
  const Fr alpha = verify_challenge(pr, pi, npub, K, h_pi);
  const Fr v0 = fr_mul(fr_sub(K.tau, alpha), K.eps_m);
  if (fr_is_zero(v0)) {
    sim_reject(pr, status, dlogs, i, DVP_SIM_V0_ZERO);
    return;
  }
  if (cs == DVP_SIM_K_PLUS_G) t = fr_sub(p, v0);
  if (cs == DVP_SIM_K_MINUS_G) t = fr_add(p, v0);
  const Fr i0 = verify_horner(pi, npub, alpha);
  // canonical throughout: mont_mul(x, c R) = x c
  Fr den = fr_add(fr_one_canon(), fr_mul(b0, K.delta2_m));
  if (fr_is_zero(den)) {  // b0 = -1 / delta^2: the next b0, whose denominator is delta^2
    b0 = fr_add(b0, fr_one_canon());
    den = fr_add(fr_one_canon(), fr_mul(b0, K.delta2_m));
  }
  // one inversion for 1 / v0 and 1 / den: fr_inv takes z as (z / R) R and returns R^2 / z, so the two products below are R / v0, R / den
  const Fr zi = fr_inv(fr_mul(v0, fr_to_mont(den)));
  const Fr v0_inv_m = fr_mul(zi, den), den_inv_m = fr_mul(zi, v0);
  const Fr k = fr_mul(fr_sub(p, t), v0_inv_m);
  const Fr num = fr_add(fr_sub(fr_mul(t, eps_inv_m), fr_mul(b0, K.delta_m)), fr_mul(i0, K.delta2_m));
  const Fr a0 = fr_mul(num, den_inv_m);
  sim_mulgen_store(k, tab, T, L, rule, pr + 30);
  store29(pr + 60, a0);
  store29(pr + 89, b0);
  status[i] = DVP_SIM_OK;
  if (dlogs) {
    dlogs[2 * i] = p;
    dlogs[2 * i + 1] = k;
  }
}

// ---- the verdict trace -----------------------------------------------------------------------------------------------------------
constexpr uint32_t TRACE_WORDS = sizeof(dvp_verify_trace) / 4;  // 122
static_assert(sizeof(dvp_verify_trace) == 488 && offsetof(dvp_verify_trace, p_xy) == 160 && offsetof(dvp_verify_trace, vk_xy) == 288 &&
                  offsetof(dvp_verify_trace, p_inf) == 480 && offsetof(dvp_verify_trace, verdict) == 485,
              "k_verify_trace writes the record by word offsets");

__device__ __forceinline__ void trace_put(uint32_t* o, uint32_t word, const Fr& a) {
#pragma unroll
  for (int k = 0; k < 8; ++k) o[word + k] = a.v[k];
}
__device__ __forceinline__ void trace_put(uint32_t* o, uint32_t word, const Aff& a) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    o[word + k] = a.x.w[k];
    o[word + 8 + k] = a.y.w[k];
  }
}

// one wave per SIMD, as k_verify: the tau-adic loop holds the running point and an accumulator beside the LDS multiplier's operands
__global__ void __launch_bounds__(256, 1)
k_verify_trace(const uint8_t* __restrict__ proofs, size_t n, const Fr* __restrict__ pub, uint32_t npub, VerifyConsts K, const Aff* __restrict__ tab,
               GfSqrTables T, int rule, uint32_t* __restrict__ out) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* pr = proofs + 118 * i;
  const Fr* pi = pub + (size_t)npub * i;
  uint32_t* o = out + (size_t)TRACE_WORDS * i;
  Aff P, Kp;
  bool p_inf, k_inf;
  const uint32_t bad = verify_decode(pr, pi, npub, T, L, rule, P, p_inf, Kp, k_inf);
  if (bad) {  // a validity bit: every other field is zero
#pragma unroll 1
    for (uint32_t w = 0; w < TRACE_WORDS - 1; ++w) o[w] = 0;
    o[TRACE_WORDS - 1] = bad << 8;
    return;
  }
  VerifyFront f;
  {
    VerifyStages s;
    verify_scalars(pr, pi, npub, K, f, &s);
    trace_put(o, 0, s.alpha);
    trace_put(o, 8, s.i0);
    trace_put(o, 16, s.r0);
  }
  trace_put(o, 24, f.u0);
  trace_put(o, 32, f.v0);
  trace_put(o, 40, P);  // an encoding of the neutral element decodes to zero coordinates
  trace_put(o, 56, Kp);
  uint32_t r0t[5], r1t[5];
  // v0 K: sum_i d_i tau^i(K), digits low to high, tau^i(K) affine (k_verify's loop, into its own accumulator)
  Ld vk = ld_infinity();
  if (!k_inf) {
    tau_partial_reduce(f.v0.v, r0t, r1t);
    Aff q = Kp;
#pragma unroll 1
    for (int s = 0; s < TAU_DIGITS / 16; ++s) {
      const uint32_t dw = tau_step16(r0t, r1t);
#pragma unroll 1
      for (int t = 0; t < 16; ++t) {
        if ((dw >> t) & 1u) madd_complete(vk, q, L);
        q.x = gf_sqr(q.x);
        q.y = gf_sqr(q.y);
      }
    }
  }
  // u0 G through the generator table (k_mulgen's loop), into a second accumulator
  Ld ug = ld_infinity();
  tau_partial_reduce(f.u0.v, r0t, r1t);
#pragma unroll 1
  for (int w = 0; w < GEN_W; ++w) {
    const uint32_t d = tau_step16(r0t, r1t);
    if (d) madd_complete(ug, tab[((size_t)w << GEN_C) + d], L);
  }
  // both affine with one inversion, of Z_vk Z_ug (a point at infinity takes part with Z = 1 and keeps zero coordinates)
  const bool vk_inf = ld_is_inf(vk), ug_inf = ld_is_inf(ug);
  Aff a_vk, a_ug;
  {
    const Gf z1 = gf_select(vk_inf, gf_one(), vk.Z), z2 = gf_select(ug_inf, gf_one(), ug.Z);
    const Gf zi = gf_inv_fast(gf_mul(z1, z2, L), T, L);
    const Gf z1i = gf_mul(zi, z2, L), z2i = gf_mul(zi, z1, L);
    a_vk.x = gf_select(vk_inf, gf_zero(), gf_mul(vk.X, z1i, L));
    a_vk.y = gf_select(vk_inf, gf_zero(), gf_mul(vk.Y, gf_sqr(z1i), L));
    a_ug.x = gf_select(ug_inf, gf_zero(), gf_mul(ug.X, z2i, L));
    a_ug.y = gf_select(ug_inf, gf_zero(), gf_mul(ug.Y, gf_sqr(z2i), L));
  }
  trace_put(o, 72, a_vk);
  trace_put(o, 88, a_ug);
  // the sum by the complete mixed addition (v0 K = +-u0 G and a neutral element on either side), then affine
  Ld sum;
  sum.X = gf_select(vk_inf, gf_one(), a_vk.x);
  sum.Y = a_vk.y;
  sum.Z = gf_select(vk_inf, gf_zero(), gf_one());
  if (!ug_inf) madd_complete(sum, a_ug, L);
  const bool sum_inf = ld_is_inf(sum);
  Aff a_sum;
  a_sum.x = gf_zero();
  a_sum.y = gf_zero();
  if (!sum_inf) {
    const Gf zi = gf_inv_fast(sum.Z, T, L);
    a_sum.x = gf_mul(sum.X, zi, L);
    a_sum.y = gf_mul(sum.Y, gf_sqr(zi), L);
  }
  trace_put(o, 104, a_sum);
  const bool eq = sum_inf == p_inf && gf_eq(a_sum.x, P.x) && gf_eq(a_sum.y, P.y);
  o[120] = (p_inf ? 1u : 0u) | (k_inf ? 1u << 8 : 0u) | (vk_inf ? 1u << 16 : 0u) | (ug_inf ? 1u << 24 : 0u);
  o[121] = (sum_inf ? 1u : 0u) | ((eq ? 0u : (uint32_t)DVP_VERIFY_EQUATION) << 8);
}

// the simulator's constants: the verifier's (trapdoor, binding), 1 / epsilon and the key
struct SimConsts {
  VerifyConsts c;
  Fr eps_inv_m;
  b3d::Words8 key;
};

static int sim_consts(const uint64_t tau[4], const uint64_t delta[4], const uint64_t eps[4], const uint8_t* seed, SimConsts* s) {
  DVP_TRY(verify_consts(tau, delta, eps, &s->c));
  if (fr_is_zero(s->c.eps_m)) return DVP_EINVAL;  // u0 = v0 = 0 whatever the proof holds: nothing to solve
  s->eps_inv_m = fr_inv(s->c.eps_m);
  uint8_t key[32];
  trapdoor_key("dv-pari simulate v1", tau, delta, eps, seed, key);
  memcpy(s->key.w, key, 32);
  return DVP_OK;
}

static int sim_enqueue(const SimConsts& s, const void* d_pub, uint32_t npub, size_t n, uint64_t index_base, const void* d_cases, const void* d_b0,
                       void* d_proofs, void* d_status, void* d_dlogs, hipStream_t st) {
  const Aff* tab;
  DVP_TRY(gen_table(&tab, st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_simulate, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const Fr*)d_pub, npub, n, s.c, s.eps_inv_m, s.key,
             index_base, (const uint8_t*)d_cases, (const Fr*)d_b0, tab, T, codec_rule_now(), (uint8_t*)d_proofs, (uint8_t*)d_status, (Fr*)d_dlogs);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

static int trace_enqueue(const VerifyConsts& c, const void* d_pub, uint32_t npub, const void* d_proofs, size_t n, void* d_out, hipStream_t st) {
  const Aff* tab;
  DVP_TRY(gen_table(&tab, st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_verify_trace, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const uint8_t*)d_proofs, n, (const Fr*)d_pub, npub,
             c, tab, T, codec_rule_now(), (uint32_t*)d_out);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

}  // namespace dvp

using namespace dvp;

// Both flavours check in the order of the verify entries: the trapdoor (epsilon = 0 included), n_public, n == 0 (DVP_OK, nothing
// touched), then the pointers, then (the host flavour) the public inputs, the case bytes and the b0 values.
extern "C" int dvp_simulate_batch_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                                      uint32_t n_public, size_t n, const uint8_t seed[32], uint64_t index_base, const void* d_cases,
                                      const void* d_b0, void* d_proofs, void* d_status, void* d_dlogs, void* stream) {
  SimConsts s;
  DVP_TRY(sim_consts(tau, delta, epsilon, seed, &s));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!d_proofs || !d_status || (n_public && !d_public_inputs)) return DVP_EINVAL;
  return sim_enqueue(s, d_public_inputs, n_public, n, index_base, d_cases, d_b0, d_proofs, d_status, d_dlogs, (hipStream_t)stream);
}

extern "C" int dvp_simulate_batch(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                                  uint32_t n_public, size_t n, const uint8_t seed[32], uint64_t index_base, const uint8_t* cases,
                                  const uint64_t* b0, uint8_t* proofs, uint8_t* status, uint64_t* dlogs) {
  SimConsts s;
  DVP_TRY(sim_consts(tau, delta, epsilon, seed, &s));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!proofs || !status || (n_public && !public_inputs)) return DVP_EINVAL;
  const size_t npub_all = (size_t)n_public * n;
  DVP_TRY(scalars_in_range(public_inputs, npub_all));  // the flat index of the first bad one
  if (cases)
    for (size_t j = 0; j < n; ++j)
      if (cases[j] > DVP_SIM_K_ZERO) {
        g_last_error_index = (int64_t)j;
        return DVP_EINVAL;
      }
  if (b0) DVP_TRY(scalars_in_range(b0, n));
  DevBuf dpub, dc, db, dp, ds, dl;
  DVP_TRY(dpub.up(public_inputs, npub_all * 32));
  DVP_TRY(dc.up_opt(cases, n));
  DVP_TRY(db.up_opt(b0, n * 32));
  DVP_TRY(dp.alloc(n * 118));
  DVP_TRY(ds.alloc(n));
  if (dlogs) DVP_TRY(dl.alloc(n * 64));
  DVP_TRY(sim_enqueue(s, dpub.p, n_public, n, index_base, dc.p, db.p, dp.p, ds.p, dl.p, 0));
  DVP_TRY(dp.down(proofs, n * 118));
  DVP_TRY(ds.down(status, n));
  return dlogs ? dl.down(dlogs, n * 64) : DVP_OK;
}

extern "C" int dvp_verify_trace_batch_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                                          uint32_t n_public, const void* d_proofs, size_t n, void* d_out, void* stream) {
  VerifyConsts c;
  DVP_TRY(verify_consts(tau, delta, epsilon, &c));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!d_proofs || !d_out || (n_public && !d_public_inputs)) return DVP_EINVAL;
  return trace_enqueue(c, d_public_inputs, n_public, d_proofs, n, d_out, (hipStream_t)stream);
}

extern "C" int dvp_verify_trace_batch(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                                      uint32_t n_public, const uint8_t* proofs, size_t n, dvp_verify_trace* out) {
  VerifyConsts c;
  DVP_TRY(verify_consts(tau, delta, epsilon, &c));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!proofs || !out || (n_public && !public_inputs)) return DVP_EINVAL;
  const size_t npub_all = (size_t)n_public * n;
  DVP_TRY(scalars_in_range(public_inputs, npub_all));  // the flat index of the first bad one
  DevBuf dp, dpub, dt;
  DVP_TRY(dp.up(proofs, n * 118));
  DVP_TRY(dpub.up(public_inputs, npub_all * 32));
  DVP_TRY(dt.alloc(n * sizeof(dvp_verify_trace)));
  DVP_TRY(trace_enqueue(c, dpub.p, n_public, dp.p, n, dt.p, 0));
  return dt.down(out, n * sizeof(dvp_verify_trace));
}
