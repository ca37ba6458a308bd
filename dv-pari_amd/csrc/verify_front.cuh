// The front half of SRS::verify for one proof, shared by verify.hip (k_verify_rlc_prep) and simulate.hip (k_simulate, k_verify_trace):
// the trapdoor constants, the FrBits range check, the public-input digest, the decode with its validity bits, the transcript
// challenge and the scalars u0, v0.  k_verify keeps its own text of all this (verify.hip says why).
#pragma once
#include "blake3.h"
#include "blake3_dev.cuh"
#include "codec.cuh"
#include "common.h"
#include "fr.cuh"
#include "k233.cuh"

namespace dvp {

constexpr uint32_t VERIFY_B3_LEVELS = 8;
constexpr uint32_t VERIFY_MAX_PUBLIC = DVP_VERIFY_MAX_PUBLIC;
static_assert((size_t)VERIFY_MAX_PUBLIC * 29 <= ((size_t)1024 << VERIFY_B3_LEVELS), "public inputs beyond the subtree levels");

struct VerifyConsts {
  Fr tau;       // canonical
  Fr delta_m;   // delta * R
  Fr delta2_m;  // delta^2 * R
  Fr eps_m;     // epsilon * R
  b3d::Words8 h_ct;  // H(srs_hash || circuit_hash): the compile-time half of the transcript (src/srs.rs:386-404), dvp_verify_set_binding
};
// verify.hip: the caller's trapdoor (DVP_EINVAL for a value >= p) and the binding in force, read once per call
int verify_consts(const uint64_t tau[4], const uint64_t delta[4], const uint64_t eps[4], VerifyConsts* c);

// the key of an entry that draws from BLAKE3 (the combined check's coefficients, the simulator's scalars): the caller's seed, or
// BLAKE3(tag || tau || delta || epsilon), each as 32 little-endian bytes -- deterministic, and secret as long as the trapdoor is
inline void trapdoor_key(const char* tag, const uint64_t tau[4], const uint64_t delta[4], const uint64_t eps[4], const uint8_t* seed,
                         uint8_t key[32]) {
  if (seed) {
    memcpy(key, seed, 32);
    return;
  }
  const size_t T = strlen(tag);
  std::vector<uint8_t> buf(T + 96);
  memcpy(buf.data(), tag, T);
  const uint64_t* v[3] = {tau, delta, eps};
  for (int s = 0; s < 3; ++s)
    for (int b = 0; b < 32; ++b) buf[T + 32 * s + b] = (uint8_t)(v[s][b >> 3] >> (8 * (b & 7)));
  b3::hash(buf.data(), buf.size(), key);
}

// a < p for 8 little-endian 32-bit limbs (FrBits::to_fr's validity flag when the top limb holds byte 28 only)
__device__ __forceinline__ bool fr_below_p(const Fr& a) {
  uint64_t borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint64_t t = (uint64_t)a.v[k] - fr_p_limb(k) - borrow;
    borrow = (t >> 63) & 1;
  }
  return borrow != 0;
}

// 29 little-endian bytes (FrBits) -> 8 limbs
__device__ __forceinline__ Fr load29(const uint8_t* src) {
  Fr a;
#pragma unroll
  for (int k = 0; k < 8; ++k) a.v[k] = 0;
#pragma unroll
  for (int b = 0; b < 29; ++b) a.v[b >> 2] |= (uint32_t)src[b] << (8 * (b & 3));
  return a;
}

// 16 message words of block `blk_off` (byte offset) of the public-input buffer: each Fr as its 29-byte LE (src/proving.rs:147-150)
__device__ __forceinline__ void pub_block(const uint8_t* pub, uint32_t len, uint32_t blk_off, uint32_t m[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t off = blk_off + 4 * k + b;
      if (off < len) {
        const uint32_t j = off / 29u, r = off - 29u * j;
        w |= (uint32_t)pub[32 * (size_t)j + r] << (8 * b);
      }
    }
    m[k] = w;
  }
}

// BLAKE3 of the n_pub x 29 public-input bytes (any length up to 2^VERIFY_B3_LEVELS chunks): the BLAKE3 tree with the chaining
// values of complete subtrees in lv[level] -- indexed only by compile-time constants (selects), so the stack stays in registers
__device__ __forceinline__ void pub_digest(const uint8_t* pub, uint32_t npub, uint32_t out[8]) {
  constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  constexpr uint32_t CHUNK_START = 1, CHUNK_END = 2, PARENT = 4, ROOT = 8;
  const uint32_t len = 29u * npub;
  const uint32_t nchunks = len ? (len + 1023) / 1024 : 1;
  uint32_t lv[VERIFY_B3_LEVELS][8];
#pragma unroll
  for (uint32_t l = 0; l < VERIFY_B3_LEVELS; ++l)
#pragma unroll
    for (int i = 0; i < 8; ++i) lv[l][i] = 0;
  uint32_t cv[8], m[16];
#pragma unroll 1
  for (uint32_t c = 0; c < nchunks; ++c) {
    const uint32_t c_off = 1024 * c, c_len = min(1024u, len - c_off);
    const uint32_t nblocks = c_len ? (c_len + 63) / 64 : 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) cv[i] = IV[i];
#pragma unroll 1
    for (uint32_t b = 0; b < nblocks; ++b) {
      pub_block(pub, len, c_off + 64 * b, m);
      const bool last = b + 1 == nblocks;
      const uint32_t fl = (b == 0 ? CHUNK_START : 0u) | (last ? CHUNK_END : 0u) | (last && nchunks == 1 ? ROOT : 0u);
      b3d::compress(cv, m, last ? c_len - 64 * b : 64u, fl, c);
    }
    if (c + 1 == nchunks) break;
    // more chunks follow: merge the complete subtrees below this one (binary increment of the chunk count)
    uint32_t l = 0;
#pragma unroll 1
    while ((c >> l) & 1u) {
#pragma unroll
      for (uint32_t q = 0; q < VERIFY_B3_LEVELS; ++q)
        if (q == l) {
#pragma unroll
          for (int i = 0; i < 8; ++i) { m[i] = lv[q][i]; m[8 + i] = cv[i]; }
        }
#pragma unroll
      for (int i = 0; i < 8; ++i) cv[i] = IV[i];
      b3d::compress(cv, m, 64, PARENT);
      ++l;
    }
#pragma unroll
    for (uint32_t q = 0; q < VERIFY_B3_LEVELS; ++q)
      if (q == l) {
#pragma unroll
        for (int i = 0; i < 8; ++i) lv[q][i] = cv[i];
      }
  }
  // finalise: the last chunk folded into the pending subtrees, smallest first; the last parent is the root
  const uint32_t rest = nchunks - 1;
#pragma unroll 1
  for (uint32_t l = 0; rest >> l; ++l) {
    if (!((rest >> l) & 1u)) continue;
#pragma unroll
    for (uint32_t q = 0; q < VERIFY_B3_LEVELS; ++q)
      if (q == l) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { m[i] = lv[q][i]; m[8 + i] = cv[i]; }
      }
#pragma unroll
    for (int i = 0; i < 8; ++i) cv[i] = IV[i];
    b3d::compress(cv, m, 64, PARENT | ((rest >> (l + 1)) ? 0u : ROOT));
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = cv[i];
}

// The front half of SRS::verify for one proof (k_verify_rlc_prep, k_verify_trace): decode P and K, the FrBits range checks of a0
// and b0, canonical public inputs, then (only for a well-formed proof) the transcript alpha and the scalars u0, v0.  The
// DVP_VERIFY_* validity bits are k_verify's; f.h_pi is H(public inputs), which the random-linear-combination coefficient binds as
// well.  This is a copy of k_verify's first half, not shared with it: k_verify calling a shared function compiles to another
// register allocation (70 -> 33 AGPRs, 69 -> 104 spilled SGPRs), so k_verify keeps its own text and the two must be changed together.
// It comes in two parts so that the caller can store the decoded points before the transcript: verify_decode, then (for a
// well-formed proof only) verify_scalars.
struct VerifyFront {
  Fr u0, v0;
  uint32_t h_pi[8];
};
// the values between the transcript and the scalars, for a caller that reports them (k_verify_trace); canonical
struct VerifyStages {
  Fr alpha, i0, r0;
};

__device__ __forceinline__ uint32_t verify_decode(const uint8_t* pr, const Fr* pi, uint32_t npub, const GfSqrTables& T, const GfLdsK& L,
                                                  int rule, Aff& P, bool& p_inf, Aff& Kp, bool& k_inf) {
  uint32_t bad = 0;
  if (!codec_decode(pr, rule, T, L, P, p_inf)) bad |= DVP_VERIFY_BAD_COMMIT_P;
  if (!codec_decode(pr + 30, rule, T, L, Kp, k_inf)) bad |= DVP_VERIFY_BAD_KZG_K;
  if (!fr_below_p(load29(pr + 60))) bad |= DVP_VERIFY_BAD_A0;
  if (!fr_below_p(load29(pr + 89))) bad |= DVP_VERIFY_BAD_B0;
#pragma unroll 1
  for (uint32_t j = 0; j < npub; ++j)
    if (!fr_below_p(pi[j])) bad |= DVP_VERIFY_BAD_PUBLIC;
  return bad;
}

// alpha = Transcript::output: H(H_ct || H(H(commit_p) || H(pub))), top four bytes cleared (src/proving.rs:164-197); commit_p is the
// 30 bytes at pr, h_pi receives H(pub)
__device__ __forceinline__ Fr verify_challenge(const uint8_t* pr, const Fr* pi, uint32_t npub, const VerifyConsts& K, uint32_t h_pi[8]) {
  Fr alpha;
  uint32_t blk[16], h_wc[8], h_rt[8], out[8];
#pragma unroll
  for (int k = 0; k < 16; ++k) blk[k] = 0;
#pragma unroll
  for (int b = 0; b < 30; ++b) blk[b >> 2] |= (uint32_t)pr[b] << (8 * (b & 3));
  b3d::hash_chunk(blk, 30, h_wc);
  pub_digest((const uint8_t*)pi, npub, h_pi);
#pragma unroll
  for (int k = 0; k < 8; ++k) { blk[k] = h_wc[k]; blk[8 + k] = h_pi[k]; }
  b3d::hash_chunk(blk, 64, h_rt);
#pragma unroll
  for (int k = 0; k < 8; ++k) { blk[k] = K.h_ct.w[k]; blk[8 + k] = h_rt[k]; }
  b3d::hash_chunk(blk, 64, out);
#pragma unroll
  for (int k = 0; k < 7; ++k) alpha.v[k] = out[k];
  alpha.v[7] = 0;  // 224 bits, always < p
  return alpha;
}

// i0 = sum_j pub_j alpha^j by Horner (canonical: mont_mul(x, c R) = x c)
__device__ __forceinline__ Fr verify_horner(const Fr* pi, uint32_t npub, const Fr& alpha) {
  const Fr alpha_m = fr_to_mont(alpha);
  Fr i0 = fr_zero();
#pragma unroll 1
  for (uint32_t j = npub; j-- > 0;) i0 = fr_add(fr_mul(i0, alpha_m), pi[j]);
  return i0;
}

__device__ __forceinline__ void verify_scalars(const uint8_t* pr, const Fr* pi, uint32_t npub, const VerifyConsts& K, VerifyFront& f,
                                               VerifyStages* st = nullptr) {
  const Fr a0 = load29(pr + 60), b0 = load29(pr + 89);
  const Fr alpha = verify_challenge(pr, pi, npub, K, f.h_pi);
  // scalars (canonical throughout)
  const Fr i0 = verify_horner(pi, npub, alpha);
  const Fr r0 = fr_sub(fr_mul(a0, fr_to_mont(b0)), i0);
  f.u0 = fr_mul(fr_add(fr_add(a0, fr_mul(b0, K.delta_m)), fr_mul(r0, K.delta2_m)), K.eps_m);
  f.v0 = fr_mul(fr_sub(K.tau, alpha), K.eps_m);
  if (st) {
    st->alpha = alpha;
    st->i0 = i0;
    st->r0 = r0;
  }
}

}  // namespace dvp
