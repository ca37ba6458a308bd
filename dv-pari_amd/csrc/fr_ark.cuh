// Fr as arkworks holds it in memory <-> the canonical limbs of the ABI, one element at a time.
//
// The crate's Fr is Fp256<MontBackend<FqConfig, 4>> (src/curve.rs:16-22): four little-endian u64 holding a 2^256 mod p, always below p.
// Read as eight 32-bit words on a little-endian machine that is the ABI's own limb order, so the two maps are
//
//   fr_from_ark_words: out = (x mod p) 2^-256 mod p        fr_to_ark_words: out = (a mod p) 2^256 mod p
//
// for ANY x, a < 2^256: the input is reduced first (fr_reduce_le_words, fr_wire.cuh -- a no-op on what arkworks stores), which leaves no
// error path and keeps fr_mul's "operands below 2^232" true whatever the bytes are; then ONE fr_mul (x y 2^-232) by a constant
// (fr.cuh: DVP_FR_2M24_LIMBS, DVP_FR_2P488_LIMBS).  The results are canonical.  The same source on the host (dvp_debug_fr_ark_host) and
// in k_fr_from_ark / k_fr_to_ark (fr_ark.hip).
#pragma once
#include "fr.cuh"
#include "fr_wire.cuh"

namespace dvp {

DVP_HD void fr_from_ark_words(const uint32_t in[8], uint32_t out[8]) {
  constexpr uint32_t k[8] = DVP_FR_2M24_LIMBS;
  Fr x, c;
  fr_reduce_le_words(in, x.v);
#pragma unroll
  for (int i = 0; i < 8; ++i) c.v[i] = k[i];
  const Fr r = fr_mul(x, c);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = r.v[i];
}

DVP_HD void fr_to_ark_words(const uint32_t in[8], uint32_t out[8]) {
  constexpr uint32_t k[8] = DVP_FR_2P488_LIMBS;
  Fr a, c;
  fr_reduce_le_words(in, a.v);
#pragma unroll
  for (int i = 0; i < 8; ++i) c.v[i] = k[i];
  const Fr r = fr_mul(a, c);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = r.v[i];
}

// is the arkworks-form element at `ark` (32 bytes, any alignment) the field's one, 2^256 mod p in any representative below 2^256?
// The constant wire of an assignment (src/proving.rs:449-452) as a host that keeps [1, public.., private..] in one Vec<Fr> holds it.
DVP_HD bool fr_ark_is_one(const uint8_t* ark) {
  constexpr uint32_t one[8] = DVP_FR_2P256_LIMBS;
  uint32_t w[8], r[8];
  __builtin_memcpy(w, ark, 32);
  fr_reduce_le_words(w, r);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= r[i] ^ one[i];
  return o == 0;
}

}  // namespace dvp
