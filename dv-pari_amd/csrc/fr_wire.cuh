// gnark_element_to_fr (src/gnark_r1cs.rs:58-77) on one element: 32 bytes big-endian, any x < 2^256, -> x mod p as the canonical
// 8 x 32-bit little-endian limbs of the ABI.  Exactly Fr::from_be_bytes_mod_order, without a loop over bits and without a division:
//
//   p = 2^231 + c, c = limbs 0..3 of DVP_FR_P_LIMBS (fr.cuh; 115 bits).  Write x = q 2^231 + r with q = x >> 231 < 2^25, r < 2^231.
//   2^231 = p - c, so x = q p + (r - q c): x mod p is r - q c when r >= q c, and r - q c + p otherwise.  Both lie in [0, p):
//   q c < 2^140 < p, so r - q c + p > 0, and r - q c < 2^231 < p.
//
// q c is four 32 x 32 -> 64 products (v_mad_u64_u32 on the device), the subtraction one borrow chain, the correction a masked add of p:
// no branch, the same source on the host (cache.cpp's file entry, dvp_debug_fr_from_be32_host) and in k_fr_from_be32 (fr_wire.hip).
#pragma once
#include <stdint.h>

#include "fr.cuh"  // DVP_FR_P_LIMBS

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DVP_WIRE_HD __host__ __device__ __forceinline__
#else
#define DVP_WIRE_HD inline
#endif

namespace dvp {

// The reduction itself, on a value that is little-endian already: le[k] = bits 32k .. 32k+31 of any x < 2^256, out = x mod p, canonical
// (the arkworks-form entries of fr_ark.cuh reduce with it before they scale).
DVP_WIRE_HD void fr_reduce_le_words(const uint32_t le[8], uint32_t out[8]) {
  constexpr uint32_t P32[8] = DVP_FR_P_LIMBS;
  uint32_t x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = le[i];
  const uint32_t q = x[7] >> 7;  // bit 231 is bit 7 of limb 7
  x[7] &= 0x7fu;                 // r
  uint32_t t[8];                 // q c: limbs 0..3 of c are those of p, the carry out of limb 3 is limb 4 (q c < 2^140)
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc += (uint64_t)q * P32[i];  // < 2^57 + 2^32
    t[i] = (uint32_t)acc;
    acc >>= 32;
  }
  t[4] = (uint32_t)acc;
  t[5] = t[6] = t[7] = 0;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)x[i] - t[i] - borrow;
    x[i] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
  const uint32_t mask = 0u - borrow;  // r < q c: add p back (the carry out of limb 7 cancels the borrow)
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t s = (uint64_t)x[i] + (P32[i] & mask) + carry;
    out[i] = (uint32_t)s;
    carry = (uint32_t)(s >> 32);
  }
}

// be[k] = the k-th 32-bit word of the 32 bytes as a little-endian machine loads it (be[0] holds the four most significant bytes)
DVP_WIRE_HD void fr_from_be32_words(const uint32_t be[8], uint32_t out[8]) {
  constexpr uint32_t P32[8] = DVP_FR_P_LIMBS;
  uint32_t x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = __builtin_bswap32(be[7 - i]);  // byte reversal = word reversal + a swap inside each word
  // from here on the body of fr_reduce_le_words, repeated: calling it instead moves k_fr_from_be32's device code (same size, other bytes)
  const uint32_t q = x[7] >> 7;
  x[7] &= 0x7fu;
  uint32_t t[8];
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc += (uint64_t)q * P32[i];
    t[i] = (uint32_t)acc;
    acc >>= 32;
  }
  t[4] = (uint32_t)acc;
  t[5] = t[6] = t[7] = 0;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)x[i] - t[i] - borrow;
    x[i] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
  const uint32_t mask = 0u - borrow;
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t s = (uint64_t)x[i] + (P32[i] & mask) + carry;
    out[i] = (uint32_t)s;
    carry = (uint32_t)(s >> 32);
  }
}

// does the element at `be` (32 bytes, any alignment) reduce to 1?  The constant wire of a witness (src/proving.rs:449-452): the one
// element the host looks at, in dvp_prove_be32 and, before cache_dir is opened, in dvp_prove_cache_dir_witness_file
DVP_WIRE_HD bool fr_be32_is_one(const uint8_t* be) {
  uint32_t w[8], r[8];
  __builtin_memcpy(w, be, 32);
  fr_from_be32_words(w, r);
  return r[0] == 1 && (r[1] | r[2] | r[3] | r[4] | r[5] | r[6] | r[7]) == 0;
}

}  // namespace dvp
