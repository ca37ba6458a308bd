// BLAKE3 on the device, one lane per hash (hash mode only, written from the BLAKE3 specification like blake3.h, the host
// flavour): prove.hip's k_transcript and verify.hip's k_verify.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvp {
namespace b3d {
struct Words8 { uint32_t w[8]; };
__device__ __forceinline__ uint32_t rotr(uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); }
#define DVP_B3G(a, b, c, d, mx, my)                      \
  do {                                                   \
    s[a] = s[a] + s[b] + (mx); s[d] = rotr(s[d] ^ s[a], 16); \
    s[c] = s[c] + s[d];        s[b] = rotr(s[b] ^ s[c], 12); \
    s[a] = s[a] + s[b] + (my); s[d] = rotr(s[d] ^ s[a], 8);  \
    s[c] = s[c] + s[d];        s[b] = rotr(s[b] ^ s[c], 7);  \
  } while (0)
// one compression (chunk counter < 2^32; 0 for a single-chunk hash and for parent nodes): cv' = first eight output words
__device__ __forceinline__ void compress(uint32_t cv[8], const uint32_t blk[16], uint32_t block_len, uint32_t flags, uint32_t counter = 0) {
  constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  constexpr int PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  uint32_t s[16], m[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = cv[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[8 + i] = IV[i];
  s[12] = counter; s[13] = 0; s[14] = block_len; s[15] = flags;
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = blk[i];
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    DVP_B3G(0, 4, 8, 12, m[0], m[1]); DVP_B3G(1, 5, 9, 13, m[2], m[3]); DVP_B3G(2, 6, 10, 14, m[4], m[5]); DVP_B3G(3, 7, 11, 15, m[6], m[7]);
    DVP_B3G(0, 5, 10, 15, m[8], m[9]); DVP_B3G(1, 6, 11, 12, m[10], m[11]); DVP_B3G(2, 7, 8, 13, m[12], m[13]); DVP_B3G(3, 4, 9, 14, m[14], m[15]);
    if (r < 6) {
      uint32_t t[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) t[i] = m[PERM[i]];
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = t[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) cv[i] = s[i] ^ s[i + 8];
}
#undef DVP_B3G
// BLAKE3 of `len` <= 1024 bytes held as zero-padded little-endian words
__device__ __forceinline__ void hash_chunk(const uint32_t* words, uint32_t len, uint32_t out[8]) {
  constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = IV[i];
  const uint32_t nblocks = len ? (len + 63) / 64 : 1;
#pragma unroll 1
  for (uint32_t b = 0; b < nblocks; ++b) {
    uint32_t blk[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) blk[i] = words[16 * b + i];
    const bool last = b + 1 == nblocks;
    compress(out, blk, last ? len - 64 * b : 64u, (b == 0 ? 1u : 0u) | (last ? (2u | 8u) : 0u));  // CHUNK_START | CHUNK_END | ROOT
  }
}
}  // namespace b3d

}  // namespace dvp
