// MSM recode: the entry-word layout of the fixed-base mode (FXW_*, ITEM_NEG), the tau-adic recoder k_recode<DIGIT> and
// the signed binary recoder (fx_recode_signed_each, fx_load_scalar, k_recode_signed).  Part of msm.hip's translation unit: msm.hip
// includes it, and its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include "common.h"
#include "tau.cuh"

namespace dvp {

// Entry word of the fixed-base mode (one u32 per (slot, scalar)): bit 31 = valid, bits 20..27 = row of the pre-rotated
// table (the power of tau the base is taken at), bits 0..19 = bucket key.  0 = empty slot.
// Bit 28 = the entry SUBTRACTS its point (signed-digit flavours): carried into bit 31 of the sorted item (ITEM_NEG) and applied
// where the point is loaded (-(x, y) = (x, x + y): free).
constexpr uint32_t FXW_VALID = 0x80000000u, FXW_KEY_MASK = 0xfffffu, FXW_NEG = 0x10000000u, ITEM_NEG = 0x80000000u;
constexpr int FXW_ROW_SHIFT = 20;
__host__ __device__ __forceinline__ uint32_t fxw_key(uint32_t d) { return d & FXW_KEY_MASK; }
__host__ __device__ __forceinline__ uint32_t fxw_row(uint32_t d) { return (d >> FXW_ROW_SHIFT) & 0xffu; }

// One thread per scalar: digits[w][i] (c-bit patterns) + bucket histogram.
// Scalars >= r are rejected (flag); points flagged infinite contribute nothing.
template <class DIGIT>
__global__ void __launch_bounds__(256)
k_recode(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t n, int c, int W, int n_narrow,
         DIGIT* __restrict__ digits, unsigned long long* __restrict__ err) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = scalars[(size_t)i * 8 + k];
  bool skip = inf && inf[i];
  if (!tau_scalar_is_canonical(s)) {
    atomicMin(err, (unsigned long long)i);
    skip = true;
  }
  uint32_t r0[5], r1[5];
  tau_partial_reduce(s, r0, r1);
  if (skip) {
#pragma unroll
    for (int k = 0; k < 5; ++k) r0[k] = r1[k] = 0;
  }
  // expansion: u = r0 & 1; r0 -= u; h = r0 >> 1 (arithmetic); (r0, r1) = (r1 - h, -h)
  // windows 0 .. n_narrow-1 are c-1 digits wide, the rest c (fixed-base mode evens the windows out, see MsmFixedCtx).
  // Digits arrive sixteen at a time (tau_step16) into a 64-bit shift register; windows are cut from its low end.
  const int total = W * c - n_narrow;
  uint64_t buf = 0;
  int nb = 0, w = 0, width = n_narrow > 0 ? c - 1 : c;
  for (int done = 0; done < total; done += 16) {
    buf |= (uint64_t)tau_step16(r0, r1) << nb;
    nb += 16;
    while (nb >= width && w < W) {
      const uint32_t dv = (uint32_t)(buf & ((1ull << width) - 1));
      if (sizeof(DIGIT) == 4)  // fixed-base mode: entry word = valid | table row | bucket key (see FXW_*)
        digits[(size_t)w * n + i] = (DIGIT)(dv ? (FXW_VALID | ((uint32_t)w << FXW_ROW_SHIFT) | dv) : 0u);
      else
        digits[(size_t)w * n + i] = (DIGIT)dv;
      buf >>= width;
      nb -= width;
      ++w;
      width = w < n_narrow ? c - 1 : c;
    }
  }
  uint32_t rest = (uint32_t)buf | (uint32_t)(buf >> 32);  // digits beyond the last window
#pragma unroll
  for (int k = 0; k < 5; ++k) rest |= r0[k] | r1[k];
  if (rest) atomicMin(err, (unsigned long long)i | (1ull << 62));  // expansion longer than W*c digits
}

// Signed aligned windows over the BINARY digits (MsmFixedCtx::signed_digits; table row w = 2^(o_w) P): the
// textbook signed-digit bucket method.  Window w holds d_w = bits [c w, c w + c) plus the carry of the window below; a digit
// above 2^(c-1) becomes d_w - 2^c with a carry of one, so |d_w| <= 2^(c-1): HALF the buckets per window bit of the unsigned
// windows (key = |d_w|; |d_w| = 2^(c-1), probability 2^-c, shares key 0, whose bucket the tail weighs by 2^(c-1)), the sign
// travels with the entry (FXW_NEG) and is applied when the point is loaded.  W = ceil(234 / c) windows take a canonical scalar
// (< 2^232) including the last carry.  No tau-adic expansion: a few shifts per window.
// the entry words of one scalar, window by window: f(w, word), word == 0 where the window contributes nothing.  Returns the last carry
// (zero for a canonical scalar: the widths add up to >= 234).
template <class F>
__device__ __forceinline__ uint32_t fx_recode_signed_each(const uint32_t* s /* 9 words, s[8] = 0 */, int c, int W, int n_narrow, F&& f) {
  // the n_narrow LOW windows are c - 1 bits wide, the rest c (widths evened out so that the 234 bits fill every window: a short
  // top window would send every scalar into a handful of buckets)
  uint32_t carry = 0;
  int bit = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int width = w < n_narrow ? c - 1 : c;
    const uint32_t half = 1u << (width - 1), mask = (1u << width) - 1;
    const int wd = bit >> 5, sh = bit & 31;
    uint32_t lo = wd < 8 ? s[wd] : 0u, hi = wd + 1 < 9 ? s[wd + 1] : 0u;
    uint32_t d = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & mask;
    bit += width;
    d += carry;
    carry = 0;
    uint32_t word = 0;
    if (d > mask) {  // all ones + carry: digit 0, carry on
      carry = 1;
    } else if (d > half) {  // d - 2^width < 0
      carry = 1;
      d = (1u << width) - d;  // |d| in [1, 2^(width-1))
      word = FXW_VALID | FXW_NEG | ((uint32_t)w << FXW_ROW_SHIFT) | d;
    } else if (d) {
      word = FXW_VALID | ((uint32_t)w << FXW_ROW_SHIFT) | (d & ((1u << (c - 1)) - 1));  // a full-width d == 2^(c-1) -> key 0
    }
    f(w, word);
  }
  return carry;
}
// loads scalar i; false = it contributes no entries (neutral base, or not canonical -- `report` then records its index)
__device__ __forceinline__ bool fx_load_scalar(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t i, uint32_t* s,
                                               unsigned long long* __restrict__ err, bool report) {
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = scalars[(size_t)i * 8 + k];
  s[8] = 0;
  bool skip = inf && inf[i];
  if (!tau_scalar_is_canonical(s)) {
    if (report) atomicMin(err, (unsigned long long)i);
    skip = true;
  }
  return !skip;
}
__global__ void __launch_bounds__(256)
k_recode_signed(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t n, int c, int W, int n_narrow,
                uint32_t* __restrict__ words, unsigned long long* __restrict__ err) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[9];
  const bool live = fx_load_scalar(scalars, inf, i, s, err, true);
  const uint32_t carry = fx_recode_signed_each(s, c, W, n_narrow, [&](int w, uint32_t word) { words[(size_t)w * n + i] = live ? word : 0u; });
  if (carry && live) atomicMin(err, (unsigned long long)i | (1ull << 62));  // cannot happen: the widths add up to >= 234
}

}  // namespace dvp
