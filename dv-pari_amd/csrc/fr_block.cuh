// The one block-wide sum of Fr values: every kernel that folds one Fr per lane (the barycentric and dot-product partials and finals of
// fr_ops.hip, the prover's k_bary3_*, the verifier's combination sum) goes through it.  Fr addition returns the canonical
// representative, so a sum does not depend on the shape of the tree.
#pragma once
#include "fr.cuh"

namespace dvp {

// A two-level sum over a vector: level 1 is at most FR_SUM_BLOCKS blocks of FR_SUM_LANES lanes, each lane striding the vector by the
// whole grid, level 2 one block over their partials.  A vector longer than FR_SUM_LANES * FR_SUM_BLOCKS makes lanes take a second
// element (srs_check.hip sizes its level 1 by these; the tests read them from here).
constexpr uint32_t FR_SUM_LANES = 256;
constexpr uint32_t FR_SUM_BLOCKS = 1024;

// sum over a 256-lane block of one Fr per lane, through sh[256]: every lane gets the total, and the closing barrier leaves sh free for
// the next call.  (Callers unroll their loop over the three sums: a runtime index put s[] / res[] into 112 B of scratch per lane.)
__device__ __forceinline__ Fr block_sum256(const Fr& x, Fr* sh) {
  sh[threadIdx.x] = x;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fr_add(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  const Fr total = sh[0];
  __syncthreads();
  return total;
}

}  // namespace dvp
