// dvp_debug_fr_op (include/dvpari_internal.h): ONE function of fr.cuh per element, on raw 256-bit values, either in a kernel (one
// element per lane: the device build of the function as every kernel gets it, the explicit v_mad_u64_u32 chains included) or in a
// host loop over the same DVP_HD functions (no HIP call: runs on a machine without a GPU).  tests/fr_cases.py holds the integer
// reference and the case sets; nothing on a proof path calls this file.
#include <cstring>

#include "common.h"
#include "fr.cuh"

namespace dvp {

// inputs / outputs an op reads and writes (index = enum dvp_fr_op)
constexpr int FROP_N_IN[DVP_FROP_COUNT] = {2, 2, 1, 1, 1, 1, 2, 1, 1, 1, 4, 3, 2, 1, 1, 1, 1, 2, 3, 6, 1, 1, 1, 2, 1, 1};
constexpr int FROP_N_OUT[DVP_FROP_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1};

template <int OP>
DVP_HD void fr_debug_apply(const Fr* x, Fr* y) {
  switch (OP) {
    case DVP_FROP_ADD: y[0] = fr_add(x[0], x[1]); break;
    case DVP_FROP_SUB: y[0] = fr_sub(x[0], x[1]); break;
    case DVP_FROP_NEG: y[0] = fr_neg(x[0]); break;
    case DVP_FROP_DBL: y[0] = fr_dbl(x[0]); break;
    case DVP_FROP_COND_SUB_P: y[0] = fr_cond_sub_p(x[0]); break;
    case DVP_FROP_IS_CANONICAL:
      y[0] = fr_zero();
      y[0].v[0] = fr_is_canonical(x[0]) ? 1u : 0u;
      break;
    case DVP_FROP_MUL: y[0] = fr_mul(x[0], x[1]); break;
    case DVP_FROP_SQR: y[0] = fr_sqr(x[0]); break;
    case DVP_FROP_TO_MONT: y[0] = fr_to_mont(x[0]); break;
    case DVP_FROP_FROM_MONT: y[0] = fr_from_mont(x[0]); break;
    case DVP_FROP_DOT2: y[0] = fr_dot2(fr29_from(x[0]), fr29_from(x[1]), fr29_from(x[2]), fr29_from(x[3])); break;
    case DVP_FROP_MULADD29: y[0] = fr_muladd29(fr29_from(x[0]), fr29_from(x[1]), fr29_from(x[2])); break;
    case DVP_FROP_MUL29: y[0] = fr_mul29(fr29_from(x[0]), fr29_from(x[1])); break;
    case DVP_FROP_ROUNDTRIP29: {
      uint32_t l[8];
      fr_to29(x[0], l);
      y[0] = fr_from29(l);
      break;
    }
    case DVP_FROP_ROUNDTRIP30: y[0] = fr30_to_fr(fr30_from(x[0])); break;
    case DVP_FROP_CONST30: y[0] = fr30_to_fr(fr30_const(x[0])); break;
    case DVP_FROP_CANON30: y[0] = fr30_canon(fr30_from(x[0])); break;
    case DVP_FROP_SUB_LAZY30: y[0] = fr30_to_fr(fr30_sub_lazy(fr30_from(x[0]), fr30_from(x[1]))); break;
    case DVP_FROP_MULADD30: y[0] = fr30_to_fr(fr30_muladd(fr30_from(x[0]), fr30_from(x[1]), fr30_from(x[2]))); break;
    case DVP_FROP_MULADD30_X2: {
      Fr30 r0, r1;
      fr30_muladd_x2(fr30_from(x[0]), fr30_from(x[1]), fr30_from(x[2]), fr30_from(x[3]), fr30_from(x[4]), fr30_from(x[5]), r0, r1);
      y[0] = fr30_to_fr(r0);
      y[1] = fr30_to_fr(r1);
      break;
    }
    case DVP_FROP_INV: y[0] = fr_inv(x[0]); break;
    case DVP_FROP_INV_GCD_RAW: y[0] = fr_inv_gcd_raw(x[0]); break;
    case DVP_FROP_INV_FERMAT: y[0] = fr_inv_fermat(x[0]); break;
    case DVP_FROP_POW_U64: y[0] = fr_pow_u64(x[0], (uint64_t)x[1].v[0] | ((uint64_t)x[1].v[1] << 32)); break;
    case DVP_FROP_LIMBS29: fr_to29(x[0], y[0].v); break;
    case DVP_FROP_LIMBS30: {
      const Fr30 s = fr30_from(x[0]);
#pragma unroll
      for (int i = 0; i < 8; ++i) y[0].v[i] = s.l[i];
      break;
    }
    default: break;
  }
}

struct FrDebugPtrs {
  const Fr* in[6];
  Fr* out[2];
};

template <int OP>
__global__ void __launch_bounds__(256) k_fr_debug(FrDebugPtrs p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr x[6], y[2];
#pragma unroll
  for (int k = 0; k < FROP_N_IN[OP]; ++k) x[k] = p.in[k][i];
  fr_debug_apply<OP>(x, y);
#pragma unroll
  for (int k = 0; k < FROP_N_OUT[OP]; ++k) p.out[k][i] = y[k];
}

template <int OP>
static void fr_debug_host(const uint64_t* const* in, size_t n, uint64_t* const* out) {
  for (size_t i = 0; i < n; ++i) {
    Fr x[6], y[2];
    for (int k = 0; k < FROP_N_IN[OP]; ++k) memcpy(x[k].v, in[k] + 4 * i, 32);
    fr_debug_apply<OP>(x, y);
    for (int k = 0; k < FROP_N_OUT[OP]; ++k) memcpy(out[k] + 4 * i, y[k].v, 32);
  }
}

template <int OP>
static void fr_debug_launch(const FrDebugPtrs& p, size_t n) {
  DVP_LAUNCH((k_fr_debug<OP>), dim3(cdiv(n, 256)), dim3(256), 0, 0, p, n);
}

// ---- the preconditions, in plain integer compares on the host (no function under test decides them, bar one: see MULADD30) --------
static bool lt_limbs(const Fr& a, const uint32_t* b) {  // a < b, both 8 x 32 bits
  for (int i = 7; i >= 0; --i)
    if (a.v[i] != b[i]) return a.v[i] < b[i];
  return false;
}
static bool lt_p_shl(const Fr& a, int s) {  // a < p * 2^s, s <= 7
  constexpr uint32_t p[8] = DVP_FR_P_LIMBS;
  uint32_t b[8];
  for (int i = 0; i < 8; ++i) b[i] = s ? (p[i] << s) | (i ? p[i - 1] >> (32 - s) : 0u) : p[i];
  return lt_limbs(a, b);
}
static bool lt_pow2(const Fr& a, int bits) {  // a < 2^bits, bits < 256
  for (int i = 7; i >= 0; --i) {
    const int lo = 32 * i;
    if (lo >= bits) {
      if (a.v[i]) return false;
    } else if (bits - lo < 32) {
      if (a.v[i] >> (bits - lo)) return false;
    }
  }
  return true;
}

static bool fr_debug_precondition(int op, const Fr* x) {
  switch (op) {
    case DVP_FROP_ADD: case DVP_FROP_SUB: case DVP_FROP_MUL: case DVP_FROP_MUL29: return lt_p_shl(x[0], 0) && lt_p_shl(x[1], 0);
    case DVP_FROP_NEG: case DVP_FROP_DBL: case DVP_FROP_SQR: case DVP_FROP_TO_MONT: case DVP_FROP_FROM_MONT:
    case DVP_FROP_INV: case DVP_FROP_INV_GCD_RAW: case DVP_FROP_INV_FERMAT: case DVP_FROP_CONST30: return lt_p_shl(x[0], 0);
    case DVP_FROP_COND_SUB_P: case DVP_FROP_CANON30: return lt_p_shl(x[0], 1);
    case DVP_FROP_IS_CANONICAL: return true;
    case DVP_FROP_DOT2: return lt_p_shl(x[0], 0) && lt_p_shl(x[1], 0) && lt_p_shl(x[2], 0) && lt_p_shl(x[3], 0);
    case DVP_FROP_MULADD29: return lt_p_shl(x[0], 0) && lt_p_shl(x[1], 0) && lt_p_shl(x[2], 0);
    case DVP_FROP_ROUNDTRIP29: case DVP_FROP_LIMBS29: return lt_pow2(x[0], 232);
    case DVP_FROP_ROUNDTRIP30: case DVP_FROP_LIMBS30: return lt_pow2(x[0], 240);
    case DVP_FROP_SUB_LAZY30: return lt_pow2(x[0], 239) && lt_p_shl(x[1], 7);
    case DVP_FROP_MULADD30: case DVP_FROP_MULADD30_X2:
      for (int k = 0; k < (op == DVP_FROP_MULADD30 ? 3 : 6); k += 3) {
        if (!lt_p_shl(x[k], 0) || !lt_pow2(x[k + 1], 240) || !lt_pow2(x[k + 2], 240)) return false;
        // a b / R' + (at most p) + c < 2p + 2^240 < 2^241 fits limb 7's 32 bits, so the host product is exact here and its limb 7
        // tells whether the result stays below 2^240
        if (fr30_muladd(fr30_from(x[k]), fr30_from(x[k + 1]), fr30_from(x[k + 2])).l[7] >> 30) return false;
      }
      return true;
    case DVP_FROP_POW_U64: return lt_p_shl(x[0], 0) && lt_pow2(x[1], 64);
    default: return false;
  }
}

}  // namespace dvp

using namespace dvp;

#define DVP_FROP_EACH(X)                                                                                                       \
  X(DVP_FROP_ADD) X(DVP_FROP_SUB) X(DVP_FROP_NEG) X(DVP_FROP_DBL) X(DVP_FROP_COND_SUB_P) X(DVP_FROP_IS_CANONICAL) X(DVP_FROP_MUL)   \
  X(DVP_FROP_SQR) X(DVP_FROP_TO_MONT) X(DVP_FROP_FROM_MONT) X(DVP_FROP_DOT2) X(DVP_FROP_MULADD29) X(DVP_FROP_MUL29)               \
  X(DVP_FROP_ROUNDTRIP29) X(DVP_FROP_ROUNDTRIP30) X(DVP_FROP_CONST30) X(DVP_FROP_CANON30) X(DVP_FROP_SUB_LAZY30) X(DVP_FROP_MULADD30) \
  X(DVP_FROP_MULADD30_X2) X(DVP_FROP_INV) X(DVP_FROP_INV_GCD_RAW) X(DVP_FROP_INV_FERMAT) X(DVP_FROP_POW_U64) X(DVP_FROP_LIMBS29)   \
  X(DVP_FROP_LIMBS30)

extern "C" int dvp_debug_fr_op(int op, const uint64_t* const in[6], size_t n, int on_device, uint64_t* const out[2]) {
  if (op < 0 || op >= DVP_FROP_COUNT || !in || !out) return DVP_EINVAL;
  if (!n) return DVP_OK;
  const int n_in = FROP_N_IN[op], n_out = FROP_N_OUT[op];
  for (int k = 0; k < n_in; ++k)
    if (!in[k]) return DVP_EINVAL;
  for (int k = 0; k < n_out; ++k)
    if (!out[k]) return DVP_EINVAL;
  for (size_t i = 0; i < n; ++i) {
    Fr x[6];
    for (int k = 0; k < n_in; ++k) memcpy(x[k].v, in[k] + 4 * i, 32);
    if (!fr_debug_precondition(op, x)) {
      g_last_error_index = (int64_t)i;
      return DVP_EINVAL;
    }
  }
  if (!on_device) {
    switch (op) {
#define X(OP) case OP: fr_debug_host<OP>(in, n, out); break;
      DVP_FROP_EACH(X)
#undef X
    }
    return DVP_OK;
  }
  DevBuf d_in[6], d_out[2];
  FrDebugPtrs p = {};
  for (int k = 0; k < n_in; ++k) {
    DVP_TRY(d_in[k].up(in[k], n * sizeof(Fr)));
    p.in[k] = d_in[k].as<Fr>();
  }
  for (int k = 0; k < n_out; ++k) {
    DVP_TRY(d_out[k].alloc(n * sizeof(Fr)));
    p.out[k] = d_out[k].as<Fr>();
  }
  switch (op) {
#define X(OP) case OP: fr_debug_launch<OP>(p, n); break;
    DVP_FROP_EACH(X)
#undef X
  }
  DVP_HIP(hipGetLastError());
  for (int k = 0; k < n_out; ++k) DVP_TRY(d_out[k].down(out[k], n * sizeof(Fr)));
  return DVP_OK;
}
