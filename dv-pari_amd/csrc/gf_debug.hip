// dvp_debug_gf_op (include/dvpari_internal.h): ONE function of gf233.cuh or k233.cuh per element, on raw 256-bit values, in a kernel
// launched as the production kernels are (256-thread workgroups, the multipliers' dynamic LDS per wave, the tables of
// gf_sqr_tables()).  A lane -- a quad, a row of 16 lanes for GfLdsQ / GfLdsH -- works through several elements one after the other, so
// an element finds the previous one's table in its LDS region, as an addition chain of a production kernel does.
// tests/gf_cases.py holds the case sets, oracle/pyref.py is the reference; nothing on a proof path calls this file.
//
// What this does NOT test: the functions are compiled here under THIS kernel's register allocation and schedule.  The code generated
// for them inside k_affine_round, k_merge and the other production kernels (spills, the order of LDS operations around inlined
// products) is a different compilation of the same source; the MSM, codec and verify tests remain the check of those.
#include <cstring>
#include <type_traits>

#include "common.h"
#include "k233.cuh"
#include "host_api.h"

namespace dvp {

// values an op reads / writes (index = enum dvp_gf_op); a flag goes to out[3] on top of the values
constexpr int GFOP_N_IN[DVP_GFOP_COUNT] = {2, 2, 3, 1, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, 3, 5, 5, 4, 6, 6, 3, 3, 3, 6, 3, 3};
constexpr int GFOP_N_OUT[DVP_GFOP_COUNT] = {1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2};
constexpr bool gfop_has_flag(int op) {
  return op == DVP_GFOP_LD_MADD_FAST || op == DVP_GFOP_LD_ADD_NODBL || op == DVP_GFOP_LAM_ADD || op == DVP_GFOP_LD_TO_AFF;
}
// the forms an op exists in
constexpr bool gfop_valid(int op, int form) {
  switch (op) {
    case DVP_GFOP_MUL: case DVP_GFOP_LD_DBL: case DVP_GFOP_LD_MADD: case DVP_GFOP_LD_ADD: return true;
    case DVP_GFOP_MUL2: case DVP_GFOP_INV_FAST: case DVP_GFOP_LD_MADD_FAST: case DVP_GFOP_LD_ADD_AFF_AFF: case DVP_GFOP_LD_ADD_NODBL:
    case DVP_GFOP_LAM_FROM_LD: case DVP_GFOP_LAM_TO_LD: case DVP_GFOP_LAM_DBL: case DVP_GFOP_LAM_ADD: return form != DVP_GFFORM_REG;
    default: return form == DVP_GFFORM_REG;
  }
}

struct GfReg {};  // DVP_GFFORM_REG: no multiplier state
template <int FORM> struct GfForm;
template <> struct GfForm<DVP_GFFORM_REG> {
  typedef GfReg LT;
  static constexpr uint32_t G = 1, LDS_PER_WAVE = 0;
  static GF_DEV LT init(char*) { return GfReg{}; }
};
template <> struct GfForm<DVP_GFFORM_LDS> {
  typedef GfLds LT;
  static constexpr uint32_t G = 1, LDS_PER_WAVE = GF_LDS_BYTES_PER_WAVE;
  static GF_DEV LT init(char* lds) { return gf_lds_init(lds); }
};
template <> struct GfForm<DVP_GFFORM_LDSQ> {
  typedef GfLdsQ LT;
  static constexpr uint32_t G = 4, LDS_PER_WAVE = GF_LDS_BYTES_PER_WAVE;
  static GF_DEV LT init(char* lds) { return gf_ldsq_init(lds); }
};
template <> struct GfForm<DVP_GFFORM_LDSH> {
  typedef GfLdsH LT;
  static constexpr uint32_t G = 16, LDS_PER_WAVE = GF_LDS_BYTES_PER_WAVE;
  static GF_DEV LT init(char* lds) { return gf_ldsh_init(lds); }
};
template <> struct GfForm<DVP_GFFORM_LDSK> {
  typedef GfLdsK LT;
  static constexpr uint32_t G = 1, LDS_PER_WAVE = GF_LDSK_BYTES_PER_WAVE;
  static GF_DEV LT init(char* lds) { return gf_ldsk_init(lds); }
};
constexpr uint32_t GFFORM_G[DVP_GFFORM_COUNT] = {1, 1, 4, 16, 1};

GF_DEV Gf gf_flag(bool b) {
  Gf r = gf_zero();
  r.w[0] = b ? 1u : 0u;
  return r;
}

template <int OP, class LT>
GF_DEV void gf_debug_apply(const Gf* x, Gf* y, uint32_t param, const GfSqrTables& T, const LT& L) {
  constexpr bool REG = std::is_same<LT, GfReg>::value;
  Ld p, q;
  p.X = x[0]; p.Y = x[1]; p.Z = x[2];
  q.X = x[3]; q.Y = x[4]; q.Z = x[5];
  Aff qa;
  qa.x = x[3]; qa.y = x[4];
  if constexpr (OP == DVP_GFOP_ADD) {
    y[0] = gf_add(x[0], x[1]);
  } else if constexpr (OP == DVP_GFOP_MUL) {
    if constexpr (REG) y[0] = gf_mul(x[0], x[1]); else y[0] = gf_mul(x[0], x[1], L);
  } else if constexpr (OP == DVP_GFOP_MUL2) {
    gf_mul2(x[0], x[1], x[2], L, y[0], y[1]);
  } else if constexpr (OP == DVP_GFOP_SQR) {
    y[0] = gf_sqr(x[0]);
  } else if constexpr (OP == DVP_GFOP_SQR_N) {
    y[0] = gf_sqr_n(x[0], (int)param);
  } else if constexpr (OP == DVP_GFOP_REDUCE16_15 || OP == DVP_GFOP_REDUCE16_14) {
    uint32_t c[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      c[i] = x[0].w[i];
      c[8 + i] = x[1].w[i];
    }
    y[0] = gf_reduce16<OP == DVP_GFOP_REDUCE16_15 ? 15 : 14>(c);
  } else if constexpr (OP == DVP_GFOP_SQR_TAB) {
    const uint32_t sel = param & 0xffu;
    const Gf* tab = sel == 0 ? T.t29 : sel == 1 ? T.t58 : sel == 2 ? T.t116 : sel == 3 ? T.th : sel == 4 ? T.t14 : T.t7;
    if (param & 0x100u) y[0] = gf_sqr_tab_wide(x[0], tab); else y[0] = gf_sqr_tab(x[0], tab);
  } else if constexpr (OP == DVP_GFOP_SQR_N_FAST) {
    y[0] = gf_sqr_n_fast(x[0], (int)param, T);
  } else if constexpr (OP == DVP_GFOP_INV) {
    y[0] = gf_inv(x[0]);
  } else if constexpr (OP == DVP_GFOP_INV_FAST) {
    y[0] = gf_inv_fast(x[0], T, L);
  } else if constexpr (OP == DVP_GFOP_SQRT) {
    y[0] = gf_sqrt(x[0]);
  } else if constexpr (OP == DVP_GFOP_TRACE) {
    y[0] = gf_flag(gf_trace(x[0]) != 0u);
  } else if constexpr (OP == DVP_GFOP_HALFTRACE) {
    y[0] = gf_halftrace(x[0]);
  } else if constexpr (OP == DVP_GFOP_LD_DBL) {
    if constexpr (REG) p = ld_dbl(p); else p = ld_dbl(p, L);
  } else if constexpr (OP == DVP_GFOP_LD_MADD) {
    if constexpr (REG) p = ld_madd(p, qa); else p = ld_madd(p, qa, L);
  } else if constexpr (OP == DVP_GFOP_LD_MADD_FAST) {
    y[3] = gf_flag(ld_madd_fast(p, qa, L));
  } else if constexpr (OP == DVP_GFOP_LD_ADD_AFF_AFF) {
    Aff pa, qb;
    pa.x = x[0]; pa.y = x[1];
    qb.x = x[2]; qb.y = x[3];
    ld_add_aff_aff(pa, qb, p, L);
  } else if constexpr (OP == DVP_GFOP_LD_ADD) {
    if constexpr (REG) p = ld_add(p, q); else p = ld_add(p, q, L);
  } else if constexpr (OP == DVP_GFOP_LD_ADD_NODBL) {
    y[3] = gf_flag(ld_add_nodbl(p, q, L));
  } else if constexpr (OP == DVP_GFOP_LAM_FROM_LD) {
    lam_from_ld(p, L);
  } else if constexpr (OP == DVP_GFOP_LAM_TO_LD) {
    lam_to_ld(p, L);
  } else if constexpr (OP == DVP_GFOP_LAM_DBL) {
    lam_dbl_ip(p, L);
  } else if constexpr (OP == DVP_GFOP_LAM_ADD) {
    y[3] = gf_flag(lam_add_ip(p, q, L));
  } else if constexpr (OP == DVP_GFOP_LD_FROB_N) {
    p = ld_frob_n(p, (int)param);
  } else if constexpr (OP == DVP_GFOP_LD_TO_AFF) {
    Aff a;
    y[3] = gf_flag(ld_to_aff(p, &a));
    y[0] = a.x;
    y[1] = a.y;
  }
  if constexpr (OP >= DVP_GFOP_LD_DBL && OP != DVP_GFOP_LD_TO_AFF) {
    y[0] = p.X; y[1] = p.Y; y[2] = p.Z;
  }
}

struct GfDebugPtrs {
  const Gf* in[6];
  Gf* out[4];
};

// groups = groups of G lanes that get elements: group g works through the elements g, g + groups, g + 2 groups, ...; n G < 2^31
template <int OP, int FORM>
__global__ void __launch_bounds__(256) k_gf_debug(GfDebugPtrs ptr, uint32_t n, uint32_t groups, uint32_t param, GfSqrTables T) {
  extern __shared__ char lds_raw[];
  typedef GfForm<FORM> F;
  const typename F::LT L = F::init(lds_raw);
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t g = lane / F::G, r = lane % F::G;
  if (g >= groups) return;  // a whole quad / row at a time (groups are aligned)
#pragma unroll 1
  for (uint32_t e = g; e < n; e += groups) {
    Gf x[6], y[4];
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = k < GFOP_N_IN[OP] ? ptr.in[k][e] : gf_zero();
    gf_debug_apply<OP>(x, y, param, T, L);
    const size_t o = (size_t)e * F::G + r;
#pragma unroll
    for (int k = 0; k < GFOP_N_OUT[OP]; ++k) ptr.out[k][o] = y[k];
    if (gfop_has_flag(OP)) ptr.out[3][o] = y[3];
  }
}

template <int OP, int FORM>
static int gf_debug_launch(const GfDebugPtrs& p, size_t n, uint32_t param, const GfSqrTables& T) {
  if constexpr (!gfop_valid(OP, FORM)) {
    return DVP_EINVAL;
  } else {
    typedef GfForm<FORM> F;
    const uint32_t waves = (uint32_t)((n * F::G + 127) / 128);  // two elements per group where there are that many
    const uint32_t groups = (waves ? waves : 1u) * 64u / F::G;
    const uint32_t lds = 4u * F::LDS_PER_WAVE;
    if (lds) DVP_HIP(hipFuncSetAttribute((const void*)k_gf_debug<OP, FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DVP_LAUNCH((k_gf_debug<OP, FORM>), dim3(cdiv((size_t)groups * F::G, 256)), dim3(256), lds, 0, p, (uint32_t)n, groups, param, T);
    DVP_HIP(hipGetLastError());
    return DVP_OK;
  }
}
template <int OP>
static int gf_debug_launch_form(int form, const GfDebugPtrs& p, size_t n, uint32_t param, const GfSqrTables& T) {
  switch (form) {
    case DVP_GFFORM_REG: return gf_debug_launch<OP, DVP_GFFORM_REG>(p, n, param, T);
    case DVP_GFFORM_LDS: return gf_debug_launch<OP, DVP_GFFORM_LDS>(p, n, param, T);
    case DVP_GFFORM_LDSQ: return gf_debug_launch<OP, DVP_GFFORM_LDSQ>(p, n, param, T);
    case DVP_GFFORM_LDSH: return gf_debug_launch<OP, DVP_GFFORM_LDSH>(p, n, param, T);
    case DVP_GFFORM_LDSK: return gf_debug_launch<OP, DVP_GFFORM_LDSK>(p, n, param, T);
    default: return DVP_EINVAL;
  }
}

}  // namespace dvp

using namespace dvp;

#define DVP_GFOP_EACH(X)                                                                                                              \
  X(DVP_GFOP_ADD) X(DVP_GFOP_MUL) X(DVP_GFOP_MUL2) X(DVP_GFOP_SQR) X(DVP_GFOP_SQR_N) X(DVP_GFOP_REDUCE16_15) X(DVP_GFOP_REDUCE16_14)      \
  X(DVP_GFOP_SQR_TAB) X(DVP_GFOP_SQR_N_FAST) X(DVP_GFOP_INV) X(DVP_GFOP_INV_FAST) X(DVP_GFOP_SQRT) X(DVP_GFOP_TRACE) X(DVP_GFOP_HALFTRACE) \
  X(DVP_GFOP_LD_DBL) X(DVP_GFOP_LD_MADD) X(DVP_GFOP_LD_MADD_FAST) X(DVP_GFOP_LD_ADD_AFF_AFF) X(DVP_GFOP_LD_ADD) X(DVP_GFOP_LD_ADD_NODBL)  \
  X(DVP_GFOP_LAM_FROM_LD) X(DVP_GFOP_LAM_TO_LD) X(DVP_GFOP_LAM_DBL) X(DVP_GFOP_LAM_ADD) X(DVP_GFOP_LD_FROB_N) X(DVP_GFOP_LD_TO_AFF)

extern "C" int dvp_debug_gf_op(int op, int form, const uint64_t* const in[6], size_t n, uint64_t param, uint64_t* const out[4]) {
  if (op < 0 || op >= DVP_GFOP_COUNT || form < 0 || form >= DVP_GFFORM_COUNT || !gfop_valid(op, form) || !in || !out) return DVP_EINVAL;
  if (!n) return DVP_OK;
  const int n_in = GFOP_N_IN[op], n_out = GFOP_N_OUT[op];
  const bool flag = gfop_has_flag(op);
  for (int k = 0; k < n_in; ++k)
    if (!in[k]) return DVP_EINVAL;
  for (int k = 0; k < n_out; ++k)
    if (!out[k]) return DVP_EINVAL;
  if (flag && !out[3]) return DVP_EINVAL;
  const uint32_t G = GFFORM_G[form];
  if (n > (size_t)0x7fffffffu / G) return DVP_EINVAL;
  // ---- the preconditions, in plain compares on the host, before any device call -----------------------------------------------------
  g_last_error_index = -1;
  if ((op == DVP_GFOP_SQR_N || op == DVP_GFOP_SQR_N_FAST || op == DVP_GFOP_LD_FROB_N) && param > 232) return DVP_EINVAL;
  if (op == DVP_GFOP_SQR_TAB) {
    const uint64_t sel = param & 0xffu;
    if ((param & ~(uint64_t)0x1ff) || sel > 5) return DVP_EINVAL;
    const long long tabs = tune().gf_inv_tabs;  // what gf_sqr_tables() hands out: t14 from 1, t7 from 2
    if ((sel == 4 && tabs < 1) || (sel == 5 && tabs < 2)) return DVP_EINVAL;
  }
  const bool raw512 = op == DVP_GFOP_REDUCE16_15 || op == DVP_GFOP_REDUCE16_14;
  for (size_t i = 0; i < n; ++i) {
    bool ok = true;
    if (raw512) {
      if (op == DVP_GFOP_REDUCE16_14 && (in[1][4 * i + 3] >> 32)) ok = false;  // word 15
    } else {
      for (int k = 0; k < n_in; ++k)
        if (in[k][4 * i + 3] >> 41) ok = false;  // bits 233 .. 255
    }
    if (!ok) {
      g_last_error_index = (int64_t)i;
      return DVP_EINVAL;
    }
  }
  // ---- device ----------------------------------------------------------------------------------------------------------------------
  GfSqrTables T = {};
  if (op == DVP_GFOP_SQR_TAB || op == DVP_GFOP_SQR_N_FAST || op == DVP_GFOP_INV_FAST) DVP_TRY(gf_sqr_tables(&T, 0));
  DevBuf d_in[6], d_out[4];
  GfDebugPtrs p = {};
  for (int k = 0; k < n_in; ++k) {
    DVP_TRY(d_in[k].up(in[k], n * sizeof(Gf)));
    p.in[k] = d_in[k].as<Gf>();
  }
  for (int k = 0; k < 4; ++k) {
    if (!(k < n_out || (k == 3 && flag))) continue;
    DVP_TRY(d_out[k].alloc(n * G * sizeof(Gf)));
    p.out[k] = d_out[k].as<Gf>();
  }
  int rc = DVP_EINVAL;
  switch (op) {
#define X(OP) case OP: rc = gf_debug_launch_form<OP>(form, p, n, (uint32_t)param, T); break;
    DVP_GFOP_EACH(X)
#undef X
  }
  DVP_TRY(rc);
  DVP_HIP(hipDeviceSynchronize());
  for (int k = 0; k < 4; ++k)
    if (p.out[k]) DVP_TRY(d_out[k].down(out[k], n * G * sizeof(Gf)));
  return DVP_OK;
}
