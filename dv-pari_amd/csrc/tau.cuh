// tau-adic recoding of sect233k1 scalars (shared by msm.hip and codec.hip).
//
// On K-233 (a = 0, mu = -1) the Frobenius tau(x,y) = (x^2,y^2) satisfies tau^2 + tau + 2 = 0 and acts
// on E[r] as multiplication by lambda (the root of x^2+x+2 mod r with tau(G) = lambda*G).  A scalar
// s is first reduced modulo delta = (tau^233 - 1)/(tau - 1) (Solinas' partial reduction, with a
// 256-bit fixed-point reciprocal instead of an exact rounding: any rho = s (mod delta) is valid, the
// rounding only affects the length) and then expanded in base tau with digits {0,1}:
// x^2 + x + 2 is a canonical-number-system polynomial, so the expansion is finite and unique.
// The reference gets the same effect inside xs233's xsk233_mul_frob (src/curve.rs:118-123).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.cuh"  // DVP_FR_P_LIMBS

namespace dvp {

// constants: oracle/pyref.py tau_constants()
// delta = D0 + D1*tau, N(delta) = r;  conj(delta) = (D0 - D1) - D1*tau;  A_i = floor(|conj_i| 2^256 / r)
static __constant__ uint32_t TAU_D0[4] = {0xba75bb3bu, 0xda32c0f4u, 0x2dcb0ed1u, 0x00032540u};
static __constant__ uint32_t TAU_D1[4] = {0xcb36bee6u, 0x16aa143cu, 0x2d7ae36eu, 0x000882d7u};
static __constant__ uint32_t TAU_C0M[4] = {0x10c103abu, 0x3c775348u, 0xffafd49cu, 0x00055d96u};  // D1 - D0
static __constant__ uint32_t TAU_A0[5] = {0x55720891u, 0x90218207u, 0x3878eea6u, 0x2dff5fa9u, 0x00000abbu};
static __constant__ uint32_t TAU_A1[5] = {0xcb1ecea9u, 0x79966d7du, 0xdc2d5428u, 0xae5af5c6u, 0x00001105u};
// TAU_DIGITS = 240 is a PROVEN bound on the length of the expansion, not an observed one (observed maximum: 236):
//   rho = s - kappa*delta with kappa_i = round(s c_i / r) computed through a 256-bit fixed-point reciprocal, so
//   rho/delta = e0 + e1 tau with |e_i| <= 1/2 + 2^-24, hence N(rho) = N(delta) (e0^2 - e0 e1 + 2 e1^2) <= r (1 + 2^-21)
//   and |rho| = sqrt(N(rho)) < 2^115.51 (r < 2^231.01).  One expansion step maps rho to (rho - u)/tau, u in {0,1}, and
//   |tau| = sqrt 2, so |rho_(k+1)| <= (|rho_k| + 1)/sqrt 2, i.e. |rho_k| < |rho_0| 2^(-k/2) + 1/(sqrt 2 - 1).  After
//   k = 233 steps |rho_233| < 2^(115.51-116.5) + 2.4143 < 2.92, so N(rho_233) <= 8; every element of Z[tau] of norm
//   <= 9 has an expansion of at most 7 digits (exhaustive enumeration, tests/test_oracle.py::test_tau_length_bound).
//   Total <= 233 + 7 = 240.  The windows of both MSM modes cover >= 240 digits (msm.hip: MsmFixedCtx::set_c keeps an
//   overflow window of c >= 8 digits above digit 234; msm_plan adds ceil(6/c) overflow windows), so the "expansion
//   longer than the windows" flag of k_recode cannot fire for a canonical scalar; it stays as an internal check.
constexpr int TAU_DIGITS = 240;

// out[0..no) = low `no` limbs of a[0..na) * b[0..nb)
template <int NA, int NB, int NO>
__device__ __forceinline__ void mp_mul_lo(const uint32_t* a, const uint32_t* b, uint32_t* out) {
#pragma unroll
  for (int i = 0; i < NO; ++i) out[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (i + j < NO) {
        c += (uint64_t)a[i] * b[j] + out[i + j];
        out[i + j] = (uint32_t)c;
        c >>= 32;
      }
    }
    if (i + NB < NO) out[i + NB] = (uint32_t)c;
  }
}

// Q = round(s * A / 2^256), s: 8 limbs, A: 5 limbs -> 4 limbs (value < 2^117)
__device__ __forceinline__ void tau_round_mul(const uint32_t* s, const uint32_t* A, uint32_t* Q) {
  uint32_t t[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      c += (uint64_t)s[i] * A[j] + t[i + j];
      t[i + j] = (uint32_t)c;
      c >>= 32;
    }
    t[i + 5] = (uint32_t)c;
  }
  // + 2^255, then >> 256
  uint64_t c = (uint64_t)t[7] + 0x80000000u;
  c >>= 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c += t[8 + i];
    Q[i] = (uint32_t)c;
    c >>= 32;
  }
}


// s < r ?
__device__ __forceinline__ bool tau_scalar_is_canonical(const uint32_t* s) {
  const uint32_t p[8] = DVP_FR_P_LIMBS;
  uint64_t borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint64_t t = (uint64_t)s[k] - p[k] - borrow;
    borrow = (t >> 63) & 1;
  }
  return borrow != 0;
}

// rho = r0 + r1*tau = s (mod delta); components are 160-bit two's complement, |r_i| < 2^118
__device__ __forceinline__ void tau_partial_reduce(const uint32_t* s, uint32_t* r0, uint32_t* r1) {
  uint32_t Q0[4], Q1[4];
  tau_round_mul(s, TAU_A0, Q0);
  tau_round_mul(s, TAU_A1, Q1);
  // rho0 = s + Q0*D0 - 2*Q1*D1 ; rho1 = Q0*D1 - Q1*(D1-D0)      (mod 2^160)
  uint32_t t0[5], t1[5];
  mp_mul_lo<4, 4, 5>(Q0, TAU_D0, t0);
  mp_mul_lo<4, 4, 5>(Q1, TAU_D1, t1);
  {
    uint64_t cy = 0;
    int64_t bw = 0;
    uint32_t acc[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {  // s + t0
      cy += (uint64_t)s[k] + t0[k];
      acc[k] = (uint32_t)cy;
      cy >>= 32;
    }
    uint32_t prev = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {  // - 2*t1
      uint32_t d = (t1[k] << 1) | prev;
      prev = t1[k] >> 31;
      int64_t v = (int64_t)acc[k] - d + bw;
      r0[k] = (uint32_t)v;
      bw = v >> 32;
    }
  }
  mp_mul_lo<4, 4, 5>(Q0, TAU_D1, t0);
  mp_mul_lo<4, 4, 5>(Q1, TAU_C0M, t1);
  {
    int64_t bw = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      int64_t v = (int64_t)t0[k] - t1[k] + bw;
      r1[k] = (uint32_t)v;
      bw = v >> 32;
    }
  }
}

// one digit: u = rho mod tau in {0,1}; rho <- (rho - u)/tau, i.e. (r0,r1) <- (r1 - h, -h), h = (r0-u)/2
__device__ __forceinline__ uint32_t tau_step(uint32_t* r0, uint32_t* r1) {
  uint32_t u = r0[0] & 1u;
  uint32_t h[5];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = (r0[k] >> 1) | (r0[k + 1] << 31);
  h[4] = (uint32_t)((int32_t)r0[4] >> 1);
  int64_t b1 = 0, b2 = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    int64_t v = (int64_t)r1[k] - h[k] + b1;
    r0[k] = (uint32_t)v;
    b1 = v >> 32;
    int64_t z = (int64_t)0 - h[k] + b2;
    r1[k] = (uint32_t)z;
    b2 = z >> 32;
  }
  return u;
}

// sixteen digits at once.  The digits depend only on the low bits of (r0, r1), so they come from a 32-bit copy of the
// one-digit recurrence (after j steps the low 32-j bits are still exact); then rho <- (rho - D) / tau^16 in one
// multi-limb pass: D = sum d_i tau^i = p + q tau by Horner, tau^16 = 178 - 93 tau, N(tau^16) = 2^16 and
// conj(tau^16) = 271 + 93 tau, so with x = r0 - p, y = r1 - q:
//     r0' = (271 x - 186 y) / 2^16,   r1' = (93 x + 178 y) / 2^16          (exact divisions).
// ~3x fewer instructions than sixteen tau_step calls.  Returns the digits, digit i in bit i.
__device__ __forceinline__ uint32_t tau_step16(uint32_t* r0, uint32_t* r1) {
  uint32_t lo0 = r0[0], lo1 = r1[0], dw = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    uint32_t u = lo0 & 1u;
    uint32_t h = (lo0 - u) >> 1;
    lo0 = lo1 - h;
    lo1 = 0u - h;
    dw |= u << i;
  }
  int32_t p = 0, q = 0;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    int32_t d = (int32_t)((dw >> i) & 1u);
    int32_t np = d - 2 * q, nq = p - q;
    p = np;
    q = nq;
  }
  // x = r0 - p, y = r1 - q (5-limb two's complement), then the two linear combinations with carries in int64
  uint32_t x[5], y[5];
  {
    int64_t bx = -(int64_t)p, by = -(int64_t)q;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      bx += (int64_t)(uint64_t)r0[k];
      x[k] = (uint32_t)bx;
      bx >>= 32;
      by += (int64_t)(uint64_t)r1[k];
      y[k] = (uint32_t)by;
      by >>= 32;
    }
  }
  uint32_t n0[5], n1[5];
  int64_t c0 = 0, c1 = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    // limbs 0..3 are unsigned digits, limb 4 carries the sign
    int64_t xv = k < 4 ? (int64_t)(uint64_t)x[k] : (int64_t)(int32_t)x[k];
    int64_t yv = k < 4 ? (int64_t)(uint64_t)y[k] : (int64_t)(int32_t)y[k];
    c0 += 271 * xv - 186 * yv;
    c1 += 93 * xv + 178 * yv;
    n0[k] = (uint32_t)c0;
    n1[k] = (uint32_t)c1;
    c0 >>= 32;
    c1 >>= 32;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r0[k] = (n0[k] >> 16) | (n0[k + 1] << 16);
    r1[k] = (n1[k] >> 16) | (n1[k + 1] << 16);
  }
  r0[4] = (uint32_t)((int32_t)n0[4] >> 16);
  r1[4] = (uint32_t)((int32_t)n1[4] >> 16);
  return dw;
}

// ---- width-w tau-NAF (Solinas 2000, section 5.3/6, for mu = -1) of a partially reduced scalar: points_mul.hip ----------------------------
// rho = sum_j s_j alpha_(u_j) tau^j with s_j in {+1, -1}, u_j odd < 2^(w-1), at most one non-zero digit among any w consecutive
// positions.  alpha_u = beta_u + gamma_u tau = u mods tau^w: the element of least norm in u + tau^w Z[tau].  One step: rho odd (r0 odd)
// -> u = (r0 + r1 t_w) mods 2^w, where t_w is the integer with tau = t_w (mod tau^w) (the EVEN root of t^2 + t + 2 mod 2^w: tau is
// no unit modulo tau^w), rho <- rho - sign(u) alpha_|u|, which tau^w divides; then rho <- rho / tau (tau_step on an even r0).
// Nothing here is typed in: t_w, alpha_u and the tail length below are derived from tau^2 = -tau - 2 at compile time.
struct ZTau {
  int a, b;  // a + b tau
};
constexpr ZTau ztau_mul(ZTau x, ZTau y) { return ZTau{x.a * y.a - 2 * x.b * y.b, x.a * y.b + x.b * y.a - x.b * y.b}; }
constexpr int ztau_norm(ZTau x) { return x.a * x.a - x.a * x.b + 2 * x.b * x.b; }
constexpr ZTau ztau_pow_tau(int w) {
  ZTau x{1, 0};
  for (int i = 0; i < w; ++i) x = ztau_mul(x, ZTau{0, 1});
  return x;
}
constexpr int tnaf_tw(int w) {
  for (int t = 0; t < (1 << w); t += 2)
    if (((t * t + t + 2) & ((1 << w) - 1)) == 0) return t;
  return -1;
}
constexpr int tnaf_iabs(int v) { return v < 0 ? -v : v; }
constexpr int TNAF_MAX_ENTRIES = 8;  // w <= 5
struct TnafTable {
  int w, tw, entries;  // entries = 2^(w-2): entry e holds alpha_(2e+1)
  int beta[TNAF_MAX_ENTRIES], gamma[TNAF_MAX_ENTRIES];
  int max_norm;
};
// least norm over u - q tau^w, q in a box that holds the nearest lattice points; ties go to the smallest (|beta|, |gamma|, beta, gamma)
constexpr TnafTable tnaf_make(int w) {
  TnafTable t{};
  t.w = w;
  t.tw = tnaf_tw(w);
  t.entries = 1 << (w - 2);
  t.max_norm = 0;
  const ZTau tp = ztau_pow_tau(w);
  for (int e = 0; e < t.entries; ++e) {
    const int u = 2 * e + 1;
    bool have = false;
    int bn = 0, bb = 0, bg = 0;
    for (int q0 = -4; q0 <= 4; ++q0)
      for (int q1 = -4; q1 <= 4; ++q1) {
        const ZTau m = ztau_mul(ZTau{q0, q1}, tp);
        const ZTau c{u - m.a, -m.b};
        const int n = ztau_norm(c);
        bool better = !have || n < bn;
        if (have && n == bn) {
          const int k0[4] = {tnaf_iabs(c.a), tnaf_iabs(c.b), c.a, c.b}, k1[4] = {tnaf_iabs(bb), tnaf_iabs(bg), bb, bg};
          for (int i = 0; i < 4; ++i) {
            if (k0[i] != k1[i]) {
              better = k0[i] < k1[i];
              break;
            }
          }
        }
        if (better) {
          have = true;
          bn = n;
          bb = c.a;
          bg = c.b;
        }
      }
    t.beta[e] = bb;
    t.gamma[e] = bg;
    if (bn > t.max_norm) t.max_norm = bn;
  }
  return t;
}
// digits of the expansion of one small element (0 = the recoding did not end within `cap` steps)
constexpr int tnaf_small_len(const TnafTable& t, ZTau rho, int cap) {
  int n = 0;
  while (rho.a != 0 || rho.b != 0) {
    if (n == cap) return 0;
    if (rho.a & 1) {
      int u = (rho.a + rho.b * t.tw) & ((1 << t.w) - 1);
      if (u >= (1 << (t.w - 1))) u -= 1 << t.w;
      const int s = u > 0 ? 1 : -1, e = (tnaf_iabs(u) - 1) / 2;
      rho.a -= s * t.beta[e];
      rho.b -= s * t.gamma[e];
    }
    const int h = rho.a / 2;  // exact: rho.a is even here
    rho = ZTau{rho.b - h, -h};
    ++n;
  }
  return n;
}
// the longest expansion among the elements of norm <= nb (-1 = one of them does not end): N(a + b tau) >= 7 a^2 / 8 and >= 7 b^2 / 4,
// so |a|, |b| <= 16 covers every norm up to 224
constexpr int tnaf_tail_len(const TnafTable& t, int nb) {
  int mx = 0;
  for (int a = -16; a <= 16; ++a)
    for (int b = -16; b <= 16; ++b) {
      if (ztau_norm(ZTau{a, b}) > nb) continue;
      if (a == 0 && b == 0) continue;
      const int n = tnaf_small_len(t, ZTau{a, b}, 64);
      if (n == 0) return -1;
      if (n > mx) mx = n;
    }
  return mx;
}
// TnafDigits<W>::value is a PROVEN bound on the number of digit positions, in the style of TAU_DIGITS above:
//   |rho_0| < 2^115.51 (the partial reduction: see TAU_DIGITS).  One step maps rho to (rho - d) / tau with d = 0 or +-alpha_u, so with
//   A = sqrt(max_u N(alpha_u)) (max norm 2, 8, 16 for w = 3, 4, 5):  |rho_(k+1)| <= (|rho_k| + A) / sqrt 2, hence
//   |rho_k| < |rho_0| 2^(-k/2) + A / (sqrt 2 - 1).  After k = 233 steps |rho_233| < 2^(-0.99) + 2.41422 A, i.e.
//   N(rho_233) <= NB = (0.5035 + 2.41422 A)^2: 15, 53, 103 for w = 3, 4, 5 (tnaf_norm_bound rounds UP, to 16, 54, 104).
//   Every element of norm <= NB has an expansion of at most TAIL = 6, 8, 9 digits: exhaustive enumeration at compile time
//   (tnaf_tail_len, which also shows that each of them ends).  Total <= 233 + TAIL = 239, 241, 242; observed maximum 234.
// The non-zero digits are at least w positions apart (tau^w divides rho after a subtraction), so there are at most
// ceil(value / w) of them: TnafDigits<W>::max_nonzero.
constexpr int tnaf_norm_bound(int max_norm) {
  // ceil((0.5035 + 2.41422 sqrt(max_norm))^2) + 1 with sqrt rounded up by Newton's iteration from above
  double s = max_norm > 1 ? (double)max_norm : 1.0;
  for (int i = 0; i < 60; ++i) s = 0.5 * (s + (double)max_norm / s);
  s *= 1.0 + 1e-12;
  const double b = 0.5035 + 2.41422 * s;
  return (int)(b * b) + 1;
}
template <int W>
struct TnafDigits {
  static_assert(W >= 3 && W <= 5, "window width");
  static constexpr TnafTable table = tnaf_make(W);
  static constexpr int tail = tnaf_tail_len(table, tnaf_norm_bound(table.max_norm));
  static_assert(tail > 0, "an element of small norm whose tau-NAF does not end");
  static constexpr int value = 233 + tail;
  static constexpr int max_nonzero = (value + W - 1) / W;
};
static_assert(TnafDigits<3>::value == 239 && TnafDigits<4>::value == 241 && TnafDigits<5>::value == 242, "the bound the comment states");

// one position of the width-W tau-NAF of rho = r0 + r1 tau (160-bit two's complement, as tau_partial_reduce leaves them): returns the
// signed digit (0, or +-u with u odd < 2^(W-1)) and replaces rho by (rho - digit's alpha) / tau.  Branch-free.
template <int W>
__device__ __forceinline__ int tnaf_step(uint32_t* r0, uint32_t* r1) {
  constexpr TnafTable t = TnafDigits<W>::table;
  const uint32_t odd = r0[0] & 1u;
  const uint32_t uu = (r0[0] + r1[0] * (uint32_t)t.tw) & ((1u << W) - 1);
  const int su = ((int)uu - (int)((uu >> (W - 1)) << W)) * (int)odd;  // mods 2^W; 0 for an even rho
  const int au = su < 0 ? -su : su;
  int b = 0, g = 0;
#pragma unroll
  for (int e = 0; e < t.entries; ++e) {
    if (au == 2 * e + 1) {
      b = t.beta[e];
      g = t.gamma[e];
    }
  }
  if (su < 0) {
    b = -b;
    g = -g;
  }
  // rho -= (b + g tau): small signed integers into the five limbs
  int64_t c0 = -(int64_t)b, c1 = -(int64_t)g;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    c0 += (int64_t)(uint64_t)r0[k];
    r0[k] = (uint32_t)c0;
    c0 >>= 32;
    c1 += (int64_t)(uint64_t)r1[k];
    r1[k] = (uint32_t)c1;
    c1 >>= 32;
  }
  (void)tau_step(r0, r1);  // r0 is even now: the division alone
  return su;
}

}  // namespace dvp
