// ECFFT, stage 1: the curve, the leaves L_0[i] = x(coset + i g) and the layers L_(d+1) = psi_d(L_d) of a context (ecfft_init).
// Part of ecfft.hip's translation unit: included once, its host code at global scope behind `using namespace dvp` (map: top of ecfft.hip).
#pragma once
#include "ecfft_internal.h"

namespace dvp {

// ---- constants from src/ec_fft.rs:205-229 (canonical limbs) -----------------------------------
// a = 2125753088427212854352924174339172498722499297750753614229533284661082
constexpr uint32_t ECFFT_A_CANON[8] = {0xace0775au, 0x44fd5f67u, 0x76ead179u, 0x030cf18fu,
                                       0xaff1f871u, 0xd2776c4bu, 0xd93b829fu, 0x0000004eu};
// subgroup generator (order 2^28)
constexpr uint32_t ECFFT_GX_CANON[8] = {0xd0a7e150u, 0xb8963584u, 0x9981c323u, 0x88c5a0ceu,
                                        0xe7ba27e5u, 0x87f53e0eu, 0x0c8ea06bu, 0x00000049u};
constexpr uint32_t ECFFT_GY_CANON[8] = {0xec5cc36eu, 0x779340c8u, 0x3c4ec51bu, 0x92c4b0adu,
                                        0x94bbcf10u, 0xe10365e3u, 0x0a0d1e5fu, 0x00000022u};
// coset offset
constexpr uint32_t ECFFT_CX_CANON[8] = {0x7608b3eau, 0x786f6278u, 0xd29e01e1u, 0x4da67d47u,
                                        0x62d59c79u, 0xac90a9e4u, 0xc2a60c19u, 0x00000039u};
constexpr uint32_t ECFFT_CY_CANON[8] = {0x6d514258u, 0xd5063f88u, 0xe1bcc7d2u, 0x0be9eee3u,
                                        0x3f498728u, 0xb4efdffeu, 0x6bdc81edu, 0x00000055u};
constexpr int ECFFT_LOG_ORDER = 28;  // subgroup_adic, src/ec_fft.rs:205

static Fr fr_from_limbs_mont(const uint32_t* c) {
  Fr r;
  for (int i = 0; i < 8; ++i) r.v[i] = c[i];
  return fr_to_mont(r);
}

// ---- host-side short-Weierstrass affine arithmetic (only O(log N) of it) -----------------------
struct SwPt {
  Fr x, y;  // Montgomery
  bool inf;
};
static SwPt sw_add(const SwPt& p, const SwPt& q, const Fr& a) {
  if (p.inf) return q;
  if (q.inf) return p;
  Fr lam;
  if (fr_eq(p.x, q.x)) {
    if (fr_is_zero(fr_add(p.y, q.y))) return SwPt{fr_zero(), fr_zero(), true};
    Fr x2 = fr_sqr(p.x);
    Fr num = fr_add(fr_add(fr_dbl(x2), x2), a);
    lam = fr_mul(num, fr_inv(fr_dbl(p.y)));
  } else {
    lam = fr_mul(fr_sub(q.y, p.y), fr_inv(fr_sub(q.x, p.x)));
  }
  SwPt r;
  r.inf = false;
  r.x = fr_sub(fr_sub(fr_sqr(lam), p.x), q.x);
  r.y = fr_sub(fr_mul(lam, fr_sub(p.x, r.x)), p.y);
  return r;
}

// ---- device kernels ----------------------------------------------------------------------------

// leaves[i] = x(coset + i*g), i < n.  tab[j] = 2^j * g (affine, Montgomery).  Jacobian mixed adds
// (madd-2007-bl); no exceptional case can occur because coset is outside the subgroup <g>.
__global__ void __launch_bounds__(256) k_leaves(const Fr* __restrict__ tab_x, const Fr* __restrict__ tab_y, Fr cx, Fr cy,
                         int log_n, Fr* __restrict__ out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr X = cx, Y = cy, Z = fr_one_mont();
  for (int j = 0; j < log_n; ++j) {
    if (!((i >> j) & 1)) continue;
    Fr x2 = tab_x[j], y2 = tab_y[j];
    Fr z1z1 = fr_sqr(Z);
    Fr u2 = fr_mul(x2, z1z1);
    Fr s2 = fr_mul(fr_mul(y2, Z), z1z1);
    Fr h = fr_sub(u2, X);
    Fr hh = fr_sqr(h);
    Fr i4 = fr_dbl(fr_dbl(hh));
    Fr jj = fr_mul(h, i4);
    Fr r = fr_dbl(fr_sub(s2, Y));
    Fr v = fr_mul(X, i4);
    Fr x3 = fr_sub(fr_sub(fr_sqr(r), jj), fr_dbl(v));
    Fr y3 = fr_sub(fr_mul(r, fr_sub(v, x3)), fr_dbl(fr_mul(Y, jj)));
    Fr z3 = fr_sub(fr_sub(fr_sqr(fr_add(Z, h)), z1z1), hh);
    X = x3; Y = y3; Z = z3;
  }
  Fr zi = fr_inv(Z);
  out[i] = fr_mul(X, fr_sqr(zi));
}

// next[i] = psi(cur[i]) = cur[i] + t/(cur[i]-x0), i < half
__global__ void __launch_bounds__(256) k_next_layer(const Fr* __restrict__ cur, Fr x0, Fr t, Fr* __restrict__ next, uint32_t half) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= half) return;
  Fr x = cur[i];
  next[i] = fr_add(x, fr_mul(t, fr_inv(fr_sub(x, x0))));
}

}  // namespace dvp

static const int TPB = 256;

// the isogeny chain on the host (O(log N) curve operations), then the leaves and every layer below them on the device
static int ecfft_init(dvp_ecfft* c, uint32_t log_n, int shifted, uint32_t base_log) {
  c->log_n = (int)log_n;
  c->n_leaves = 1u << log_n;
  DVP_HIP(hipGetDevice(&c->device));
  const uint32_t N = c->n_leaves;
  Fr a = fr_from_limbs_mont(ECFFT_A_CANON);
  SwPt G{fr_from_limbs_mont(ECFFT_GX_CANON), fr_from_limbs_mont(ECFFT_GY_CANON), false};
  SwPt C{fr_from_limbs_mont(ECFFT_CX_CANON), fr_from_limbs_mont(ECFFT_CY_CANON), false};
  // g = 2^(28-log_n) * G  (src/ec_fft.rs:116-119); base generator for the D' shift (:72-82,151-155)
  SwPt g = G;
  for (int i = 0; i < ECFFT_LOG_ORDER - (int)log_n; ++i) g = sw_add(g, g, a);
  if (shifted) {
    SwPt bg = G;
    for (int i = 0; i < ECFFT_LOG_ORDER - (int)base_log; ++i) bg = sw_add(bg, bg, a);
    C = sw_add(C, bg, a);
  }
  // tab[j] = 2^j g ; tab[log_n-j] has order 2^j
  std::vector<SwPt> tab(log_n);
  tab[0] = g;
  for (uint32_t j = 1; j < log_n; ++j) tab[j] = sw_add(tab[j - 1], tab[j - 1], a);
  if (!fr_is_zero(tab[log_n - 1].y)) return DVP_EINVAL;  // order-2 point must have y == 0
  // q[j-1] = x of the point of order 2^j; pushed through the isogenies as we go
  std::vector<Fr> q(log_n);
  for (uint32_t j = 1; j <= log_n; ++j) q[j - 1] = tab[log_n - j].x;
  c->x0.resize(log_n);
  c->t.resize(log_n);
  Fr acur = a;
  for (uint32_t d = 0; d < log_n; ++d) {
    Fr x0 = q[d];
    Fr x0sq = fr_sqr(x0);
    Fr t = fr_add(fr_add(fr_dbl(x0sq), x0sq), acur);  // 3 x0^2 + a_d
    c->x0[d] = x0;
    c->t[d] = t;
    for (uint32_t j = d + 1; j < log_n; ++j) q[j] = fr_add(q[j], fr_mul(t, fr_inv(fr_sub(q[j], x0))));
    Fr t5 = fr_add(fr_dbl(fr_dbl(t)), t);
    acur = fr_sub(acur, t5);  // a_{d+1} = a_d - 5t
  }
  // device: layers
  c->layer_off.resize(log_n + 1);
  size_t off = 0;
  for (uint32_t d = 0; d <= log_n; ++d) {
    c->layer_off[d] = off;
    off += (size_t)(N >> d);
  }
  DVP_HIP(hipMalloc((void**)&c->layers, off * sizeof(Fr)));
  {
    std::vector<Fr> tx(log_n), ty(log_n);
    for (uint32_t j = 0; j < log_n; ++j) { tx[j] = tab[j].x; ty[j] = tab[j].y; }
    DevBuf dx, dy;
    DVP_TRY(dx.up(tx.data(), log_n * sizeof(Fr)));
    DVP_TRY(dy.up(ty.data(), log_n * sizeof(Fr)));
    DVP_LAUNCH(k_leaves, dim3(cdiv(N, TPB)), dim3(TPB), 0, 0, dx.as<Fr>(), dy.as<Fr>(), C.x, C.y, (int)log_n,
                       c->layer(0), N);
    for (uint32_t d = 0; d < log_n; ++d) {
      uint32_t half = (N >> d) >> 1;
      DVP_LAUNCH(k_next_layer, dim3(cdiv(half, TPB)), dim3(TPB), 0, 0, c->layer(d), c->x0[d], c->t[d],
                         c->layer(d + 1), half);
    }
    DVP_HIP(hipGetLastError());
    DVP_HIP(hipDeviceSynchronize());
  }
  return DVP_OK;
}
