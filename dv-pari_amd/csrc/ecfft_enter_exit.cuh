// ECFFT, stage 6: enter (coefficients -> evaluations) and exit (back) on the stride-2^sl0 subtree: the pointwise kernels, the tables of
// a stride level (xnn, leaf-8 matrices, enter's and exit's folded tables) and enter_core / exit_core.  Part of ecfft.hip's translation unit.
#pragma once
#include "ecfft_extend.cuh"

namespace dvp {

// enter combine (one recursion level, all sub-problems at once):
//   lo/hi evaluations u0,v0 (even leaves) and u1,v1 (odd leaves) -> res[2i]   = u0 + xnn[2i]  *v0
//                                                                   res[2i+1] = u1 + xnn[2i+1]*v1
// `even`/`odd` hold 2*nsub vectors of h values: [.. lo_c, hi_c ..]; out holds nsub vectors of 2h.
__global__ void __launch_bounds__(256) k_enter_combine(const Fr* __restrict__ even, const Fr* __restrict__ odd,
                                const Fr* __restrict__ xnn, Fr* __restrict__ out, uint32_t h, uint32_t total) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total) return;  // total = nsub*h
  uint32_t c = tid / h, i = tid - c * h;
  size_t lo = (size_t)(2 * c) * h + i, hi = lo + h;
  Fr u0 = even[lo], v0 = even[hi], u1 = odd[lo], v1 = odd[hi];
  size_t o = (size_t)c * 2 * h + 2 * i;
  out[o] = fr_add(u0, fr_mul(xnn[2 * i], v0));
  out[o + 1] = fr_add(u1, fr_mul(xnn[2 * i + 1], v1));
}

// xnn[j] = leaf_j^h over the strided tree (Montgomery)
__global__ void __launch_bounds__(256) k_pow_table(const Fr* __restrict__ L0, int sl, uint32_t sz, uint64_t e, Fr* __restrict__ out) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= sz) return;
  out[j] = fr_pow_u64(L0[(size_t)j << sl], e);
}

// (the read-outs of ecfft_debug.cuh and the input check of the host-pointer entries, ecfft.hip)
__global__ void __launch_bounds__(256) k_from_mont(const Fr* __restrict__ in, Fr* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fr_from_mont(in[i]);
}
__global__ void __launch_bounds__(256) k_check_canonical(const Fr* __restrict__ in, size_t n, unsigned long long* bad) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !fr_is_canonical(in[i])) atomicMin(bad, (unsigned long long)i);
}

// enter's combine tables of the stride-2^sl subtree (ExtIo SM 3): xe[i] = xnn[2i], t2[i] = wout[i] * xnn[2i + 1], multiplier-constant form
__global__ void __launch_bounds__(256) k_enter_fuse_tables(const Fr* __restrict__ xnn, const Fr30* __restrict__ wout, Fr30* __restrict__ xe,
                                                           Fr30* __restrict__ t2, uint32_t h) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h) return;
  xe[i] = fr30_const(xnn[2 * i]);
  // (w R') * (y R) / R' = w y R: the Montgomery form of the product, lazily reduced
  t2[i] = fr30_const(fr30_canon(fr30_muladd(wout[i], fr30_from(xnn[2 * i + 1]), fr30_zero())));
}
// The three deepest levels of enter / exit (sub-problems of 8 values: h = 4, 2, 1) as ONE pass with a constant 8 x 8 matrix (round 6):
// every sub-problem of a level lives on the same strided subtree, so enter on 8 coefficients is the Vandermonde matrix V[j][e] =
// leaf_j^e of that subtree's 8 leaves and exit is its inverse -- 72 multiply-adds per sub-problem (8 x 8 plus one per output that
// brings the lazy sum back below 2 p), one read and one write of the vector, where the recursion ran three levels of extends and
// pointwise passes (enter 3 launches, exit 9).  Same field elements: the interpolating polynomial is unique.  The matrix is uniform
// over the launch (scalar loads); a thread owns one sub-problem.
__global__ void __launch_bounds__(256) k_leaf_matmul8(const Fr* __restrict__ in, Fr* __restrict__ out, const Fr30* __restrict__ mat /* [8][8] + one */,
                                                      uint32_t nsub) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nsub) return;
  Fr30 x[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) x[q] = fr30_from(in[8 * (size_t)c + q]);
  const Fr30 one = mat[64];
#pragma unroll 1
  for (int r = 0; r < 8; r += 2) {
    Fr30 a0 = fr30_zero(), a1 = fr30_zero();
#pragma unroll
    for (int q = 0; q < 8; ++q) fr30_muladd_x2(mat[8 * r + q], x[q], a0, mat[8 * r + 8 + q], x[q], a1, a0, a1);
    const Fr30 z = fr30_zero();
    fr30_muladd_x2(one, a0, z, one, a1, z, a0, a1);  // sums of eight lazy products (< 8.1 p) -> below 1.02 p
    out[8 * (size_t)c + r] = fr30_canon(a0);
    out[8 * (size_t)c + r + 1] = fr30_canon(a1);
  }
}

// exit tables of the stride-2^sl subtree: xinv[i] = 1/xnn[2i], z0inv[i] = 1/Z_0(leaf 2i+1)
__global__ void __launch_bounds__(256)
k_exit_tables(const Fr* __restrict__ L0, int sl, uint32_t h, const Fr* __restrict__ xnn, const Fr* __restrict__ x0s,
              const Fr* __restrict__ ts, int kk, const Fr* __restrict__ c0p, Fr* __restrict__ xinv, Fr* __restrict__ z0inv) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h) return;
  xinv[i] = fr_inv(xnn[2 * i]);
  Fr leaf = L0[(size_t)(2 * i + 1) << sl];
  z0inv[i] = fr_inv(vanish_chain(leaf, x0s, ts, kk, *c0p));
}

// t0[c*h+i] = ev[c*sz+2i] * xinv[i]
__global__ void __launch_bounds__(256)
k_exit_pre(const Fr* __restrict__ ev, const Fr* __restrict__ xinv, Fr* __restrict__ t0, uint32_t h, uint32_t total) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total) return;
  uint32_t c = tid / h, i = tid - c * h;
  t0[tid] = fr_mul(xinv[i], ev[(size_t)c * 2 * h + 2 * i]);
}
// h1[c*h+i] = (ev[c*sz+2i+1] - g1[c*h+i]*xnn[2i+1]) * z0inv[i]
__global__ void __launch_bounds__(256)
k_exit_mid(const Fr* __restrict__ ev, const Fr* __restrict__ g1, const Fr* __restrict__ xnn, const Fr* __restrict__ z0inv,
           Fr* __restrict__ h1, uint32_t h, uint32_t total) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total) return;
  uint32_t c = tid / h, i = tid - c * h;
  Fr d = fr_sub(ev[(size_t)c * 2 * h + 2 * i + 1], fr_mul(xnn[2 * i + 1], g1[tid]));
  h1[tid] = fr_mul(z0inv[i], d);
}
// out[c*sz+2i] = h0*ctab[2i], out[c*sz+2i+1] = h1*ctab[2i+1]
__global__ void __launch_bounds__(256)
k_exit_mulc(const Fr* __restrict__ h0, const Fr* __restrict__ h1, const Fr* __restrict__ ctab, Fr* __restrict__ out,
            uint32_t h, uint32_t total) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total) return;
  uint32_t c = tid / h, i = tid - c * h;
  size_t o = (size_t)c * 2 * h + 2 * i;
  out[o] = fr_mul(ctab[2 * i], h0[tid]);
  out[o + 1] = fr_mul(ctab[2 * i + 1], h1[tid]);
}
// next[(2c)*h+i] = u0 ; next[(2c+1)*h+i] = (ev[c*sz+2i] - u0) * xinv[i]
__global__ void __launch_bounds__(256)
k_exit_post(const Fr* __restrict__ ev, const Fr* __restrict__ u0, const Fr* __restrict__ xinv, Fr* __restrict__ next,
            uint32_t h, uint32_t total) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total) return;
  uint32_t c = tid / h, i = tid - c * h;
  Fr u = u0[tid];
  next[(size_t)(2 * c) * h + i] = u;
  next[(size_t)(2 * c + 1) * h + i] = fr_mul(xinv[i], fr_sub(ev[(size_t)c * 2 * h + 2 * i], u));
}

// exit's folded tables of one stride level (ExtIo; all in the multiplier's constant form, indexed by the position i < h):
//   P  = win * xinv                      first extend of a redc reads the even entries:      x = P[i] * ev[2 (c h + i)]
//   R  = P * ctab[2i]                    ... or the previous redc's even half h0:            x = R[i] * h0[c h + i]
//   nA = -(wout * xnn[2i+1] * z0inv)     its last pass stores h1 = B * ev_odd + nA * x       (B = z0inv; B2 = z0inv * ctab[2i+1] on h1)
//   XI = xinv                            the level's last extend stores (u, XI * (ev_even - u))
// win / wout are the twists of the even -> odd extend of this level (MatSet to_even = 0).
__global__ void __launch_bounds__(256)
k_exit_fuse_tables(const Fr30* __restrict__ win, const Fr30* __restrict__ wout, const Fr* __restrict__ xinv, const Fr* __restrict__ z0inv,
                   const Fr* __restrict__ xnn, const Fr* __restrict__ ctab, Fr30* __restrict__ P, Fr30* __restrict__ R, Fr30* __restrict__ nA,
                   Fr30* __restrict__ B, Fr30* __restrict__ B2, Fr30* __restrict__ XI, uint32_t h) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h) return;
  const Fr30 z = fr30_zero();
  const Fr xi = xinv[i], zi = z0inv[i];
  // (w R') * (y R) / R' = w y R: the Montgomery form of the product
  const Fr p = fr30_canon(fr30_muladd(win[i], fr30_from(xi), z));
  const Fr a = fr30_canon(fr30_muladd(wout[i], fr30_from(xnn[2 * i + 1]), z));
  P[i] = fr30_const(p);
  R[i] = fr30_const(fr_mul(p, ctab[2 * i]));
  nA[i] = fr30_const(fr_neg(fr_mul(a, zi)));
  B[i] = fr30_const(zi);
  B2[i] = fr30_const(fr_mul(zi, ctab[2 * i + 1]));
  XI[i] = fr30_const(xi);
}

// the deepest exit level (h = 1: two evaluations per sub-problem, every extend the identity) in one pass: what k_exit_pre / _mid /
// _mulc / _pre / _mid / _post do with six launches and two copies.  out[2c] = u, out[2c + 1] = xinv (ev0 - u)
__global__ void __launch_bounds__(256)
k_exit_leaf(const Fr* __restrict__ ev, const Fr* __restrict__ xinv, const Fr* __restrict__ z0inv, const Fr* __restrict__ xnn,
            const Fr* __restrict__ ctab, Fr* __restrict__ out, uint32_t nsub) {
  uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nsub) return;
  const Fr xi = xinv[0], zi = z0inv[0], xo = xnn[1], ce = ctab[0], co = ctab[1];
  const Fr e0 = ev[2 * (size_t)c], e1 = ev[2 * (size_t)c + 1];
  const Fr g1 = fr_mul(xi, e0);
  const Fr h1 = fr_mul(zi, fr_sub(e1, fr_mul(xo, g1)));              // = h0
  const Fr g2 = fr_mul(xi, fr_mul(ce, h1));
  const Fr u = fr_mul(zi, fr_sub(fr_mul(co, h1), fr_mul(xo, g2)));
  out[2 * (size_t)c] = u;
  out[2 * (size_t)c + 1] = fr_mul(xi, fr_sub(e0, u));
}

// helpers for the z0z0 bootstrap
__global__ void __launch_bounds__(256) k_neg_from_mont_even(const Fr* __restrict__ xnn, Fr* __restrict__ out, uint32_t h) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < h) out[i] = fr_neg(fr_from_mont(xnn[2 * i]));
}
__global__ void __launch_bounds__(256) k_mul_canon(const Fr* __restrict__ a, const Fr* __restrict__ b, Fr* __restrict__ out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fr_mul(fr_to_mont(a[i]), b[i]);  // canonical product
}
// rho[j] = A[j] + (j >= h/2 ? 2*B[j-h/2] : 0), j < h ; rho[h..2h) = 0
__global__ void __launch_bounds__(256) k_rho(const Fr* __restrict__ A, const Fr* __restrict__ B, Fr* __restrict__ rho, uint32_t h) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * h) return;
  Fr r = fr_zero();
  if (j < h) {
    r = A[j];
    if (j >= h / 2) r = fr_add(r, fr_dbl(B[j - h / 2]));
  }
  rho[j] = r;
}
__global__ void __launch_bounds__(256) k_to_mont(const Fr* __restrict__ in, Fr* __restrict__ out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fr_to_mont(in[i]);
}
// h == 1: c[0] = c[1] = s0^2 (Montgomery)
__global__ void k_c_base(const Fr* __restrict__ L0, Fr* __restrict__ ctab) {
  Fr s = fr_sqr(L0[0]);
  ctab[0] = s;
  ctab[1] = s;
}
}  // namespace dvp

// ---- enter / exit on the stride-2^sl0 subtree (M = N >> sl0 leaves) ------------------------------------
// Every function from here to exit_core runs with c->mu held by the entry that called it (ecfft_internal.h); each table is looked up
// in the context and built at its first use.
static int get_xnn(dvp_ecfft* c, int sl, Fr** out, hipStream_t st) {
  auto it = c->xnn.find(sl);
  if (it != c->xnn.end()) {
    *out = it->second;
    return DVP_OK;
  }
  uint32_t sz = c->n_leaves >> sl;
  Fr* p;
  DVP_HIP(hipMalloc((void**)&p, (size_t)sz * sizeof(Fr)));
  DVP_LAUNCH(k_pow_table, dim3(cdiv(sz, TPB)), dim3(TPB), 0, st, c->layer(0), sl, sz, (uint64_t)(sz >> 1), p);
  DVP_HIP(hipGetLastError());
  c->xnn[sl] = p;
  *out = p;
  return DVP_OK;
}

static int ensure_scratch(dvp_ecfft* c) {
  if (!c->scratch) DVP_HIP(hipMalloc((void**)&c->scratch, (size_t)6 * c->n_leaves * sizeof(Fr)));
  return DVP_OK;
}
// device copies of the per-layer isogeny constants: the body, and the locked entry of prove.hip and setup.hip (host_api.h)
static int device_consts(dvp_ecfft* c) {
  if (!c->d_x0) {
    DVP_HIP(hipMalloc((void**)&c->d_x0, c->log_n * sizeof(Fr)));
    DVP_HIP(hipMalloc((void**)&c->d_t, c->log_n * sizeof(Fr)));
    DVP_HIP(hipMemcpy(c->d_x0, c->x0.data(), c->log_n * sizeof(Fr), hipMemcpyHostToDevice));
    DVP_HIP(hipMemcpy(c->d_t, c->t.data(), c->log_n * sizeof(Fr), hipMemcpyHostToDevice));
  }
  return DVP_OK;
}
int ecfft_device_consts(dvp_ecfft* c) {
  std::lock_guard<std::mutex> g(c->mu);
  return device_consts(c);
}

static int get_leaf8(dvp_ecfft* c, Leaf8* out, hipStream_t st) {
  if (c->leaf8.enter) {
    *out = c->leaf8;
    return DVP_OK;
  }
  if (c->log_n < 3) return DVP_EINVAL;
  Fr leaf[8];
  const int k8 = c->log_n - 3;
  DVP_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < 8; ++j) DVP_HIP(hipMemcpy(&leaf[j], c->layer(0) + ((size_t)j << k8), sizeof(Fr), hipMemcpyDeviceToHost));
  // Montgomery arithmetic on the host: V[j][e] = leaf_j^e, W = V^-1 by Gauss-Jordan (the leaves are distinct: V is invertible)
  Fr V[8][8], A[8][8], W[8][8];
  for (int j = 0; j < 8; ++j) {
    V[j][0] = fr_one_mont();
    for (int e = 1; e < 8; ++e) V[j][e] = fr_mul(V[j][e - 1], leaf[j]);
    for (int e = 0; e < 8; ++e) {
      A[j][e] = V[j][e];
      W[j][e] = j == e ? fr_one_mont() : fr_zero();
    }
  }
  for (int col = 0; col < 8; ++col) {
    int piv = col;
    while (piv < 8 && fr_is_zero(A[piv][col])) ++piv;
    if (piv == 8) return DVP_EINVAL;
    if (piv != col)
      for (int e = 0; e < 8; ++e) {
        Fr t = A[piv][e]; A[piv][e] = A[col][e]; A[col][e] = t;
        t = W[piv][e]; W[piv][e] = W[col][e]; W[col][e] = t;
      }
    const Fr inv = fr_inv(A[col][col]);
    for (int e = 0; e < 8; ++e) {
      A[col][e] = fr_mul(A[col][e], inv);
      W[col][e] = fr_mul(W[col][e], inv);
    }
    for (int r = 0; r < 8; ++r) {
      if (r == col || fr_is_zero(A[r][col])) continue;
      const Fr f = A[r][col];
      for (int e = 0; e < 8; ++e) {
        A[r][e] = fr_sub(A[r][e], fr_mul(f, A[col][e]));
        W[r][e] = fr_sub(W[r][e], fr_mul(f, W[col][e]));
      }
    }
  }
  Fr30 he[65], hx[65];
  for (int r = 0; r < 8; ++r)
    for (int q = 0; q < 8; ++q) {
      he[8 * r + q] = fr30_const(V[r][q]);
      hx[8 * r + q] = fr30_const(W[r][q]);
    }
  he[64] = hx[64] = fr30_const(fr_one_mont());
  Leaf8 t;
  DVP_HIP(hipMalloc((void**)&t.enter, sizeof(he)));
  DVP_HIP(hipMalloc((void**)&t.exit, sizeof(hx)));
  DVP_HIP(hipMemcpy(t.enter, he, sizeof(he), hipMemcpyHostToDevice));
  DVP_HIP(hipMemcpy(t.exit, hx, sizeof(hx), hipMemcpyHostToDevice));
  c->leaf8 = t;
  *out = t;
  return DVP_OK;
}

static int get_enter_tab(dvp_ecfft* c, int sl, EnterTab* out, hipStream_t st) {
  auto it = c->enter_tabs.find(sl);
  if (it != c->enter_tabs.end()) {
    *out = it->second;
    return DVP_OK;
  }
  const uint32_t h = (c->n_leaves >> sl) >> 1;
  Fr* xnn;
  DVP_TRY(get_xnn(c, sl, &xnn, st));
  MatSet* ms;
  DVP_TRY(build_matset(c, sl, 0, &ms, st));
  EnterTab tb;
  DVP_HIP(hipMalloc((void**)&tb.xe, (size_t)h * sizeof(Fr30)));
  DVP_HIP(hipMalloc((void**)&tb.t2, (size_t)h * sizeof(Fr30)));
  DVP_LAUNCH(k_enter_fuse_tables, dim3(cdiv(h, TPB)), dim3(TPB), 0, st, xnn, ms->wout, tb.xe, tb.t2, h);
  DVP_HIP(hipGetLastError());
  c->enter_tabs[sl] = tb;
  *out = tb;
  return DVP_OK;
}

// enter: bottom-up over recursion depth k (sub-problem size sz = N>>k on the stride-2^k subtree).
// All sub-problems of a depth share the subtree, so each depth is ONE batched extend
// (batch 2*nsub, vectors of sz/2) plus one combine kernel.
static int enter_core(dvp_ecfft* c, int sl0, const Fr* d_coeffs, Fr* d_out, hipStream_t st) {
  const uint32_t N = c->n_leaves, M = N >> sl0;
  DVP_TRY(ensure_scratch(c));
  Fr* odd = c->scratch + M;
  Fr* bufs[2] = {c->scratch, c->scratch + 2 * (size_t)M};
  const bool fold = tune().ecfft_fold != 0;
  const Fr* even = d_coeffs;  // read in place: the first level's extend and combine only read it
  int nb = 0;
  int k_first = c->log_n - 1;
  if (fold && M >= 8) {  // levels log_n - 1 .. log_n - 3 in one pass (k_leaf_matmul8)
    Leaf8 l8;
    DVP_TRY(get_leaf8(c, &l8, st));
    Fr* dst = (c->log_n - 3 == sl0) ? d_out : bufs[nb];
    DVP_LAUNCH(k_leaf_matmul8, dim3(cdiv(M / 8, TPB)), dim3(TPB), 0, st, d_coeffs, dst, l8.enter, M / 8);
    DVP_HIP(hipGetLastError());
    even = dst;
    nb ^= 1;
    k_first = c->log_n - 4;
  }
  for (int k = k_first; k >= sl0; --k) {
    uint32_t sz = N >> k, h = sz >> 1, nsub = 1u << (k - sl0);
    Fr* dst = (k == sl0) ? d_out : bufs[nb];
    if (fold && ext_io_ok(h, 3)) {
      // the extend reads `even`, works in `odd`, and its last launch recombines straight into dst
      EnterTab tb;
      DVP_TRY(get_enter_tab(c, k, &tb, st));
      ExtIoSpec io;
      io.sm = 3;
      io.out = dst;
      io.tb = tb.xe;
      io.tc = tb.t2;
      io.aux = even;
      io.lh = 31 - __builtin_clz(h);
      DVP_TRY(extend_io(c, k, 0, even, odd, 2 * nsub, st, &io));
    } else {
      if (h > 1) DVP_TRY(extend_io(c, k, 0, even, odd, 2 * nsub, st, nullptr));  // (h == 1: a constant is its own extension)
      Fr* xnn;
      DVP_TRY(get_xnn(c, k, &xnn, st));
      DVP_LAUNCH(k_enter_combine, dim3(cdiv(nsub * h, TPB)), dim3(TPB), 0, st, even, h > 1 ? odd : even, xnn, dst, h, nsub * h);
      DVP_HIP(hipGetLastError());
    }
    even = dst;
    nb ^= 1;
  }
  if (c->log_n == sl0) DVP_HIP(hipMemcpyAsync(d_out, d_coeffs, sizeof(Fr), hipMemcpyDeviceToDevice, st));
  return DVP_OK;
}

// exit: top-down.  At depth k every sub-problem (sz evaluations on the stride-2^k subtree) is split into
// the evaluations of its low and high coefficient halves on the even subtree:
//   u = <P mod X^h> = redc(redc(P) * <Z_0^2 mod X^h>),   redc(P) = <P Z_0^-1 mod X^h>  (Montgomery-style)
//   lo <- u|even,   hi <- (P|even - u|even) / X^h|even
// exit_levels runs the levels on tables that exist (exit_core, at the end, builds them first; the table builder itself calls
// exit_levels on the even subtree, whose levels it has already built: no recursion between the two).
static int exit_levels(dvp_ecfft* c, int sl0, const Fr* d_evals, Fr* d_out, hipStream_t st) {
  const uint32_t N = c->n_leaves, M = N >> sl0;
  if (M == 1) {
    DVP_HIP(hipMemcpyAsync(d_out, d_evals, sizeof(Fr), hipMemcpyDeviceToDevice, st));
    return DVP_OK;
  }
  DVP_TRY(ensure_scratch(c));
  Fr* S = c->scratch;
  Fr* pp[2] = {S + 4 * (size_t)M, S};  // M each: the levels' outputs, in turn (the last level writes d_out itself)
  Fr* t0 = S + (size_t)M;             // M/2  (also g1)
  Fr* h1 = S + (size_t)M + M / 2;     // M/2
  Fr* h0 = S + 2 * (size_t)M;         // M/2
  Fr* r1 = S + 3 * (size_t)M;         // M
  const Fr* cur = d_evals;  // the first level reads the caller's vector in place
  int w = 0;
  const bool leaf8 = tune().ecfft_fold != 0 && M >= 8;  // the levels below sz = 8 in one pass (k_leaf_matmul8)
  const int k_end = leaf8 ? c->log_n - 3 : c->log_n;
  for (int k = sl0; k < k_end; ++k) {
    uint32_t sz = N >> k, h = sz >> 1, nsub = 1u << (k - sl0), total = nsub * h;
    Fr* nxt = k == c->log_n - 1 ? d_out : pp[w];
    const auto found = c->exit_tabs.find(k);
    if (found == c->exit_tabs.end()) return DVP_EINVAL;
    const ExitTab tb = found->second;
    Fr* xnn;
    DVP_TRY(get_xnn(c, k, &xnn, st));
    dim3 grid(cdiv(total, TPB)), blk(TPB);
    auto redc = [&](const Fr* ev) -> int {  // leaves h0 (even part) and h1 (odd part)
      DVP_LAUNCH(k_exit_pre, grid, blk, 0, st, ev, tb.xinv, t0, h, total);
      DVP_TRY(extend_io(c, k, 0, t0, t0, nsub, st, nullptr));
      DVP_LAUNCH(k_exit_mid, grid, blk, 0, st, ev, t0, xnn, tb.z0inv, h1, h, total);
      DVP_TRY(extend_io(c, k, 1, h1, h0, nsub, st, nullptr));  // (h == 1: a copy)
      return DVP_OK;
    };
    if (tb.fused && tune().ecfft_fold != 0) {
      // four extends and nothing else (round 6): every pointwise stage rides in the first / last pass of an extend (ExtIo), the
      // copy h1 -> h0 is the out-of-place first pass, and r1 = (ctab_even h0 | ctab_odd h1) is never written
      const Fr30 *P = tb.fused, *R = P + h, *nA = P + 2 * (size_t)h, *B = P + 3 * (size_t)h, *B2 = P + 4 * (size_t)h, *XI = P + 5 * (size_t)h;
      Fr* h1b = r1;  // the second redc's odd half (r1 itself is not needed any more)
      const int lh = 31 - __builtin_clz(h);
      ExtIoSpec a1;  // redc 1, even -> odd: t = xinv * ev_even in, h1 = z0inv * (ev_odd - xnn_odd * g1) out
      a1.sm = 1; a1.pre = P; a1.lshift = 1; a1.post = nA; a1.out = h1; a1.tb = B; a1.aux = cur; a1.ashift = 1; a1.aoff = 1;
      DVP_TRY(extend_io(c, k, 0, cur, t0, nsub, st, &a1));
      DVP_TRY(extend_io(c, k, 1, h1, h0, nsub, st, nullptr));  // odd -> even: h0
      ExtIoSpec a2;  // redc 2 on r1 = (ctab_even h0 | ctab_odd h1), never materialised
      a2.sm = 1; a2.pre = R; a2.post = nA; a2.out = h1b; a2.tb = B2; a2.aux = h1;
      DVP_TRY(extend_io(c, k, 0, h0, t0, nsub, st, &a2));
      ExtIoSpec b2;  // odd -> even: u; next level's (lo, hi) = (u, xinv * (ev_even - u))
      b2.sm = 2; b2.out = nxt; b2.tb = XI; b2.aux = cur; b2.lh = lh;
      DVP_TRY(extend_io(c, k, 1, h1b, h0, nsub, st, &b2));
    } else if (h == 1 && tune().ecfft_fold != 0) {
      DVP_LAUNCH(k_exit_leaf, grid, blk, 0, st, cur, tb.xinv, tb.z0inv, xnn, tb.ctab, nxt, nsub);
    } else {
      DVP_TRY(redc(cur));
      DVP_LAUNCH(k_exit_mulc, grid, blk, 0, st, h0, h1, tb.ctab, r1, h, total);
      DVP_TRY(redc(r1));
      DVP_LAUNCH(k_exit_post, grid, blk, 0, st, cur, h0, tb.xinv, nxt, h, total);
    }
    DVP_HIP(hipGetLastError());
    cur = nxt;
    w ^= 1;
  }
  if (leaf8) {
    Leaf8 l8;
    DVP_TRY(get_leaf8(c, &l8, st));
    DVP_LAUNCH(k_leaf_matmul8, dim3(cdiv(M / 8, TPB)), dim3(TPB), 0, st, cur, d_out, l8.exit, M / 8);
    DVP_HIP(hipGetLastError());
  }
  return DVP_OK;
}

// Build (once) the exit tables of every stride level >= sl, deepest first: level sl needs enter and exit on the stride-2^(sl + 1)
// subtree, whose levels are in the context by then.
static int ensure_exit_tables(dvp_ecfft* c, int sl_min, hipStream_t st) {
  const uint32_t N = c->n_leaves;
  DVP_TRY(device_consts(c));
  for (int sl = c->log_n - 1; sl >= sl_min; --sl) {
    if (c->exit_tabs.count(sl)) continue;
    uint32_t sz = N >> sl, h = sz >> 1;
    int kk = 31 - __builtin_clz(h);  // h = 2^kk even leaves -> kk isogenies collapse them
    ExitTab tb;
    DVP_HIP(hipMalloc((void**)&tb.xinv, (size_t)h * sizeof(Fr)));
    DVP_HIP(hipMalloc((void**)&tb.z0inv, (size_t)h * sizeof(Fr)));
    DVP_HIP(hipMalloc((void**)&tb.ctab, (size_t)sz * sizeof(Fr)));
    Fr* xnn;
    DVP_TRY(get_xnn(c, sl, &xnn, st));
    // the even leaves of the stride-2^sl tree all map to layer-kk leaf 0 of the strided tree = layers[kk][0]
    DVP_LAUNCH(k_exit_tables, dim3(cdiv(h, TPB)), dim3(TPB), 0, st, c->layer(0), sl, h, xnn, c->d_x0, c->d_t, kk,
                       c->layer(kk), tb.xinv, tb.z0inv);
    if (h == 1) {
      DVP_LAUNCH(k_c_base, dim3(1), dim3(1), 0, st, c->layer(0), tb.ctab);
    } else {
      // (1) z = Z_0 - X^h in coefficient form: exit on the even subtree of the evaluations -leaf^h
      DevBuf zlow, lo, hi, A, B, rho;
      DVP_TRY(zlow.alloc((size_t)h * sizeof(Fr)));
      DVP_TRY(lo.alloc((size_t)h * sizeof(Fr)));
      DVP_TRY(hi.alloc((size_t)h * sizeof(Fr)));
      DVP_TRY(A.alloc((size_t)h * sizeof(Fr)));
      DVP_TRY(B.alloc((size_t)h * sizeof(Fr)));
      DVP_TRY(rho.alloc((size_t)sz * sizeof(Fr)));
      DVP_LAUNCH(k_neg_from_mont_even, dim3(cdiv(h, TPB)), dim3(TPB), 0, st, xnn, lo.as<Fr>(), h);
      DVP_TRY(exit_levels(c, sl + 1, lo.as<Fr>(), zlow.as<Fr>(), st));
      // (2) z = z_lo + X^(h/2) z_hi;  Z_0^2 mod X^h = z_lo^2 + 2 X^(h/2) (z_lo z_hi mod X^(h/2))
      DVP_HIP(hipMemsetAsync(lo.p, 0, (size_t)h * sizeof(Fr), st));
      DVP_HIP(hipMemsetAsync(hi.p, 0, (size_t)h * sizeof(Fr), st));
      DVP_HIP(hipMemcpyAsync(lo.p, zlow.p, (size_t)(h / 2) * sizeof(Fr), hipMemcpyDeviceToDevice, st));
      DVP_HIP(hipMemcpyAsync(hi.p, zlow.as<Fr>() + h / 2, (size_t)(h / 2) * sizeof(Fr), hipMemcpyDeviceToDevice, st));
      DVP_TRY(enter_core(c, sl + 1, lo.as<Fr>(), A.as<Fr>(), st));  // <z_lo> on the even subtree
      DVP_TRY(enter_core(c, sl + 1, hi.as<Fr>(), B.as<Fr>(), st));  // <z_hi>
      DVP_LAUNCH(k_mul_canon, dim3(cdiv(h, TPB)), dim3(TPB), 0, st, A.as<Fr>(), B.as<Fr>(), hi.as<Fr>(), h);  // <z_lo z_hi>
      DVP_LAUNCH(k_mul_canon, dim3(cdiv(h, TPB)), dim3(TPB), 0, st, A.as<Fr>(), A.as<Fr>(), lo.as<Fr>(), h);  // <z_lo^2>
      DVP_TRY(exit_levels(c, sl + 1, lo.as<Fr>(), A.as<Fr>(), st));
      DVP_TRY(exit_levels(c, sl + 1, hi.as<Fr>(), B.as<Fr>(), st));
      DVP_LAUNCH(k_rho, dim3(cdiv(sz, TPB)), dim3(TPB), 0, st, A.as<Fr>(), B.as<Fr>(), rho.as<Fr>(), h);
      // (3) evaluate on the whole subtree, keep in Montgomery form
      DevBuf ev;
      DVP_TRY(ev.alloc((size_t)sz * sizeof(Fr)));
      DVP_TRY(enter_core(c, sl, rho.as<Fr>(), ev.as<Fr>(), st));
      DVP_LAUNCH(k_to_mont, dim3(cdiv(sz, TPB)), dim3(TPB), 0, st, ev.as<Fr>(), tb.ctab, sz);
      DVP_HIP(hipGetLastError());
      DVP_HIP(hipStreamSynchronize(st));  // DevBufs go out of scope
    }
    DVP_HIP(hipGetLastError());
    if (ext_io_ok(h, 1)) {
      MatSet* ms;
      DVP_TRY(build_matset(c, sl, 0, &ms, st));
      DVP_HIP(hipMalloc((void**)&tb.fused, (size_t)6 * h * sizeof(Fr30)));
      Fr30* f = tb.fused;
      DVP_LAUNCH(k_exit_fuse_tables, dim3(cdiv(h, TPB)), dim3(TPB), 0, st, ms->win, ms->wout, tb.xinv, tb.z0inv, xnn, tb.ctab, f, f + h, f + 2 * (size_t)h,
                         f + 3 * (size_t)h, f + 4 * (size_t)h, f + 5 * (size_t)h, h);
      DVP_HIP(hipGetLastError());
    }
    c->exit_tabs[sl] = tb;
  }
  return DVP_OK;
}
static int exit_core(dvp_ecfft* c, int sl0, const Fr* d_evals, Fr* d_out, hipStream_t st) {
  DVP_TRY(ensure_exit_tables(c, sl0, st));
  return exit_levels(c, sl0, d_evals, d_out, st);
}
