// ECFFT, stage 2: the constants of an extend on one (stride, direction) -- twisted-butterfly pairs and the twists (build_matset);
// the reference's true 2x2 matrices for the read-outs of ecfft_debug.cuh (k_build_mats).  Part of ecfft.hip's translation unit.
#pragma once
#include "ecfft_domain.cuh"

namespace dvp {

// 2x2 matrices of one layer of one (strided) tree.  Ld = layer-d leaves of the full tree; the
// strided tree's leaf j is Ld[j << sl] and it has 2*nd leaves.  Pair i < nd/2:
//   decompose  (from leaves 2i+src, 2i+src+nd):  inverse of [[v0, s0 v0],[v1, s1 v1]]
//   recombine  (from leaves 2i+dst, 2i+dst+nd):            [[v0, s0 v0],[v1, s1 v1]]
// with v = (s - x0)^(nd/2 - 1).
// Matrix entries are consumed only by fr_dot2, so they are stored pre-sliced into 29-bit limbs (same 32 bytes).
__device__ __forceinline__ Fr29 mat_store(const Fr& a) { return fr29_from(a); }

__global__ void __launch_bounds__(256) k_build_mats(const Fr* __restrict__ Ld, int sl, uint32_t nd, Fr x0, int src, int dst,
                             Fr29* __restrict__ dec, Fr29* __restrict__ rec) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t h = nd >> 1;
  if (i >= h) return;
  uint64_t e = (uint64_t)h - 1;
  {
    Fr s0 = Ld[(size_t)(2 * i + src) << sl];
    Fr s1 = Ld[(size_t)(2 * i + src + nd) << sl];
    Fr v0 = fr_pow_u64(fr_sub(s0, x0), e);
    Fr v1 = fr_pow_u64(fr_sub(s1, x0), e);
    Fr det = fr_mul(fr_mul(v0, v1), fr_sub(s1, s0));
    Fr inv = fr_inv(det);
    Fr iv0 = fr_mul(inv, v0), iv1 = fr_mul(inv, v1);
    dec[4 * (size_t)i + 0] = mat_store(fr_mul(s1, iv1));
    dec[4 * (size_t)i + 1] = mat_store(fr_neg(fr_mul(s0, iv0)));
    dec[4 * (size_t)i + 2] = mat_store(fr_neg(iv1));
    dec[4 * (size_t)i + 3] = mat_store(iv0);
  }
  {
    Fr s0 = Ld[(size_t)(2 * i + dst) << sl];
    Fr s1 = Ld[(size_t)(2 * i + dst + nd) << sl];
    Fr v0 = fr_pow_u64(fr_sub(s0, x0), e);
    Fr v1 = fr_pow_u64(fr_sub(s1, x0), e);
    rec[4 * (size_t)i + 0] = mat_store(v0);
    rec[4 * (size_t)i + 1] = mat_store(fr_mul(s0, v0));
    rec[4 * (size_t)i + 2] = mat_store(v1);
    rec[4 * (size_t)i + 3] = mat_store(fr_mul(s1, v1));
  }
}

// ---- TWISTED butterflies (round 4) ---------------------------------------------------------------------------------------
// The matrices above are  recombine = diag(v0, v1) [[1, s0], [1, s1]]  with v = q(s)^(h - 1) (q = the isogeny's denominator) and
// decompose = its inverse.  Carry every value divided by the twist  W_d(s) = v_d(s) W_{d+1}(psi_d(s)),  W_bottom = 1  -- the
// product of the v factors along the point's orbit down the isogeny chain.  Both halves of a decomposition live at the same
// image point t, so they share ONE twist W_{d+1}(t), and in twisted values Q = P / W a butterfly is just
//      recombine   Q(s0) = Q0 + s0 Q1,   Q(s1) = Q0 + s1 Q1
//      decompose   Q1 = (Q(s0) - Q(s1)) / (s0 - s1),   Q0 = Q(s0) - s0 Q1
// TWO field products per pair (each with its addition folded into the Montgomery accumulation, fr_muladd29: 2 x 96 limb
// products) instead of the FOUR of a general 2x2 matrix (2 x fr_dot2: 2 x 160), and 64 bytes of constants per pair instead of
// 128.  The twist depends only on the point, i.e. on the position in the top-level vector: an extend multiplies its input by
// 1 / W^src once (fused into its first pass) and its output by W^dst once (fused into its last pass); at the bottom both twists
// are 1, which is where the source and destination halves meet.  Values are the same field elements as before: every parity
// test (oracle extend / enter / exit element for element, FFTR sections, proofs) is unchanged.
// Constants per pair (Montgomery form, pre-sliced): decompose (1 / (s0 - s1), -s0), recombine (s0, s1); layer d at offset
// 2 (n - (n >> d)).  The true 2x2 matrices are still built on demand for dvp_debug_ecfft_matrices / FFTR tree files (k_build_mats).
__global__ void __launch_bounds__(256) k_build_twiddles(const Fr* __restrict__ Ld, int sl, uint32_t nd, int src, int dst, Fr30* __restrict__ dec,
                                                        Fr30* __restrict__ rec) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t h = nd >> 1;
  if (i >= h) return;
  {
    Fr s0 = Ld[(size_t)(2 * i + src) << sl];
    Fr s1 = Ld[(size_t)(2 * i + src + nd) << sl];
    dec[2 * (size_t)i + 0] = fr30_const(fr_inv(fr_sub(s0, s1)));
    dec[2 * (size_t)i + 1] = fr30_const(fr_neg(s0));
  }
  rec[2 * (size_t)i + 0] = fr30_const(Ld[(size_t)(2 * i + dst) << sl]);
  rec[2 * (size_t)i + 1] = fr30_const(Ld[(size_t)(2 * i + dst + nd) << sl]);
}
// W_d[j] = v_d(point of position j in a block of nd values) * W_{d+1}[j mod (nd / 2)], bottom up; positions j < nd/2 sit at the
// first point of pair j, the others at the second point of pair j - nd/2 (that is where the in-place butterflies leave them)
__global__ void __launch_bounds__(256) k_twist_layer(const Fr* __restrict__ Ld, int sl, uint32_t nd, Fr x0, int parity, const Fr* __restrict__ w_next,
                                                     Fr* __restrict__ w_cur) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nd) return;
  const uint32_t h = nd >> 1, i = j & (h - 1);
  const Fr s = Ld[(size_t)(2 * i + parity + (j >= h ? nd : 0)) << sl];
  Fr v = fr_pow_u64(fr_sub(s, x0), (uint64_t)h - 1);
  if (w_next) v = fr_mul(v, w_next[i]);
  w_cur[j] = v;
}
__global__ void __launch_bounds__(256) k_twist_finish(const Fr* __restrict__ w_src, const Fr* __restrict__ w_dst, uint32_t n, Fr30* __restrict__ win,
                                                      Fr30* __restrict__ wout) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  win[j] = fr30_const(fr_inv(w_src[j]));
  wout[j] = fr30_const(w_dst[j]);
}

}  // namespace dvp

// the constants of the extends on the stride-2^sl subtree in one direction, built at the first one (the caller holds c->mu)
static int build_matset(dvp_ecfft* c, int sl, int to_even, MatSet** out, hipStream_t st) {
  int key = sl * 2 + to_even;
  auto it = c->mats.find(key);
  if (it != c->mats.end()) {
    *out = &it->second;
    return DVP_OK;
  }
  uint32_t n = (c->n_leaves >> sl) >> 1;  // evaluations moved by extend on this subtree
  MatSet ms;
  if (n > 1) {
    size_t bytes = (size_t)(n - 1) * 2 * sizeof(Fr30);
    DVP_HIP(hipMalloc((void**)&ms.dec, bytes));
    DVP_HIP(hipMalloc((void**)&ms.rec, bytes));
    DVP_HIP(hipMalloc((void**)&ms.win, (size_t)n * sizeof(Fr30)));
    DVP_HIP(hipMalloc((void**)&ms.wout, (size_t)n * sizeof(Fr30)));
    int src = to_even ? 1 : 0, dst = to_even ? 0 : 1;
    int ln = 31 - __builtin_clz(n);
    for (int d = 0; d < ln; ++d) {
      uint32_t nd = n >> d;
      size_t off = 2 * (size_t)(n - nd);
      DVP_LAUNCH(k_build_twiddles, dim3(cdiv(nd >> 1, TPB)), dim3(TPB), 0, st, c->layer(d), sl, nd, src, dst, ms.dec + off, ms.rec + off);
    }
    // the twists, bottom up: W_d from W_{d+1} (ping-pong), once per parity
    DevBuf wa, wb, ws, wd;
    DVP_TRY(wa.alloc((size_t)n * sizeof(Fr)));
    DVP_TRY(wb.alloc((size_t)n * sizeof(Fr)));
    DVP_TRY(ws.alloc((size_t)n * sizeof(Fr)));
    DVP_TRY(wd.alloc((size_t)n * sizeof(Fr)));
    for (int par = 0; par < 2; ++par) {
      const int parity = par == 0 ? src : dst;
      Fr* cur = wa.as<Fr>();
      Fr* nxt = wb.as<Fr>();
      const Fr* prev = nullptr;
      for (int d = ln - 1; d >= 0; --d) {
        uint32_t nd = n >> d;
        Fr* outp = d == 0 ? (par == 0 ? ws.as<Fr>() : wd.as<Fr>()) : cur;
        DVP_LAUNCH(k_twist_layer, dim3(cdiv(nd, TPB)), dim3(TPB), 0, st, c->layer(d), sl, nd, c->x0[d], parity, prev, outp);
        prev = outp;
        Fr* t = cur; cur = nxt; nxt = t;
      }
    }
    DVP_LAUNCH(k_twist_finish, dim3(cdiv(n, TPB)), dim3(TPB), 0, st, ws.as<Fr>(), wd.as<Fr>(), n, ms.win, ms.wout);
    DVP_HIP(hipGetLastError());
    DVP_HIP(hipStreamSynchronize(st));  // the scratch buffers go out of scope
  }
  c->mats[key] = ms;
  *out = &c->mats[key];
  return DVP_OK;
}
