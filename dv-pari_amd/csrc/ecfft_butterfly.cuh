// ECFFT, stage 3: the butterflies on lazy 30-bit-limb values and the register passes of one, two and three layers over the top of
// long vectors (k_butterfly, k_butterfly4, k_butterfly8).  Part of ecfft.hip's translation unit.
#pragma once
#include "fr.cuh"

namespace dvp {

// ---- the butterflies on lazy 30-bit-limb values (fr.cuh: Fr30) ---------------------------------------------------------------
// Between the passes of an extend the data buffer holds Fr30 values (same 32 bytes as an Fr): the pass that carries the input twist
// (`pre`, always the first) slices its canonical input, the pass that carries the output twist (`post`, always the last) reduces and
// re-slices; everything in between is multiply-accumulate only.  Bounds (in units of p, fr.cuh): the input twist leaves < 1.01; a
// decompose step gives Q1 < 1.4 and Q0 < bound(e0) + 1.01; a recombine step bound(Q0) + 1 + bound(Q1)/512: at most +1.13 per layer,
// < 64 after the 2 x 27 layers of the largest tree -- the lent 128 p of fr30_sub_lazy always covers its subtrahend.
struct Tw {
  Fr30 a, b;
};
__device__ __forceinline__ Tw tw_load(const Fr30* __restrict__ t, uint32_t i) {
  Tw r;
  r.a = t[2 * (size_t)i];
  r.b = t[2 * (size_t)i + 1];
  return r;
}
__device__ __forceinline__ Fr30 ld30(const Fr* p) {  // a value a previous pass stored in Fr30 form
  const Fr v = *p;
  Fr30 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = v.v[i];
  return r;
}
__device__ __forceinline__ void st30(Fr* p, const Fr30& a) {
  Fr v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v.v[i] = a.l[i];
  *p = v;
}
// two independent decompose steps: (e0, e1) = (Q(s0), Q(s1)) -> (Q0, Q1); t = (1 / (s0 - s1), -s0)
__device__ __forceinline__ void bf_dec2(Fr30& a0, Fr30& a1, const Tw& ta, Fr30& b0, Fr30& b1, const Tw& tb) {
  const Fr30 z = fr30_zero();
  Fr30 qa, qb;
  fr30_muladd_x2(ta.a, fr30_sub_lazy(a0, a1), z, tb.a, fr30_sub_lazy(b0, b1), z, qa, qb);
  fr30_muladd_x2(ta.b, qa, a0, tb.b, qb, b0, a0, b0);
  a1 = qa;
  b1 = qb;
}
__device__ __forceinline__ void bf_dec(Fr30& e0, Fr30& e1, const Tw& t) {
  const Fr30 q1 = fr30_muladd(t.a, fr30_sub_lazy(e0, e1), fr30_zero());
  e0 = fr30_muladd(t.b, q1, e0);
  e1 = q1;
}
// (e0, e1) = (Q0, Q1) -> (Q(s0), Q(s1)); t = (s0, s1): the two products of one step are independent
__device__ __forceinline__ void bf_rec(Fr30& e0, Fr30& e1, const Tw& t) { fr30_muladd_x2(t.a, e1, e0, t.b, e1, e0, e0, e1); }
// the twists of the first / last pass, two values at a time
__device__ __forceinline__ void tw_in2(const Fr30* __restrict__ w, uint32_t p0, uint32_t p1, const Fr& x0, const Fr& x1, Fr30& r0, Fr30& r1) {
  const Fr30 z = fr30_zero();
  fr30_muladd_x2(w[p0], fr30_from(x0), z, w[p1], fr30_from(x1), z, r0, r1);
}
__device__ __forceinline__ void tw_out2(const Fr30* __restrict__ w, uint32_t p0, uint32_t p1, const Fr30& x0, const Fr30& x1, Fr& r0, Fr& r1) {
  const Fr30 z = fr30_zero();
  Fr30 y0, y1;
  fr30_muladd_x2(w[p0], x0, z, w[p1], x1, z, y0, y1);
  r0 = fr30_canon(y0);
  r1 = fr30_canon(y1);
}

// One butterfly pass over `batch` vectors of n values.  Blocks of size 2h; pair (i, i+h) inside each block uses constants i of
// this layer.  One thread = one pair for all batch vectors, so the constants are read once per pair and reused `batch` times.
// pre / post (nullptr = none): the twists of the first / last pass of an extend, indexed by the position in the vector.
template <int BATCH, bool DEC>
__global__ void __launch_bounds__(256) k_butterfly(const Fr* src /* == data, or the untouched input of the first pass */, Fr* data,
                                                   const Fr30* __restrict__ tws, int lh, uint32_t n, const Fr30* __restrict__ pre,
                                                   const Fr30* __restrict__ post, uint32_t nv /* values per vector (twist index range) */) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (n >> 1)) return;
  uint32_t h = 1u << lh;
  uint32_t i = tid & (h - 1);
  uint32_t i0 = ((tid >> lh) << (lh + 1)) | i;
  uint32_t i1 = i0 + h;
  const Tw t = tw_load(tws, i);
  const uint32_t p0 = i0 & (nv - 1), p1 = i1 & (nv - 1);
#pragma unroll
  for (int b = 0; b < BATCH; ++b) {
    Fr* v = data + (size_t)b * n;
    const Fr* u = src + (size_t)b * n;
    Fr30 e0, e1;
    if (pre) tw_in2(pre, p0, p1, u[i0], u[i1], e0, e1); else { e0 = ld30(u + i0); e1 = ld30(u + i1); }
    if (DEC) bf_dec(e0, e1, t); else bf_rec(e0, e1, t);
    if (post) {
      Fr o0, o1;
      tw_out2(post, p0, p1, e0, e1, o0, o1);
      v[i0] = o0;
      v[i1] = o1;
    } else {
      st30(v + i0, e0);
      st30(v + i1, e1);
    }
  }
}

// TWO butterfly layers in one pass (radix 4): layer d (pairs h1 = 2^lh apart) and layer d + 1 (pairs h2 = h1 / 2 apart) only mix
// the four values {j, j + h2, j + h1, j + h1 + h2} of a block of 4 h2, so one thread loads them once, applies both layers in
// registers and stores them once: half the HBM round trips of the data.  Constants: two pairs of layer d (j, j + h2) and one of
// layer d + 1 (j, shared by both of its pairs).  DEC = decompose order (wide layer first); recombine runs the narrow layer first.
// BATCH vectors: lane = (quad of values, vector) with the vector index fastest, so the BATCH lanes that need the same constants
// sit in the same wave and their loads are one request.
// MAP: where the constants of half-block position i sit in a layer's table -- i itself for data held in vector order (TwId); a tile
// of a long vector (k_extend_top) maps its rows and columns back to vector positions (TwTile)
struct TwId {
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return i; }
};
template <bool DEC, class MAP = TwId>
__device__ __forceinline__ void radix4(Fr30& x0, Fr30& x1, Fr30& x2, Fr30& x3, const Fr30* __restrict__ tw_wide, const Fr30* __restrict__ tw_narrow,
                                       uint32_t j, uint32_t h2, MAP f = MAP()) {
  if (DEC) {
    bf_dec2(x0, x2, tw_load(tw_wide, f(j)), x1, x3, tw_load(tw_wide, f(j + h2)));
    const Tw c = tw_load(tw_narrow, f(j));
    bf_dec2(x0, x1, c, x2, x3, c);
  } else {
    {
      const Tw c = tw_load(tw_narrow, f(j));
      bf_rec(x0, x1, c);
      bf_rec(x2, x3, c);
    }
    bf_rec(x0, x2, tw_load(tw_wide, f(j)));
    bf_rec(x1, x3, tw_load(tw_wide, f(j + h2)));
  }
}
template <int BATCH, bool DEC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_butterfly4(const Fr* src /* == data, or the untouched input of the first pass */, Fr* data,
                                                    const Fr30* __restrict__ tw_wide, const Fr30* __restrict__ tw_narrow, int lh2, uint32_t n,
                                                    const Fr30* __restrict__ pre, const Fr30* __restrict__ post, uint32_t nv) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t tid = gid / BATCH, bv = gid - tid * BATCH;
  if (tid >= (n >> 2)) return;
  const uint32_t h2 = 1u << lh2, h1 = h2 << 1;
  const uint32_t j = tid & (h2 - 1);
  const uint32_t i0 = ((tid >> lh2) << (lh2 + 2)) | j;
  Fr* v = data + (size_t)bv * n + i0;
  const Fr* u = src + (size_t)bv * n + i0;
  const uint32_t p0 = i0 & (nv - 1);
  Fr30 x0, x1, x2, x3;
  if (pre) {
    tw_in2(pre, p0, p0 + h2, u[0], u[h2], x0, x1);
    tw_in2(pre, p0 + h1, p0 + h1 + h2, u[h1], u[h1 + h2], x2, x3);
  } else {
    x0 = ld30(u); x1 = ld30(u + h2); x2 = ld30(u + h1); x3 = ld30(u + h1 + h2);
  }
  radix4<DEC>(x0, x1, x2, x3, tw_wide, tw_narrow, j, h2);
  if (post) {
    Fr o0, o1, o2, o3;
    tw_out2(post, p0, p0 + h2, x0, x1, o0, o1);
    tw_out2(post, p0 + h1, p0 + h1 + h2, x2, x3, o2, o3);
    v[0] = o0; v[h2] = o1; v[h1] = o2; v[h1 + h2] = o3;
  } else {
    st30(v, x0); st30(v + h2, x1); st30(v + h1, x2); st30(v + h1 + h2, x3);
  }
}

// THREE layers in one pass (radix 8) for the top of long vectors: with the lazy multiplier a two-layer pass is HBM-bound (192 MB of
// data + up to 48 MB of constants in ~52 us at m = 2^20, batch 3), so a third layer per round trip is nearly free.  A thread owns the
// eight values i0 + {0, h3, h2, h2 + h3, h1, h1 + h3, h1 + h2, h1 + h2 + h3} (h1 = 2 h2 = 4 h3 = the widest pair distance); constants:
// four pairs of layer d (j, j + h3, j + h2, j + h2 + h3), two of layer d + 1 (j, j + h3), one of layer d + 2 (j).
#ifndef DVP_BF8_WAVES
#define DVP_BF8_WAVES 3
#endif
template <int BATCH, bool DEC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DVP_BF8_WAVES, DVP_BF8_WAVES))) k_butterfly8(const Fr* src, Fr* data, const Fr30* __restrict__ tw0, const Fr30* __restrict__ tw1,
                                                    const Fr30* __restrict__ tw2, int lh3, uint32_t n, const Fr30* __restrict__ pre,
                                                    const Fr30* __restrict__ post, uint32_t nv) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t tid = gid / BATCH, bv = gid - tid * BATCH;
  if (tid >= (n >> 3)) return;
  const uint32_t h3 = 1u << lh3, h2 = h3 << 1, h1 = h3 << 2;
  const uint32_t j = tid & (h3 - 1);
  const uint32_t i0 = ((tid >> lh3) << (lh3 + 3)) | j;
  Fr* v = data + (size_t)bv * n + i0;
  const Fr* u = src + (size_t)bv * n + i0;
  const uint32_t p0 = i0 & (nv - 1);
  Fr30 x[8];
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    const uint32_t o0 = (k & 4 ? h1 : 0) + (k & 2 ? h2 : 0), o1 = o0 + h3;
    if (pre) tw_in2(pre, p0 + o0, p0 + o1, u[o0], u[o1], x[k], x[k + 1]);
    else { x[k] = ld30(u + o0); x[k + 1] = ld30(u + o1); }
  }
  if (DEC) {
    bf_dec2(x[0], x[4], tw_load(tw0, j), x[1], x[5], tw_load(tw0, j + h3));
    bf_dec2(x[2], x[6], tw_load(tw0, j + h2), x[3], x[7], tw_load(tw0, j + h2 + h3));
    {
      const Tw a = tw_load(tw1, j), b = tw_load(tw1, j + h3);
      bf_dec2(x[0], x[2], a, x[1], x[3], b);
      bf_dec2(x[4], x[6], a, x[5], x[7], b);
    }
    const Tw c = tw_load(tw2, j);
    bf_dec2(x[0], x[1], c, x[2], x[3], c);
    bf_dec2(x[4], x[5], c, x[6], x[7], c);
  } else {
    {
      const Tw c = tw_load(tw2, j);
      bf_rec(x[0], x[1], c); bf_rec(x[2], x[3], c); bf_rec(x[4], x[5], c); bf_rec(x[6], x[7], c);
    }
    {
      const Tw a = tw_load(tw1, j), b = tw_load(tw1, j + h3);
      bf_rec(x[0], x[2], a); bf_rec(x[1], x[3], b); bf_rec(x[4], x[6], a); bf_rec(x[5], x[7], b);
    }
    bf_rec(x[0], x[4], tw_load(tw0, j));
    bf_rec(x[1], x[5], tw_load(tw0, j + h3));
    bf_rec(x[2], x[6], tw_load(tw0, j + h2));
    bf_rec(x[3], x[7], tw_load(tw0, j + h2 + h3));
  }
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    const uint32_t o0 = (k & 4 ? h1 : 0) + (k & 2 ? h2 : 0), o1 = o0 + h3;
    if (post) {
      Fr r0, r1;
      tw_out2(post, p0 + o0, p0 + o1, x[k], x[k + 1], r0, r1);
      v[o0] = r0;
      v[o1] = r1;
    } else {
      st30(v + o0, x[k]);
      st30(v + o1, x[k + 1]);
    }
  }
}

}  // namespace dvp
