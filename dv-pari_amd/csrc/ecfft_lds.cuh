// ECFFT, stage 4: the LDS kernels of an extend -- k_extend_fused (the innermost layers of a 2048-value block) and k_extend_top (up to
// nine layers above it on a tile) -- and ExtIo, what the first launch reads and the last one writes.  Part of ecfft.hip's translation unit.
#pragma once
#include "ecfft_butterfly.cuh"

namespace dvp {

// ---- what the first launch of an extend reads and the last one writes (round 6) -----------------------------------------------
// SM = 0 is the extend proper: the input twist on the way in (x = pre[p] * src[g]), the output twist on the way out.  exit and enter
// used to wrap every extend in separate pointwise launches (k_exit_pre / _mid / _mulc / _post, a device-to-device copy, k_enter_combine:
// seven HBM passes and a copy around the four extends of an exit level); all of them are products with per-position tables, so they
// fold into the twists: the tables are multiplied together once (k_exit_fuse_tables) and the LDS kernels' first / last pass do the rest.
//   load (every SM):   x = pre[p] * src[g << lshift]       lshift = 1 reads the even entries of an interleaved vector
//   SM 1 ("mid"):      out[g] = tb[p] * aux[(g << ashift) + aoff] + post[p] * x                 (post = -(wout * xnn_odd * z0inv))
//   SM 2 ("post"):     u = post[p] * x;  out[(2c) h + i] = u;  out[(2c + 1) h + i] = tb[p] * (aux[2 g] - u),   g = c h + i
//   SM 3 ("combine"):  enter's recombination, vectors 2c (lo) and 2c + 1 (hi) of one workgroup:
//                      out[c 2h + 2i] = aux[lo] + tb[i] * aux[hi];  out[c 2h + 2i + 1] = post[i] * x_lo + tc[i] * x_hi
// Products are lazy (fr.cuh): a sum of two of them is below 2.2 p, two conditional subtractions bring it home.
template <int SM>
struct ExtIo {
  const Fr30* pre = nullptr;
  int lshift = 0;
  const Fr30* post = nullptr;
  Fr* out = nullptr;
  const Fr30* tb = nullptr;
  const Fr30* tc = nullptr;
  const Fr* aux = nullptr;
  int ashift = 0, aoff = 0, lh = 0;
};
__device__ __forceinline__ Fr fr30_canon2(const Fr30& a) { return fr_cond_sub_p(fr_cond_sub_p(fr30_to_fr(a))); }
template <int SM>
__device__ __forceinline__ void io_load2(const ExtIo<SM>& io, const Fr* src, size_t g0, size_t g1, uint32_t p0, uint32_t p1, Fr30& r0, Fr30& r1) {
  if (io.pre) tw_in2(io.pre, p0, p1, src[g0 << io.lshift], src[g1 << io.lshift], r0, r1);
  else {
    r0 = ld30(src + g0);
    r1 = ld30(src + g1);
  }
}
// the last launch's stores for SM 0 .. 2 (two values of one thread; SM 3 pairs values across vectors: k_extend_fused does it itself)
template <int SM>
__device__ __forceinline__ void io_store2(const ExtIo<SM>& io, Fr* data, size_t g0, size_t g1, uint32_t p0, uint32_t p1, const Fr30& x0, const Fr30& x1) {
  if (SM == 0) {
    if (io.post) {
      Fr o0, o1;
      tw_out2(io.post, p0, p1, x0, x1, o0, o1);
      data[g0] = o0;
      data[g1] = o1;
    } else {
      st30(data + g0, x0);
      st30(data + g1, x1);
    }
  } else if (SM == 1) {
    const Fr30 z = fr30_zero();
    Fr30 a0, a1, y0, y1;
    fr30_muladd_x2(io.tb[p0], fr30_from(io.aux[(g0 << io.ashift) + io.aoff]), z, io.tb[p1], fr30_from(io.aux[(g1 << io.ashift) + io.aoff]), z, a0, a1);
    fr30_muladd_x2(io.post[p0], x0, a0, io.post[p1], x1, a1, y0, y1);
    io.out[g0] = fr30_canon2(y0);
    io.out[g1] = fr30_canon2(y1);
  } else if (SM == 2) {
    Fr u0, u1;
    tw_out2(io.post, p0, p1, x0, x1, u0, u1);
    const Fr d0 = fr_sub(io.aux[g0 << 1], u0), d1 = fr_sub(io.aux[g1 << 1], u1);
    const uint32_t hm = (1u << io.lh) - 1u;
    const size_t o0 = ((g0 >> io.lh) << (io.lh + 1)) + (g0 & hm), o1 = ((g1 >> io.lh) << (io.lh + 1)) + (g1 & hm);
    io.out[o0] = u0;
    io.out[o1] = u1;
    Fr v0, v1;
    tw_out2(io.tb, p0, p1, fr30_from(d0), fr30_from(d1), v0, v1);
    io.out[o0 + (hm + 1u)] = v0;
    io.out[o1 + (hm + 1u)] = v1;
  }
}

// Fused bottom of an extend: the last `lb` decompose layers and the first `lb` recombine layers only mix
// elements inside aligned blocks of 2^lb <= 2048 values, so a workgroup keeps 2048 consecutive values
// (64 KB) in LDS and runs all 2*lb butterfly layers on them in ONE launch and ONE HBM round trip (the
// per-layer kernels of ecfft_butterfly.cuh then cover only the top layers of long vectors).  The constants of these layers
// total < 0.25 MB per tree and are served from L2.  `data` is the concatenation of the batch vectors.
constexpr int FUSE_LOG = 11;
constexpr uint32_t FUSE_ELEMS = 1u << FUSE_LOG;
#ifndef DVP_FUSE_TPB
#define DVP_FUSE_TPB 512
#endif
constexpr int FUSE_TPB = DVP_FUSE_TPB;  // 64 KB of LDS per workgroup: two workgroups per CU, FUSE_TPB / 128 waves per SIMD

template <bool DEC, class MAP = TwId>
__device__ __forceinline__ void lds_bfly(Fr30* x, const Fr30* __restrict__ tws, int lh, uint32_t pairs, MAP f = MAP()) {
  const uint32_t h = 1u << lh;
  for (uint32_t q = threadIdx.x; q < pairs; q += blockDim.x) {
    uint32_t i = q & (h - 1);
    uint32_t i0 = ((q >> lh) << (lh + 1)) | i, i1 = i0 + h;
    Fr30 e0 = x[i0], e1 = x[i1];
    if (DEC) bf_dec(e0, e1, tw_load(tws, f(i))); else bf_rec(e0, e1, tw_load(tws, f(i)));
    x[i0] = e0;
    x[i1] = e1;
  }
  __syncthreads();
}
// two layers per barrier inside the block (the radix-4 step of k_butterfly4 on the LDS copy): half the barriers and half the LDS
// round trips of the per-layer loop.  lh2 = log2 of the narrow layer's pair distance; wide layer first when DEC.
// (Round 5 measured THREE layers per barrier, the radix-8 step of k_butterfly8 on the LDS copy, in this kernel and in k_extend_top:
// eight values and seven constant pairs per thread spill 250 B per lane at the 128 VGPRs of 512-thread workgroups and still cost a
// wave per SIMD at 384 threads -- the prover's three extends 0.77 -> 0.99 / 1.16 ms, enter 3.4 -> 3.9 / 4.3 ms: not kept.)
template <bool DEC, class MAP = TwId>
__device__ __forceinline__ void lds_bfly4(Fr30* x, const Fr30* __restrict__ tw_wide, const Fr30* __restrict__ tw_narrow, int lh2, uint32_t quads, MAP f = MAP()) {
  const uint32_t h2 = 1u << lh2, h1 = h2 << 1;
  for (uint32_t q = threadIdx.x; q < quads; q += blockDim.x) {
    const uint32_t j = q & (h2 - 1);
    const uint32_t i0 = ((q >> lh2) << (lh2 + 2)) | j;
    Fr30 x0 = x[i0], x1 = x[i0 + h2], x2 = x[i0 + h1], x3 = x[i0 + h1 + h2];
    radix4<DEC, MAP>(x0, x1, x2, x3, tw_wide, tw_narrow, j, h2, f);
    x[i0] = x0; x[i0 + h2] = x1; x[i0 + h1] = x2; x[i0 + h1 + h2] = x3;
  }
  __syncthreads();
}

template <int SM>
__global__ void __launch_bounds__(FUSE_TPB) __attribute__((amdgpu_waves_per_eu(FUSE_TPB / 128, FUSE_TPB / 128)))
k_extend_fused(const Fr* src /* == data unless this is the first pass of an out-of-place extend */, Fr* data, const Fr30* __restrict__ dec,
               const Fr30* __restrict__ rec, uint32_t n, int ln, int lb, size_t total, const ExtIo<SM> io) {
  __shared__ Fr30 x[FUSE_ELEMS];
  const size_t base = (size_t)blockIdx.x * FUSE_ELEMS;
  const uint32_t elems = (uint32_t)min((size_t)FUSE_ELEMS, total - base);
  const uint32_t pos0 = (uint32_t)(base & (size_t)(n - 1));  // position of the block's first value inside its vector (n is a power of two)
  // two values per thread and trip (k, k + elems / 2): their twist products are independent
  const uint32_t half = elems >> 1;  // elems is even: a batch of vectors of n >= 2 values
  for (uint32_t k = threadIdx.x; k < half; k += blockDim.x)
    io_load2(io, src, base + k, base + k + half, (pos0 + k) & (n - 1), (pos0 + k + half) & (n - 1), x[k], x[k + half]);
  __syncthreads();
  auto tw_of = [&](const Fr30* b, int L) { return b + 2 * (size_t)(n - (n >> (ln - lb + L))); };
  const bool whole = elems == FUSE_ELEMS || (elems & 3u) == 0;  // (a short last block still holds whole sub-blocks of every layer it runs)
  {
    int L = 0;  // decompose, sub-block size 2^(lb-L); two layers per barrier while two remain
    if (whole)
      for (; L + 1 < lb; L += 2) lds_bfly4<true>(x, tw_of(dec, L), tw_of(dec, L + 1), lb - L - 2, elems >> 2);
    for (; L < lb; ++L) lds_bfly<true>(x, tw_of(dec, L), lb - L - 1, elems >> 1);
  }
  {
    int L = lb - 1;  // recombine: the odd layer (the innermost one) first, as the decompose left it
    if (whole && (lb & 1)) { lds_bfly<false>(x, tw_of(rec, L), lb - L - 1, elems >> 1); --L; }
    if (whole)
      for (; L >= 1; L -= 2) lds_bfly4<false>(x, tw_of(rec, L - 1), tw_of(rec, L), lb - L - 1, elems >> 2);
    for (; L >= 0; --L) lds_bfly<false>(x, tw_of(rec, L), lb - L - 1, elems >> 1);
  }
  if (SM == 3) {
    // enter's combine: the block holds whole (lo, hi) pairs of vectors of n = 2^lh <= 1024 values (the host checks); thread q owns
    // position i of pair cl
    const int lh = io.lh;
    const uint32_t hm = n - 1u;
    for (uint32_t q = threadIdx.x; q < half; q += blockDim.x) {
      const uint32_t i = q & hm, e_lo = ((q >> lh) << (lh + 1)) + i, e_hi = e_lo + n;
      const Fr30 z = fr30_zero();
      Fr30 a, b, ye, yo;
      fr30_muladd_x2(io.post[i], x[e_lo], z, io.tb[i], fr30_from(io.aux[base + e_hi]), fr30_from(io.aux[base + e_lo]), a, ye);
      yo = fr30_muladd(io.tc[i], x[e_hi], a);
      const size_t o = base + ((size_t)(q >> lh) << (lh + 1)) + 2u * i;
      io.out[o] = fr30_canon2(ye);
      io.out[o + 1] = fr30_canon2(yo);
    }
    return;
  }
  for (uint32_t k = threadIdx.x; k < half; k += blockDim.x)
    io_store2(io, data, base + k, base + k + half, (pos0 + k) & (n - 1), (pos0 + k + half) & (n - 1), x[k], x[k + half]);
}

// Fused TOP of an extend (round 5): the `tl` layers d0 .. d0 + tl - 1 of a long vector mix values that sit S = n >> (d0 + tl) apart
// (the pair distance of the narrowest of them) inside blocks of n >> d0 values.  A workgroup takes a TILE of such a block -- R = 2^tl
// rows S apart, C = FUSE_ELEMS / R consecutive columns (a row of the tile is C x 32 B of consecutive memory: whole 128-byte lines
// from C = 4, i.e. tl <= 9) -- into LDS and runs all tl layers on it: ONE launch and one HBM round trip where k_butterfly8 took
// ceil(tl / 3).  The 2^20-constraint prover's extends (top = 9 layers above the 2048-value blocks of k_extend_fused) go from
// 3 + 1 + 3 launches to 1 + 1 + 1.  LDS position e = row * C + col; the constants of half-block position i of a layer sit at vector
// position (i / C) * S + col0 + i % C (TwTile).  DEC: wide layer first (the first launch of an extend, with the input twist `pre`);
// otherwise narrow first (the last launch, with the output twist `post`).  In place: a tile is read completely before it is written
// and no two workgroups share a value.
struct TwTile {
  uint32_t lc, ls, col0;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return ((i >> lc) << ls) + col0 + (i & ((1u << lc) - 1u)); }
};
template <bool DEC, int SM>
__global__ void __launch_bounds__(FUSE_TPB) __attribute__((amdgpu_waves_per_eu(FUSE_TPB / 128, FUSE_TPB / 128)))
k_extend_top(const Fr* src, Fr* data, const Fr30* __restrict__ tw /* dec or rec, whole table */, uint32_t n, int ln, int d0, int tl,
             uint32_t batch, const ExtIo<SM> io) {
  __shared__ Fr30 x[FUSE_ELEMS];
  // SM 3 (enter's combine, last launch, d0 == 0): a tile takes its rows from vectors 2u AND 2u + 1 -- the rows of a vector are
  // S = n >> tl apart and 2^tl S = n, so row 2^tl + r of the "unit" (2u, 2u + 1) is row r of vector 2u + 1: twice the rows, half the
  // columns, and x[k], x[k + half] are the two vectors' values at the same position, which is what the combine pairs
  constexpr int PR = SM == 3 ? 1 : 0;
  const int lc = FUSE_LOG - tl - PR, ls = ln - d0 - tl;   // log2 of the tile's columns and of the row distance
  const uint32_t groups = 1u << (ls - lc);                // tiles per block of n >> d0 values (per unit of two vectors with SM 3)
  // workgroup -> (vector, tile of that vector).  The same tile of the `batch` vectors reads the same constants (64 bytes per pair
  // and layer: as many bytes as the data), and consecutive workgroups go to the 8 XCDs in turn: eight tiles of vector 0, the same
  // eight of vector 1, .. -- so that the workgroups sharing constants land on the SAME XCD one dispatch round apart and the second
  // and third find them in its L2 (a tile-major order put them on three different XCDs: three fetches from memory)
  // (a vector of fewer than eight tiles -- the many short vectors of an enter / exit level -- is walked tile by tile)
  const uint32_t tpv = (n << PR) >> FUSE_LOG;  // tiles per vector (per unit)
  const uint32_t per8 = 8u * (batch >> PR), grp8 = blockIdx.x / per8, rem = blockIdx.x - grp8 * per8;
  const uint32_t vec = tpv >= 8u ? rem >> 3 : blockIdx.x / tpv, tv = tpv >= 8u ? ((grp8 << 3) | (rem & 7u)) : blockIdx.x - vec * tpv;
  const uint32_t gb = (vec << d0) + (tv >> (ls - lc)), cg = tv & (groups - 1u);
  const size_t base = ((size_t)gb << (ln - d0 + PR)) + ((size_t)cg << lc);
  const uint32_t cmask = (1u << lc) - 1u, half = FUSE_ELEMS >> 1;
  auto gidx = [&](uint32_t e) -> size_t { return base + ((size_t)(e >> lc) << ls) + (e & cmask); };
  for (uint32_t k = threadIdx.x; k < half; k += blockDim.x) {
    const size_t g0 = gidx(k), g1 = gidx(k + half);
    io_load2(io, src, g0, g1, (uint32_t)(g0 & (size_t)(n - 1)), (uint32_t)(g1 & (size_t)(n - 1)), x[k], x[k + half]);
  }
  __syncthreads();
  const TwTile f{(uint32_t)lc, (uint32_t)ls, cg << lc};
  auto tw_of = [&](int L) { return tw + 2 * (size_t)(n - (n >> (d0 + L))); };  // layer d0 + L: rows 2^(tl - 1 - L) apart
  if (DEC) {
    int L = 0;
    for (; L + 1 < tl; L += 2) lds_bfly4<true, TwTile>(x, tw_of(L), tw_of(L + 1), tl - L - 2 + lc, FUSE_ELEMS >> 2, f);
    for (; L < tl; ++L) lds_bfly<true, TwTile>(x, tw_of(L), tl - L - 1 + lc, FUSE_ELEMS >> 1, f);
  } else {
    int L = tl - 1;
    if (tl & 1) { lds_bfly<false, TwTile>(x, tw_of(L), tl - L - 1 + lc, FUSE_ELEMS >> 1, f); --L; }
    for (; L >= 1; L -= 2) lds_bfly4<false, TwTile>(x, tw_of(L - 1), tw_of(L), tl - L - 1 + lc, FUSE_ELEMS >> 2, f);
  }
  if (SM == 3) {
    for (uint32_t k = threadIdx.x; k < half; k += blockDim.x) {
      const size_t g0 = gidx(k), g1 = g0 + n;  // == gidx(k + half): the same position of vector 2u + 1
      const uint32_t i = (uint32_t)(g0 & (size_t)(n - 1));
      const Fr30 z = fr30_zero();
      Fr30 a, ye, yo;
      fr30_muladd_x2(io.post[i], x[k], z, io.tb[i], fr30_from(io.aux[g1]), fr30_from(io.aux[g0]), a, ye);
      yo = fr30_muladd(io.tc[i], x[k + half], a);
      io.out[g0 + i] = fr30_canon2(ye);  // unit u starts at u 2n = g0 - i: out[u 2n + 2i], out[u 2n + 2i + 1]
      io.out[g0 + i + 1] = fr30_canon2(yo);
    }
    return;
  }
  for (uint32_t k = threadIdx.x; k < half; k += blockDim.x) {
    const size_t g0 = gidx(k), g1 = gidx(k + half);
    io_store2(io, data, g0, g1, (uint32_t)(g0 & (size_t)(n - 1)), (uint32_t)(g1 & (size_t)(n - 1)), x[k], x[k + half]);
  }
}

}  // namespace dvp
