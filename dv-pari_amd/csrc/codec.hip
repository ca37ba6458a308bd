// xsk233 30-byte codec, batched fixed-base multiplication (the SRS commitment loop) and the
// wire-format MSM entry point.
//
//   CurvePoint::to_bytes / from_bytes       src/curve.rs:93-109      -> dvp_points_encode / _decode
//   read_point_vec_from_file's decode loop  src/io_utils.rs:217-226  -> dvp_points_decode
//   point_scalar_mul_gen sweeps             src/srs.rs:130-133,138-144,155-158 -> dvp_mulgen_batch*
//   multi_scalar_mul on file-format inputs  src/proving.rs:462-463,511-512,666-680 -> dvp_msm_xsk233
//
// CODEC RULE (candidate; byte-level parity with xs233 is UNPINNED -- the reference holds no
// known-answer bytes and the xs233 source is not available offline):
//   xsk233 = { P + N : P in E[r] }, N = (0,1).  With (x,s)-coordinates on the N=(0,0) model,
//   Pornin's encoding is w = sqrt(s/x) of the element P + N; expressed on the E[r] representative
//   P = (x,y) that is  w = sqrt(x + y/x + 1)  (lambda-coordinate of P plus one); neutral -> 0.
//   Decoding: e = w^2 + w, solve x^2 + e x + 1 = 0 (half-trace), roots are x(P) and x(P+N) = 1/x;
//   y = x (w^2 + 1 + x); keep the root whose point lies in E[r] = 4E (two trace tests).
#include <atomic>
#include <cstdlib>

#include "common.h"
#include "k233.cuh"
#include "tau.cuh"
#include "codec.cuh"
#include "host_api.h"

namespace dvp {

// NIST K-233 base point
__constant__ uint32_t K233_GX[8] = {0xefad6126u, 0x0a4c9d6eu, 0x19c26bf5u, 0x149563a4u,
                                    0x29f22ff4u, 0x7e731af1u, 0x32ba853au, 0x00000172u};
__constant__ uint32_t K233_GY[8] = {0x56fae6a3u, 0x56e0c110u, 0xf18aeb9bu, 0x27a8cd9bu,
                                    0x555a67c4u, 0x19b7f70fu, 0x537dece8u, 0x000001dbu};

__device__ __forceinline__ bool k233_on_curve(const Aff& p) {
  // y^2 + xy = x^3 + 1
  Gf lhs = gf_add(gf_sqr(p.y), gf_mul(p.x, p.y));
  Gf rhs = gf_add(gf_mul(gf_sqr(p.x), p.x), gf_one());
  return gf_eq(lhs, rhs);
}

__global__ void __launch_bounds__(256)
k_encode(const Aff* __restrict__ pts, const uint8_t* __restrict__ inf, size_t n, GfSqrTables T, uint8_t* __restrict__ out, int rule) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Gf w = gf_zero();
  if (!(inf && inf[i])) {
    Aff p = pts[i];
    Gf lam1 = gf_add(gf_add(p.x, gf_mul(p.y, gf_inv_fast(p.x, T, L), L)), gf_one());
    w = gf_sqr_tab(gf_sqr_tab(lam1, T.t116), T.t116);  // sqrt = 232 squarings = two 116-step table passes
    if (rule) w = codec_present(w, rule, T);
  }
  store30(out + i * 30, w, rule);
}

// one point (a proof's commit_p / kzg_k), latency only: one quad of lanes through the quad-cooperative multiplier
// (45 us against 90 for a single lane), infinity flag read as the u32 the MSM writes
__global__ void __launch_bounds__(64)
k_encode_point(const Aff* __restrict__ pt, const uint32_t* __restrict__ inf32, GfSqrTables T, uint8_t* __restrict__ out, int rule) {
  extern __shared__ char lds_raw[];
  GfLdsQ L = gf_ldsq_init(lds_raw);
  if (threadIdx.x >= 4) return;
  Gf w = gf_zero();
  if (!*inf32) {
    Aff p = *pt;
    Gf lam1 = gf_add(gf_add(p.x, gf_mul(p.y, gf_inv_fast(p.x, T, L), L)), gf_one());
    w = gf_sqr_tab(gf_sqr_tab(lam1, T.t116), T.t116);
    if (rule) w = codec_present(w, rule, T);
  }
  if (threadIdx.x == 0) store30(out, w, rule);
}

__global__ void __launch_bounds__(256, 2)
k_decode(const uint8_t* __restrict__ enc, size_t n, GfSqrTables T, Aff* __restrict__ out, uint8_t* __restrict__ inf,
         unsigned long long* __restrict__ err, int rule) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Aff r;
  bool is_inf;
  bool ok = codec_decode(enc + i * 30, rule, T, L, r, is_inf);
  if (!ok) {
    atomicMin(err, (unsigned long long)i);
    is_inf = true;
  }
  out[i] = r;
  inf[i] = is_inf ? 1 : 0;
}

// One affine point per lane -> one class byte (include/dvpari.h: DVP_POINT_*), for the entries that take affine points from a caller:
// the kernels behind them assume reduced coordinates and points of E[r].  The classes partition the curve's affine points: E = E[r] x
// Z/4, so a point is in E[r], in E[r] + N (N = (0,1), the point of order 2: xsk233's own view of a group element), or -- Tr(x) = 1 --
// outside 2E.  Tr(x) = 0 puts P in 2E; of 2E = E[r] u (E[r] + N) the half's trace test (k233_in_subgroup) keeps E[r].
// The three products x y, x x^2 (curve equation) and (lambda + 1) x (the half) share the operand x and so ONE build of its half tables
// (gf_mul3); lambda is a table pass over x alone, so all three multipliers are known before the first lookup.  An unreduced
// coordinate never reaches the multiplier (gf_k_split / gf_k_combine assume reduced operands): such a lane is classified first and
// skips the arithmetic, as do the lanes of points at infinity.
// summary = { first bad index (atomicMin), number of bad points }: both from the lowest bad lane of a wave only, so clean input pays
// for no atomic at all.
__global__ void __launch_bounds__(256, 2)
k_points_check(const Aff* __restrict__ pts, const uint8_t* __restrict__ inf, size_t n, GfSqrTables T, uint8_t* __restrict__ classes,
               unsigned long long* __restrict__ summary) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t cls = 0;
  if (i < n && !(inf && inf[i])) {
    Aff p = pts[i];
    if ((p.x.w[7] | p.y.w[7]) >> 9) {
      cls = DVP_POINT_UNREDUCED;
    } else {
      Gf lam1 = gf_sqr_tab(p.x, T.th);  // lam^2 + lam = x when Tr(x) = 0 (some reduced element otherwise: unused then)
      lam1.w[0] ^= 1u;
      Gf xy, x3, lx;
      gf_mul3(p.y, gf_sqr(p.x), lam1, p.x, L, xy, x3, lx);
      Gf d = gf_add(gf_add(gf_sqr(p.y), xy), x3);  // y^2 + xy + x^3 + 1
      d.w[0] ^= 1u;
      if (!gf_is_zero(d)) cls = DVP_POINT_OFF_CURVE;
      else if (gf_is_zero(p.x)) cls = DVP_POINT_COSET_N;  // N itself
      else if (gf_trace(p.x)) cls = DVP_POINT_ORDER4;
      else if (gf_trace(gf_add(p.y, lx))) cls = DVP_POINT_COSET_N;  // x_half^2 = y + (lambda + 1) x
    }
  }
  if (i < n && classes) classes[i] = (uint8_t)cls;
  const unsigned long long bad = __ballot(cls != 0);
  if (bad && (threadIdx.x & 63) == (unsigned)__ffsll((long long)bad) - 1) {  // lanes hold ascending indices: the lowest bad lane has the wave's first
    atomicMin(summary, (unsigned long long)i);
    atomicAdd(summary + 1, (unsigned long long)__popcll(bad));
  }
}

// ---- fixed-base tables: tab[w][d] = sum_t d_t tau^(c w + t)(G), affine ------------------------------

__global__ void __launch_bounds__(256) k_gen_table(Aff* __restrict__ tab) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (uint32_t)(GEN_W << GEN_C)) return;
  uint32_t w = tid >> GEN_C, d = tid & ((1u << GEN_C) - 1);
  Aff g;
#pragma unroll
  for (int k = 0; k < 8; ++k) { g.x.w[k] = K233_GX[k]; g.y.w[k] = K233_GY[k]; }
  // g <- tau^(c w)(G)
  for (uint32_t s = 0; s < w * GEN_C; ++s) { g.x = gf_sqr(g.x); g.y = gf_sqr(g.y); }
  Ld acc = ld_infinity();
  for (int t = 0; t < GEN_C; ++t) {
    if ((d >> t) & 1) acc = ld_madd(acc, g);
    g.x = gf_sqr(g.x);
    g.y = gf_sqr(g.y);
  }
  Aff a;
  ld_to_aff(acc, &a);
  tab[tid] = a;  // d == 0 -> zeros, never read
}

__global__ void __launch_bounds__(256, 2)
k_mulgen(const uint32_t* __restrict__ scalars, size_t n, const Aff* __restrict__ tab, GfSqrTables T, Aff* __restrict__ out,
         uint8_t* __restrict__ out_inf, unsigned long long* __restrict__ err) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = scalars[i * 8 + k];
  uint32_t r0[5], r1[5];
  if (!tau_scalar_is_canonical(s)) {
    atomicMin(err, (unsigned long long)i);
#pragma unroll
    for (int k = 0; k < 5; ++k) r0[k] = r1[k] = 0;
  } else {
    tau_partial_reduce(s, r0, r1);
  }
  // digits sixteen per step (tau.cuh), windows of GEN_C cut from a 64-bit shift register; LDS-comb products
  Ld acc = ld_infinity();
  uint64_t buf = 0;
  int nb = 0, w = 0;
#pragma unroll 1
  for (int done = 0; done < GEN_W * GEN_C; done += 16) {
    buf |= (uint64_t)tau_step16(r0, r1) << nb;
    nb += 16;
    while (nb >= GEN_C && w < GEN_W) {
      uint32_t d = (uint32_t)buf & ((1u << GEN_C) - 1);
      buf >>= GEN_C;
      nb -= GEN_C;
      if (d) ld_madd_ip(acc, tab[((size_t)w << GEN_C) + d], L);
      ++w;
    }
  }
  Aff a;
  a.x = gf_zero();
  a.y = gf_zero();
  bool fin = !ld_is_inf(acc);
  if (fin) {
    Gf zi = gf_inv_fast(acc.Z, T, L);
    a.x = gf_mul(acc.X, zi, L);
    a.y = gf_mul(acc.Y, gf_sqr(zi), L);
  }
  out[i] = a;
  out_inf[i] = fin ? 0 : 1;
}

// the rule in force: DVP_CODEC_RULE from the environment at first use, dvp_codec_set_rule at run time
static std::atomic<int> g_codec_rule{-1};
static int codec_rule() {
  int r = g_codec_rule.load();
  if (r < 0) {
    const char* e = getenv("DVP_CODEC_RULE");
    r = e ? atoi(e) : 0;
    if (r < 0 || r >= CODEC_RULES) r = 0;
    g_codec_rule.store(r);
  }
  return r;
}

int codec_rule_now() { return codec_rule(); }  // verify.hip

static PerDevice<Aff> g_gen_tab;

int gen_table(const Aff** out, hipStream_t st) {
  Aff* tab;
  DVP_TRY(g_gen_tab.get(&tab, [&](Aff** t) -> int {
    const size_t cnt = (size_t)GEN_W << GEN_C;
    DVP_HIP(hipMalloc((void**)t, cnt * sizeof(Aff)));
    DVP_LAUNCH(k_gen_table, dim3(cdiv(cnt, 256)), dim3(256), 0, st, *t);
    DVP_HIP(hipGetLastError());
    DVP_HIP(hipStreamSynchronize(st));
    return DVP_OK;
  }));
  *out = tab;
  return DVP_OK;
}

int mulgen_dev(const void* d_scalars, size_t n, Aff* d_out, uint8_t* d_inf, hipStream_t st) {
  const Aff* tab;
  DVP_TRY(gen_table(&tab, st));
  ErrWord err;
  DVP_TRY(err.arm(st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_mulgen, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const uint32_t*)d_scalars, n, tab, T, d_out,
                     d_inf, err.word());
  DVP_HIP(hipGetLastError());
  return err.verdict(st, DVP_EINVAL);
}

int encode_dev(const Aff* d_pts, const uint8_t* d_inf, size_t n, uint8_t* d_out, hipStream_t st) {
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_encode, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, d_pts, d_inf, n, T, d_out, codec_rule());
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

int encode_point_dev(const Aff* d_pt, const uint32_t* d_inf32, uint8_t* d_out, hipStream_t st) {
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_encode_point, dim3(1), dim3(64), GF_LDS_BYTES_PER_WAVE, st, d_pt, d_inf32, T, d_out, codec_rule());
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

int decode_dev(const uint8_t* d_enc, size_t n, Aff* d_out, uint8_t* d_inf, hipStream_t st) {
  ErrWord err;
  DVP_TRY(err.arm(st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_decode, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, d_enc, n, T, d_out, d_inf, err.word(), codec_rule());
  DVP_HIP(hipGetLastError());
  return err.verdict(st, DVP_EDECODE);
}

// enqueue only: d_summary (16 bytes) is reset here, then k_points_check fills it
int points_check_dev(const void* d_xy, const void* d_inf, size_t n, void* d_classes, void* d_summary, hipStream_t st) {
  DVP_TRY(summary_reset(d_summary, st));
  if (!n) return DVP_OK;
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_points_check, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const Aff*)d_xy, (const uint8_t*)d_inf, n, T,
                     (uint8_t*)d_classes, (unsigned long long*)d_summary);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

// the check and its verdict: waits for `st`.  DVP_EPOINT with g_last_error_index = the first bad point
int points_check_wait(const void* d_xy, const void* d_inf, size_t n, void* d_classes, size_t* n_bad, hipStream_t st) {
  ErrWord sum;
  DVP_TRY(sum.alloc(16));
  DVP_TRY(points_check_dev(d_xy, d_inf, n, d_classes, sum.p, st));  // resets the summary
  return sum.verdict(st, DVP_EPOINT, n_bad);
}

// strict mode: DVP_POINTS_STRICT from the environment at first use, dvp_points_set_strict at run time
static std::atomic<int> g_points_strict{-1};
static int points_strict() {
  int s = g_points_strict.load();
  if (s < 0) {
    const char* e = getenv("DVP_POINTS_STRICT");
    s = (e && atoi(e) != 0) ? 1 : 0;
    g_points_strict.store(s);
  }
  return s;
}
// what the entries that copy affine points from a caller run on their device copy (msm.hip, prove.hip and below): nothing when strict is off
int points_check_strict(const void* d_xy, const void* d_inf, size_t n, hipStream_t st) {
  if (!n || !points_strict()) return DVP_OK;
  return points_check_wait(d_xy, d_inf, n, nullptr, nullptr, st);
}

// CurvePoint::add over two vectors (src/curve.rs:84-90): out[i] = a[i] + b[i] on the E[r] representative; complete
// (doubling, inverses and the neutral element are handled), register-only arithmetic -- a convenience entry, not a hot path.
__global__ void __launch_bounds__(128)
k_points_add(const Aff* __restrict__ a, const uint8_t* __restrict__ ainf, const Aff* __restrict__ b, const uint8_t* __restrict__ binf,
             size_t n, Aff* __restrict__ out, uint8_t* __restrict__ oinf) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Ld acc = (ainf && ainf[i]) ? ld_infinity() : ld_from_aff(a[i]);
  if (!(binf && binf[i])) acc = ld_madd(acc, b[i]);
  Aff r;
  bool fin = ld_to_aff(acc, &r);
  out[i] = r;
  oinf[i] = fin ? 0 : 1;
}

}  // namespace dvp

using namespace dvp;

extern "C" int dvp_mulgen_batch_affine(const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
  if (!n) return DVP_OK;
  if (!scalars || !out_xy || !out_inf) return DVP_EINVAL;
  DevBuf ds, dp, di;
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(dp.alloc(n * 64));
  DVP_TRY(di.alloc(n));
  DVP_TRY(mulgen_dev(ds.p, n, dp.as<Aff>(), di.as<uint8_t>(), 0));
  DVP_TRY(dp.down(out_xy, n * 64));
  return di.down(out_inf, n);
}

extern "C" int dvp_mulgen_batch(const uint64_t* scalars, size_t n, uint8_t* out_enc) {
  if (!n) return DVP_OK;
  if (!scalars || !out_enc) return DVP_EINVAL;
  DevBuf ds, dp, di, de;
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(dp.alloc(n * 64));
  DVP_TRY(di.alloc(n));
  DVP_TRY(de.alloc(n * 30));
  DVP_TRY(mulgen_dev(ds.p, n, dp.as<Aff>(), di.as<uint8_t>(), 0));
  DVP_TRY(encode_dev(dp.as<Aff>(), di.as<uint8_t>(), n, de.as<uint8_t>(), 0));
  return de.down(out_enc, n * 30);
}

extern "C" int dvp_points_encode(const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_enc) {
  if (!n) return DVP_OK;
  if (!xy || !out_enc) return DVP_EINVAL;
  DevBuf dp, di, de;
  DVP_TRY(dp.up(xy, n * 64));
  DVP_TRY(di.up_opt(inf, n));
  DVP_TRY(de.alloc(n * 30));
  DVP_TRY(points_check_strict(dp.p, di.p, n, 0));
  DVP_TRY(encode_dev(dp.as<Aff>(), di.as<uint8_t>(), n, de.as<uint8_t>(), 0));
  return de.down(out_enc, n * 30);
}

extern "C" int dvp_points_add(const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, size_t n,
                              uint64_t* out_xy, uint8_t* out_inf) {
  if (!n) return DVP_OK;
  if (!a_xy || !b_xy || !out_xy || !out_inf) return DVP_EINVAL;
  DevBuf da, db, dai, dbi, dout, doi;
  DVP_TRY(da.up(a_xy, n * 64));
  DVP_TRY(db.up(b_xy, n * 64));
  DVP_TRY(dai.up_opt(a_inf, n));
  DVP_TRY(dbi.up_opt(b_inf, n));
  DVP_TRY(dout.alloc(n * 64));
  DVP_TRY(doi.alloc(n));
  DVP_TRY(points_check_strict(da.p, dai.p, n, 0));  // operand a first: the index is b's only when a is clean
  DVP_TRY(points_check_strict(db.p, dbi.p, n, 0));
  DVP_LAUNCH(k_points_add, dim3(cdiv(n, 128)), dim3(128), 0, 0, da.as<Aff>(), dai.as<uint8_t>(), db.as<Aff>(), dbi.as<uint8_t>(), n,
                     dout.as<Aff>(), doi.as<uint8_t>());
  DVP_HIP(hipGetLastError());
  DVP_TRY(dout.down(out_xy, n * 64));
  return doi.down(out_inf, n);
}

extern "C" int dvp_points_decode(const uint8_t* enc, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
  if (!n) return DVP_OK;
  if (!enc || !out_xy || !out_inf) return DVP_EINVAL;
  DevBuf dp, di, de;
  DVP_TRY(dp.alloc(n * 64));
  DVP_TRY(di.alloc(n));
  DVP_TRY(de.up(enc, n * 30));
  const int rc = decode_dev(de.as<uint8_t>(), n, dp.as<Aff>(), di.as<uint8_t>(), 0);
  // the outputs go back even when an encoding was bad (DVP_EDECODE): that lane is flagged, the others hold their points
  DVP_TRY(dp.down(out_xy, n * 64));
  DVP_TRY(di.down(out_inf, n));
  return rc;
}

extern "C" int dvp_points_check(const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* classes, size_t* n_bad) {
  if (!n) return DVP_OK;
  if (!xy) return DVP_EINVAL;
  DevBuf dp, di, dc;
  DVP_TRY(dp.up(xy, n * 64));
  DVP_TRY(di.up_opt(inf, n));
  if (classes) DVP_TRY(dc.alloc(n));
  const int rc = points_check_wait(dp.p, di.p, n, dc.p, n_bad, 0);
  if (classes && (rc == DVP_OK || rc == DVP_EPOINT)) DVP_TRY(dc.down(classes, n));  // a bad point is a finding: its classes go back with it
  return rc;
}

extern "C" int dvp_points_check_dev(const void* d_xy, const void* d_inf, size_t n, void* d_classes, void* d_summary, void* stream) {
  if ((n && !d_xy) || !d_summary) return DVP_EINVAL;
  return points_check_dev(d_xy, d_inf, n, d_classes, d_summary, (hipStream_t)stream);
}

extern "C" int dvp_points_set_strict(int on) {
  g_points_strict.store(on ? 1 : 0);
  return DVP_OK;
}
extern "C" int dvp_points_get_strict(void) { return points_strict(); }

// k_points_check and k_decode alone on the same count, device events, median of `reps` after one warm-up launch each (tools/points_check.py)
extern "C" int dvp_ubench_points_check(const void* d_xy, const void* d_inf, const void* d_enc, size_t n, void* d_scratch, int reps,
                                       double* check_ms, double* decode_ms) {
  if (!d_xy || !d_enc || !d_scratch || !n || reps < 1 || reps > 99 || !(reps & 1) || !check_ms || !decode_ms) return DVP_EINVAL;
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, 0));
  DevBuf sum;
  DVP_TRY(sum.alloc(16));
  DVP_HIP(hipMemset(sum.p, 0xff, 16));
  const int rule = codec_rule();
  const dim3 grid(cdiv(n, 256)), block(256);
  DVP_TRY(median_ms(reps, "dvp_ubench_points_check", [&]() -> int {
    DVP_LAUNCH(k_points_check, grid, block, 4 * GF_LDSK_BYTES_PER_WAVE, 0, (const Aff*)d_xy, (const uint8_t*)d_inf, n, T, (uint8_t*)nullptr,
                       sum.as<unsigned long long>());
    return DVP_OK;
  }, check_ms));
  return median_ms(reps, "dvp_ubench_points_check", [&]() -> int {
    DVP_LAUNCH(k_decode, grid, block, 4 * GF_LDSK_BYTES_PER_WAVE, 0, (const uint8_t*)d_enc, n, T, (Aff*)d_scratch, (uint8_t*)d_scratch + n * 64,
                       sum.as<unsigned long long>(), rule);
    return DVP_OK;
  }, decode_ms);
}

// dvp_points_mul_dev (its two 8-byte fills and k_points_mul at the width in force) and k_mulgen alone on the same scalars and count, device
// events, median of `reps` after one warm-up each (tools/points_mul.py)
extern "C" int dvp_ubench_points_mul(const void* d_scalars, const void* d_xy, size_t n, void* d_scratch, int reps, double* mul_ms, double* mulgen_ms) {
  if (!d_scalars || !d_xy || !d_scratch || !n || reps < 1 || reps > 99 || !(reps & 1) || !mul_ms || !mulgen_ms) return DVP_EINVAL;
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, 0));
  const Aff* tab;
  DVP_TRY(gen_table(&tab, 0));
  DevBuf sum;
  DVP_TRY(sum.alloc(16));
  DVP_HIP(hipMemset(sum.p, 0xff, 16));
  DVP_TRY(median_ms(reps, "dvp_ubench_points_mul", [&]() -> int {
    return points_mul_dev(d_scalars, n, d_xy, nullptr, n, d_scratch, (uint8_t*)d_scratch + n * 64, sum.p, 0);
  }, mul_ms));
  return median_ms(reps, "dvp_ubench_points_mul", [&]() -> int {
    DVP_LAUNCH(k_mulgen, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, 0, (const uint32_t*)d_scalars, n, tab, T, (Aff*)d_scratch,
                       (uint8_t*)d_scratch + n * 64, sum.as<unsigned long long>());
    return DVP_OK;
  }, mulgen_ms);
}

// scalars: n x 32 B canonical LE (ark: as arkworks holds them, converted in the device buffer they were copied into, fr_ark.hip);
// bases: n x 30 B xsk233 encodings; out: 30 B encoding of the sum
static int msm_xsk233(const uint8_t* scalars, bool ark, const uint8_t* bases_enc, size_t n, uint8_t out_enc[30]) {
  if ((n && (!scalars || !bases_enc)) || !out_enc) return DVP_EINVAL;
  DevBuf ds, dp, di, de, dout;
  MsmResult sum;
  DVP_TRY(ds.up(scalars, n * 32));  // a byte copy: the scalars may sit at any address
  DVP_TRY(de.up(bases_enc, n * 30));
  DVP_TRY(dp.alloc(n * 64));
  DVP_TRY(di.alloc(n));
  DVP_TRY(dout.alloc(30));
  DVP_TRY(sum.init());
  if (n) {
    if (ark) DVP_TRY(dvp_fr_from_ark_dev(ds.p, n, ds.p, nullptr));
    DVP_TRY(decode_dev(de.as<uint8_t>(), n, dp.as<Aff>(), di.as<uint8_t>(), 0));
  }
  DVP_TRY(msm_affine_dev(ds.p, dp.p, di.p, n, sum.out(), 0));
  DVP_TRY(encode_dev(sum.as<Aff>(), sum.inf8(), 1, dout.as<uint8_t>(), 0));
  return dout.down(out_enc, 30);
}
extern "C" int dvp_msm_xsk233(const uint8_t* scalars, const uint8_t* bases_enc, size_t n, uint8_t out_enc[30]) {
  return msm_xsk233(scalars, false, bases_enc, n, out_enc);
}
// multi_scalar_mul(&[Fr], &[CurvePoint]) with the scalars as the slice holds them (src/curve.rs:141-158)
extern "C" int dvp_msm_xsk233_ark(const uint64_t* scalars_ark, const uint8_t* bases_enc, size_t n, uint8_t out_enc[30]) {
  return msm_xsk233((const uint8_t*)scalars_ark, true, bases_enc, n, out_enc);
}

// which presentation of the encoded field element the 30 bytes hold (see the table at the top of this file); 0 = the default
// candidate.  Affects every later encode / decode of the process (SRS files written under one rule must be read under it).
extern "C" int dvp_codec_set_rule(int rule) {
  if (rule < 0 || rule >= CODEC_RULES) return DVP_EINVAL;
  g_codec_rule.store(rule);
  return DVP_OK;
}
extern "C" int dvp_codec_get_rule(void) { return codec_rule(); }
