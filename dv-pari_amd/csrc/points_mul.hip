// A vector of variable-base scalar multiplications: out[i] = k_i P_i, the reference's point_scalar_mul (src/curve.rs:113-126), the
// operation its multi_scalar_mul is made of.  One lane per pair, one launch (k_points_mul<W>):
//
//   table    alpha_u P for the 2^(W-2) odd u < 2^(W-1) (tau.cuh: alpha_u = beta_u + gamma_u tau = u mods tau^W), each one addition of
//            a multiple P, 2P or 3P and the Frobenius image of another, brought to affine with ONE inversion per lane (Montgomery's
//            trick), kept in LDS
//   recode   width-W tau-NAF of the partially reduced scalar (tnaf_step), written to LDS as a list of the non-zero digits
//   loop     left to right over that list: one complete mixed addition of +-table[u] per non-zero digit, then tau (three squarings of
//            the Lopez-Dahab accumulator) once per position down to the next one
//   output   affine through gf_inv_fast, as k_mulgen
//
// Why a LIST of non-zero digits and not one loop trip per position: the lanes of a wave hold different scalars, so with one trip per
// position some lane of the 64 has a non-zero digit at almost every position and the wave would run an addition in each of the ~240
// trips, whatever W is.  With one trip per non-zero digit a wave runs max over its lanes of the digit COUNT (about 240 / (W + 1) plus
// a few) additions; the price is that the squarings of a trip run for the longest gap among the lanes.
//
// LDS per wave (one wave per workgroup): 8 KB multiplier tables | 4 KB x 2^(W-2) point table | digit list (128 B per record row),
// which the table build uses first for the Z coordinates and prefix products of its shared inversion: 26, 32 and 64 KB for W = 3, 4, 5.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "k233.cuh"
#include "tau.cuh"
#include "host_api.h"

namespace dvp {


constexpr int PM_DEFAULT_W = 3;  // the fastest of the three at 2^20 pairs (tools/README.md)

template <int W>
struct PmShape {
  static constexpr TnafTable tab = TnafDigits<W>::table;
  static constexpr int NE = 1 << (W - 2);
  static constexpr int DIGITS = TnafDigits<W>::value;
  static constexpr int MAXREC = TnafDigits<W>::max_nonzero;
  static constexpr uint32_t TABLE_OFF = GF_LDSK_BYTES_PER_WAVE;
  static constexpr uint32_t TABLE_BYTES = (uint32_t)NE * 4096;
  static constexpr uint32_t REC_OFF = TABLE_OFF + TABLE_BYTES;
  static constexpr uint32_t REC_BYTES_RAW = std::max<uint32_t>((uint32_t)MAXREC * 128, (uint32_t)(NE > 1 ? NE - 1 + (NE > 3 ? NE - 3 : 0) : 0) * 2048);
  static constexpr uint32_t REC_BYTES = (REC_BYTES_RAW + 1023) & ~1023u;
  static constexpr uint32_t LDS_BYTES = REC_OFF + REC_BYTES;
  static_assert(DIGITS <= 256, "a position must fit the 8 bits of a record");
  static_assert(tab.beta[0] == 1 && tab.gamma[0] == 0, "alpha_1 = 1: entry 0 is P itself");
};
// how entry e of the table is made: alpha_(2e+1) P = sign (|b| P + rel tau(|g| P)), sign = the sign of b, rel = sign(b) sign(g)
struct PmDesc {
  int ab, ag, rel_neg, neg;
};
template <int W>
struct PmDescs {
  PmDesc d[TNAF_MAX_ENTRIES];
};
template <int W>
constexpr PmDescs<W> pm_descs() {
  PmDescs<W> r{};
  constexpr TnafTable t = TnafDigits<W>::table;
  for (int e = 0; e < t.entries; ++e) {
    r.d[e].ab = tnaf_iabs(t.beta[e]);
    r.d[e].ag = tnaf_iabs(t.gamma[e]);
    r.d[e].rel_neg = (t.beta[e] < 0) != (t.gamma[e] < 0);
    r.d[e].neg = t.beta[e] < 0;
  }
  return r;
}
template <int W>
__constant__ const PmDescs<W> PM_DESCS = pm_descs<W>();
constexpr bool pm_descs_ok(const TnafTable& t) {  // the build has P, 2P and 3P, and both parts of an entry beyond the first are there
  for (int e = 1; e < t.entries; ++e) {
    const int ab = tnaf_iabs(t.beta[e]), ag = tnaf_iabs(t.gamma[e]);
    if (ab < 1 || ab > 3 || ag < 1 || ag > 3) return false;
  }
  return true;
}

// one Gf / one affine point of this lane in LDS: 16-byte chunks 1 KB apart, lane-interleaved (conflict-free ds_read_b128)
GF_DEV void pm_st(uint32_t addr, const Gf& a) {
  gf_lds_st(addr, (gf_u32x4){a.w[0], a.w[1], a.w[2], a.w[3]});
  gf_lds_st(addr + 1024, (gf_u32x4){a.w[4], a.w[5], a.w[6], a.w[7]});
}
GF_DEV Gf pm_ld(uint32_t addr) {
  const gf_u32x4 lo = gf_lds_ld(addr), hi = gf_lds_ld(addr + 1024);
  Gf r;
  r.w[0] = lo.x; r.w[1] = lo.y; r.w[2] = lo.z; r.w[3] = lo.w;
  r.w[4] = hi.x; r.w[5] = hi.y; r.w[6] = hi.z; r.w[7] = hi.w;
  return r;
}
GF_DEV Ld pm_frob(const Ld& p) {
  Ld r;
  r.X = gf_sqr(p.X);
  r.Y = gf_sqr(p.Y);
  r.Z = gf_sqr(p.Z);
  return r;
}

// m P for m = 1, 2, 3 from the affine P, projective: P itself, its doubling (ld_dbl with Z1 = 1: Z = x^2, X = x^4 + 1,
// Y = Z + X (y^2 + 1)), the doubling plus P.  m is the same in every lane.
template <class LT>
GF_DEV Ld pm_multiple(int m, const Aff& P, const LT& L) {
  Ld r = ld_from_aff(P);
  if (m >= 2) {
    r.Z = gf_sqr(P.x);
    r.X = gf_add(gf_sqr(r.Z), gf_one());
    r.Y = gf_add(r.Z, gf_mul(r.X, gf_add(gf_sqr(P.y), gf_one()), L));
    if (m == 3) ld_madd_distinct(r, P, L);
  }
  return r;
}

// W = 5 leaves room for two waves per CU whatever its registers, so it may use all of them; W = 3, 4 keep to two waves per SIMD
template <int W>
__global__ void __launch_bounds__(64, W == 5 ? 1 : 2)
k_points_mul(const uint32_t* scalars, uint32_t s_stride, const Aff* pts, const uint8_t* inf, size_t n, GfSqrTables T,
             Aff* out, uint8_t* out_inf, unsigned long long* __restrict__ summary) {
  using S = PmShape<W>;
  constexpr int NE = S::NE;
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);  // one wave per workgroup: lane_base = region + lane * 16
  const uint32_t tab_base = L.lane_base + S::TABLE_OFF, rec_base = L.lane_base + S::REC_OFF;
  const uint32_t lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * 64 + lane;
  const bool live = i < n;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = live ? scalars[i * s_stride + k] : 0u;
  const bool bad = live && !tau_scalar_is_canonical(s);
  {  // summary as k_points_check writes it: the lowest bad lane of a wave only
    const unsigned long long m = __ballot(bad);
    if (m && lane == (unsigned)__ffsll((long long)m) - 1) {
      atomicMin(summary, (unsigned long long)i);
      atomicAdd(summary + 1, (unsigned long long)__popcll(m));
    }
  }
  if (!live) return;
  Aff a;
  a.x = gf_zero();
  a.y = gf_zero();
  if (bad || (inf && inf[i])) {
    out[i] = a;
    out_inf[i] = 1;
    return;
  }
  const Aff P = pts[i];  // read before the store below: out may be pts

  // ---- table ----
  // Entry e >= 1 is |b| P + rel tau(|g| P) up to a sign applied once it is affine; the multiples are made again for every entry (2P is
  // one product) so that nothing but P -- read back from its own slot -- lives across the loop, which stays rolled: the descriptor is
  // the same in every lane.  Scratch region: Z_1 .. Z_(NE-1), then the prefix products Z_1 .. Z_e for e = 2 .. NE-2.
  // For P of prime order r, P != O, no two operands of an addition here coincide or are opposite, and none is O: an element c + d tau
  // of Z[tau] acts on E[r] as the scalar c + d lambda, and that scalar is 0 mod r only for elements of the ideal (delta), whose non-zero
  // members have norm >= r.  The sums and differences of the operands -- |b| +- |g| tau, and 2 +- 1 inside 3P = 2P + P -- are non-zero
  // elements of norm < 2^6, so they act as non-zero scalars: the additions without exceptional cases are enough.  (For a point
  // outside E[r] they compute some triple, a zero Z among them zeroes the shared inverse and with it the table, and the call's
  // result is as unspecified as for every affine entry.)
  pm_st(tab_base, P.x);
  pm_st(tab_base + 2048, P.y);
  if constexpr (NE > 1) {
    static_assert(pm_descs_ok(S::tab), "an entry the build cannot make from P, 2P and 3P");
    const PmDescs<W>& descs = PM_DESCS<W>;
#pragma unroll 1
    for (int e = 1; e < NE; ++e) {
      asm volatile("" ::: "memory");
      const PmDesc d = descs.d[e];
      Ld t, r;
      {
        Aff p0;
        p0.x = pm_ld(tab_base);
        p0.y = pm_ld(tab_base + 2048);
        if (d.rel_neg) p0.y = gf_add(p0.y, p0.x);
        t = pm_frob(pm_multiple(d.ag, p0, L));
      }
      asm volatile("" ::: "memory");  // P is read again rather than held across the first multiple
      {
        Aff p0;
        p0.x = pm_ld(tab_base);
        p0.y = pm_ld(tab_base + 2048);
        r = pm_multiple(d.ab, p0, L);
      }
      ld_add_distinct(r, t, L);
      pm_st(tab_base + (uint32_t)e * 4096, r.X);
      pm_st(tab_base + (uint32_t)e * 4096 + 2048, r.Y);
      pm_st(rec_base + (uint32_t)(e - 1) * 2048, r.Z);
    }
    Gf prod = pm_ld(rec_base);
#pragma unroll 1
    for (int e = 2; e < NE; ++e) {
      prod = gf_mul(prod, pm_ld(rec_base + (uint32_t)(e - 1) * 2048), L);
      if (e <= NE - 2) pm_st(rec_base + (uint32_t)(NE - 1 + e - 2) * 2048, prod);
    }
    Gf inv = gf_inv_fast(prod, T, L);  // 1 / (Z_1 ... Z_(NE-1))
#pragma unroll 1
    for (int e = NE - 1; e >= 1; --e) {
      Gf zi = inv;
      if (e > 1) {
        const Gf pre = pm_ld(rec_base + (uint32_t)(e == 2 ? 0 : NE - 1 + e - 3) * 2048);
        const Gf ze = pm_ld(rec_base + (uint32_t)(e - 1) * 2048);
        gf_mul2(pre, ze, inv, L, zi, inv);  // 1 / Z_e, and the inverse of the product below it
      }
      const uint32_t slot = tab_base + (uint32_t)e * 4096;
      const Gf x = gf_mul(pm_ld(slot), zi, L);
      Gf y = gf_mul(pm_ld(slot + 2048), gf_sqr(zi), L);
      if (descs.d[e].neg) y = gf_add(y, x);
      pm_st(slot, x);
      pm_st(slot + 2048, y);
    }
    asm volatile("" ::: "memory");
  }

  // ---- recode: record k = position | entry << 8 | negative << 11, low digits first ----
  typedef __attribute__((address_space(3))) uint16_t lds_u16;
  const uint32_t rec16 = L.lane_base - lane * 16 + S::REC_OFF + lane * 2;  // row k at + 128 k
  int cnt = 0;
  {
    uint32_t r0[5], r1[5];
    uint32_t sc[8];  // read again: the limbs are not held across the table build
#pragma unroll
    for (int k = 0; k < 8; ++k) sc[k] = scalars[i * s_stride + k];
    tau_partial_reduce(sc, r0, r1);
#pragma unroll 1
    for (int j = 0; j < S::DIGITS; ++j) {
      const int d = tnaf_step<W>(r0, r1);
      if (d != 0 && cnt < S::MAXREC) {
        const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
        *(lds_u16*)(rec16 + (uint32_t)cnt * 128) = (uint16_t)((uint32_t)j | (ad >> 1) << 8 | (d < 0 ? 1u << 11 : 0u));
        ++cnt;
      }
    }
  }

  // ---- left to right over the non-zero digits ----
  Ld acc = ld_infinity();
#pragma unroll 1
  for (int k = cnt - 1; k >= 0; --k) {
    const uint32_t rec = *(const lds_u16*)(rec16 + (uint32_t)k * 128);
    const uint32_t below = k > 0 ? (uint32_t)*(const lds_u16*)(rec16 + (uint32_t)(k - 1) * 128) & 0xffu : 0u;
    const uint32_t slot = tab_base + ((rec >> 8) & 7u) * 4096;
    Aff q;
    q.x = pm_ld(slot);
    q.y = pm_ld(slot + 2048);
    if (rec & (1u << 11)) q.y = gf_add(q.y, q.x);
    madd_complete(acc, q, L);
#pragma unroll 1
    for (uint32_t t = (rec & 0xffu) - below; t > 0; --t) acc = pm_frob(acc);
  }

  const bool fin = !ld_is_inf(acc);
  if (fin) {
    const Gf zi = gf_inv_fast(acc.Z, T, L);
    a.x = gf_mul(acc.X, zi, L);
    a.y = gf_mul(acc.Y, gf_sqr(zi), L);
  }
  out[i] = a;
  out_inf[i] = fin ? 0 : 1;
}

// the recoder alone (dvp_debug_recode_tnaf): digits[i * DIGITS + j]
template <int W>
__global__ void __launch_bounds__(256) k_recode_tnaf(const uint32_t* __restrict__ scalars, size_t n, int8_t* __restrict__ digits) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8], r0[5], r1[5];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = scalars[i * 8 + k];
  tau_partial_reduce(s, r0, r1);
  int8_t* o = digits + i * (size_t)PmShape<W>::DIGITS;
#pragma unroll 1
  for (int j = 0; j < PmShape<W>::DIGITS; ++j) o[j] = (int8_t)tnaf_step<W>(r0, r1);
}

static int points_mul_w() {
  const long long w = tune().points_mul_w;
  return (w >= 3 && w <= 5) ? (int)w : PM_DEFAULT_W;
}

template <int W>
static void pm_launch(const void* d_scalars, uint32_t stride, const void* d_xy, const void* d_inf, size_t n, const GfSqrTables& T, void* d_out_xy,
                      void* d_out_inf, void* d_summary, hipStream_t st) {
  static_assert(PmShape<W>::LDS_BYTES <= 64 * 1024, "dynamic LDS of one workgroup");
  DVP_LAUNCH(k_points_mul<W>, dim3(cdiv(n, 64)), dim3(64), PmShape<W>::LDS_BYTES, st, (const uint32_t*)d_scalars, stride, (const Aff*)d_xy,
                     (const uint8_t*)d_inf, n, T, (Aff*)d_out_xy, (uint8_t*)d_out_inf, (unsigned long long*)d_summary);
}

// enqueue only: d_summary (16 bytes) is reset here, then the kernel fills it
int points_mul_dev(const void* d_scalars, size_t n_scalars, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy, void* d_out_inf,
                   void* d_summary, hipStream_t st) {
  DVP_TRY(summary_reset(d_summary, st));
  if (!n) return DVP_OK;
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  const uint32_t stride = n_scalars == 1 ? 0u : 8u;
  switch (points_mul_w()) {
    case 3: pm_launch<3>(d_scalars, stride, d_xy, d_inf, n, T, d_out_xy, d_out_inf, d_summary, st); break;
    case 5: pm_launch<5>(d_scalars, stride, d_xy, d_inf, n, T, d_out_xy, d_out_inf, d_summary, st); break;
    default: pm_launch<4>(d_scalars, stride, d_xy, d_inf, n, T, d_out_xy, d_out_inf, d_summary, st); break;
  }
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}


}  // namespace dvp

using namespace dvp;

extern "C" int dvp_points_mul_dev(const void* d_scalars, size_t n_scalars, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy,
                                  void* d_out_inf, void* d_summary, void* stream) {
  if (!d_summary) return DVP_EINVAL;
  if (n && (!d_scalars || !d_xy || !d_out_xy || !d_out_inf || (n_scalars != 1 && n_scalars != n))) return DVP_EINVAL;
  return points_mul_dev(d_scalars, n_scalars, d_xy, d_inf, n, d_out_xy, d_out_inf, d_summary, (hipStream_t)stream);
}

extern "C" int dvp_points_mul(const uint64_t* scalars, size_t n_scalars, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_xy,
                              uint8_t* out_inf) {
  if (!n) return DVP_OK;
  if (!scalars || !xy || !out_xy || !out_inf || (n_scalars != 1 && n_scalars != n)) return DVP_EINVAL;
  DevBuf ds, dp, di, doi, dsum;
  DVP_TRY(dp.up(xy, n * 64));
  DVP_TRY(di.up_opt(inf, n));
  DVP_TRY(doi.alloc(n));
  DVP_TRY(dsum.alloc(16));
  DVP_TRY(points_check_strict(dp.p, di.p, n, 0));  // the points before the scalars, which go up only once both have passed
  DVP_TRY(scalars_in_range(scalars, n_scalars));
  DVP_TRY(ds.up(scalars, n_scalars * 32));
  DVP_TRY(points_mul_dev(ds.p, n_scalars, dp.p, di.p, n, dp.p, doi.p, dsum.p, 0));  // in place
  DVP_TRY(dp.down(out_xy, n * 64));
  return doi.down(out_inf, n);
}

extern "C" int dvp_points_mul_xsk233(const uint8_t* scalars, size_t n_scalars, const uint8_t* enc, size_t n, uint8_t* out_enc) {
  if (!n) return DVP_OK;
  if (!scalars || !enc || !out_enc || (n_scalars != 1 && n_scalars != n)) return DVP_EINVAL;
  DevBuf ds, dp, di, doi, de, dsum;
  DVP_TRY(dp.alloc(n * 64));
  DVP_TRY(di.alloc(n));
  DVP_TRY(doi.alloc(n));
  DVP_TRY(de.up(enc, n * 30));
  DVP_TRY(dsum.alloc(16));
  DVP_TRY(decode_dev(de.as<uint8_t>(), n, dp.as<Aff>(), di.as<uint8_t>(), 0));
  // 32 little-endian bytes are the four limbs on the hosts this library runs on; the check reads each through a copy, whatever the alignment
  DVP_TRY(scalars_in_range(scalars, n_scalars));
  DVP_TRY(ds.up(scalars, n_scalars * 32));
  DVP_TRY(points_mul_dev(ds.p, n_scalars, dp.p, di.p, n, dp.p, doi.p, dsum.p, 0));
  DVP_TRY(encode_dev(dp.as<Aff>(), doi.as<uint8_t>(), n, de.as<uint8_t>(), 0));
  return de.down(out_enc, n * 30);
}

// digits[i * *n_digits + j] = the signed digit of scalar i at position j; alpha[2 e] + alpha[2 e + 1] tau = alpha_(2e+1)
extern "C" int dvp_debug_recode_tnaf(const uint64_t* scalars, size_t n, int w, int8_t* digits, int* n_digits, int32_t* alpha) {
  if (!n_digits || w < 3 || w > 5 || n > (1u << 24)) return DVP_EINVAL;
  const TnafTable t = w == 3 ? TnafDigits<3>::table : (w == 4 ? TnafDigits<4>::table : TnafDigits<5>::table);
  const int nd = w == 3 ? TnafDigits<3>::value : (w == 4 ? TnafDigits<4>::value : TnafDigits<5>::value);
  *n_digits = nd;
  if (alpha)
    for (int e = 0; e < t.entries; ++e) {
      alpha[2 * e] = t.beta[e];
      alpha[2 * e + 1] = t.gamma[e];
    }
  if (!digits) return DVP_OK;
  if (!scalars || !n) return DVP_EINVAL;
  DVP_TRY(scalars_in_range(scalars, n));
  DevBuf ds, dd;
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(dd.alloc(n * (size_t)nd));
  const dim3 grid(cdiv(n, 256)), block(256);
  if (w == 3) DVP_LAUNCH(k_recode_tnaf<3>, grid, block, 0, 0, ds.as<uint32_t>(), n, dd.as<int8_t>());
  else if (w == 4) DVP_LAUNCH(k_recode_tnaf<4>, grid, block, 0, 0, ds.as<uint32_t>(), n, dd.as<int8_t>());
  else DVP_LAUNCH(k_recode_tnaf<5>, grid, block, 0, 0, ds.as<uint32_t>(), n, dd.as<int8_t>());
  DVP_HIP(hipGetLastError());
  return dd.down(digits, n * (size_t)nd);
}
