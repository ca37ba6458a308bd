// The prover's stage kernels and their device helpers: domain tables, R1CS rows, quotient, the challenge phase's vector stages (whole
// and index-sharded), the device transcript.  Part of prove.hip's translation unit: prove.hip includes it, and its kernels are launched
// and counted as prove.hip's (see the map at the top of prove.hip).
#pragma once
#include "blake3_dev.cuh"
#include "common.h"
#include "ecfft_internal.h"
#include "fr_block.cuh"  // block_sum256

namespace dvp {

// ---- domain tables from the isogeny chain ---------------------------------------------------------
// For S = even leaves (D) of the 2m-leaf tree, Z_S = U - c0 V with (U,V) the projective image under
// the first kk = log2(m) isogenies.  Forward-mode derivative gives Z_S'(s_i) for the barycentric
// weights; Z_S on the other half gives z_vals2inv.
//   bar_w[i]   = 1 / Z_S'(S[i])          (Montgomery)
//   zinv_o[i]  = 1 / Z_S(other[i])       (Montgomery)
// which = 0: S = even leaves, other = odd leaves; which = 1: mirrored.
__global__ void __launch_bounds__(256)
k_domain_tables(const Fr* __restrict__ L0, uint32_t m, const Fr* __restrict__ x0s, const Fr* __restrict__ ts, int kk,
                const Fr* __restrict__ ctop /* layer kk: 2 leaves */, int which, Fr* __restrict__ bar_w, Fr* __restrict__ zinv_o) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Fr c0 = ctop[which];
  Fr s = L0[2 * (size_t)i + which];
  Fr o = L0[2 * (size_t)i + 1 - which];
  zinv_o[i] = fr_inv(vanish_chain(o, x0s, ts, kk, c0));
  // derivative at s
  Fr u = s, v = fr_one_mont(), du = fr_one_mont(), dv = fr_zero();
  for (int d = 0; d < kk; ++d) {
    Fr x0 = x0s[d], t = ts[d];
    Fr uv = fr_mul(u, v), vv = fr_sqr(v);
    Fr duv = fr_add(fr_mul(du, v), fr_mul(u, dv));  // (uv)'
    Fr dvv = fr_dbl(fr_mul(v, dv));                 // (v^2)'
    Fr nu = fr_add(fr_sub(fr_sqr(u), fr_mul(x0, uv)), fr_mul(t, vv));
    Fr nv = fr_sub(uv, fr_mul(x0, vv));
    Fr ndu = fr_add(fr_sub(fr_dbl(fr_mul(u, du)), fr_mul(x0, duv)), fr_mul(t, dvv));
    Fr ndv = fr_sub(duv, fr_mul(x0, dvv));
    u = nu; v = nv; du = ndu; dv = ndv;
  }
  bar_w[i] = fr_inv(fr_sub(du, fr_mul(c0, dv)));
}

// contiguous Montgomery copies of D and D'
__global__ void __launch_bounds__(256) k_split_domains(const Fr* __restrict__ L0, uint32_t m, Fr* __restrict__ d, Fr* __restrict__ d2) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  d[i] = L0[2 * (size_t)i];
  d2[i] = L0[2 * (size_t)i + 1];
}

// ---- stage kernels ---------------------------------------------------------------------------------
struct Csr {
  const uint32_t* row_ptr;  // n_rows + 1
  const uint32_t* wire;
  const uint32_t* coeff;
  uint32_t n_rows;
};

__device__ __forceinline__ Fr csr_row(const Csr& m, uint32_t row, const Fr* __restrict__ coeffs_m, const Fr* __restrict__ w) {
  Fr acc = fr_zero();
  if (row >= m.n_rows) return acc;
  for (uint32_t k = m.row_ptr[row]; k < m.row_ptr[row + 1]; ++k)
    acc = fr_add(acc, fr_mul(coeffs_m[m.coeff[k]], w[m.wire[k]]));  // eval_row, src/gnark_r1cs.rs:273-280
  return acc;
}

// E = [a | b | c' | i] (4 x m, canonical).  c' = C w - i(d), i(d) = sum_j pub_j d^j (src/gnark_r1cs.rs:333-399)
__global__ void __launch_bounds__(256)
k_r1cs_eval(Csr A, Csr B, Csr C, const Fr* __restrict__ coeffs_m, const Fr* __restrict__ w, const Fr* __restrict__ dom_m,
            uint32_t npub, uint32_t m, Fr* __restrict__ E, unsigned long long* __restrict__ unsat) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Fr a = csr_row(A, i, coeffs_m, w), b = csr_row(B, i, coeffs_m, w), cw = csr_row(C, i, coeffs_m, w);
  Fr d = dom_m[i];
  Fr iv = fr_zero();
  for (int j = (int)npub - 1; j >= 0; --j) iv = fr_add(fr_mul(d, iv), w[1 + j]);  // Horner, canonical
  // a*b == c' + i  <=>  a*b == C w      (assert_eq!, src/proving.rs:389-395)
  if (!fr_eq(fr_mul(fr_to_mont(a), b), cw)) atomicMin(unsat, (unsigned long long)i);
  E[i] = a;
  E[(size_t)m + i] = b;
  E[2 * (size_t)m + i] = fr_sub(cw, iv);
  E[3 * (size_t)m + i] = iv;
}

// r2 = a2 b2 - i2 ; q2 = (r2 - c2) * z2inv        (src/proving.rs:492-508)
// HORNER: i has only npub coefficients, so for a short public input i2 = i(d'_i) is evaluated directly (the same
// canonical value the extend of i's evaluations yields, at npub products instead of an ECFFT pass).  Rule: HORNER only with
// npub <= m.  Beyond that i(X) has degree >= m, the extend of its m evaluations on D is another polynomial (the interpolant of
// degree < m), and the reference proves with that one (src/proving.rs:369-376, 415): prover_n_ext then takes the fourth extend.
template <bool HORNER>
__global__ void __launch_bounds__(256)
k_quotient(Fr* __restrict__ E2, const Fr* __restrict__ z2inv_m, uint32_t m, const Fr* __restrict__ w, const Fr* __restrict__ dom2_m,
           uint32_t npub, Fr* __restrict__ r2, Fr* __restrict__ q2) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Fr a = E2[i], b = E2[(size_t)m + i], c = E2[2 * (size_t)m + i], iv;
  if (HORNER) {
    Fr d = dom2_m[i];
    iv = fr_zero();
    for (int j = (int)npub - 1; j >= 0; --j) iv = fr_add(fr_mul(d, iv), w[1 + j]);
    E2[3 * (size_t)m + i] = iv;
  } else {
    iv = E2[3 * (size_t)m + i];
  }
  Fr r = fr_sub(fr_mul(fr_to_mont(a), b), iv);
  r2[i] = r;
  q2[i] = fr_mul(z2inv_m[i], fr_sub(r, c));
}

// den[i] = d_i - alpha, den2[i] = d'_i - alpha (canonical); flags alpha in D u D' (src/proving.rs:548-556)
__global__ void __launch_bounds__(256)
k_alpha_denoms(const Fr* __restrict__ d_m, const Fr* __restrict__ d2_m, const Fr* __restrict__ alpha_m_p, uint32_t m, Fr* __restrict__ den,
               Fr* __restrict__ den2, unsigned long long* __restrict__ hit) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Fr alpha_m = *alpha_m_p;  // from the host (dvp_prove_challenge) or from k_transcript, in the prover's own block
  Fr x = fr_sub(d_m[i], alpha_m), y = fr_sub(d2_m[i], alpha_m);
  if (fr_is_zero(x) || fr_is_zero(y)) atomicMin(hit, (unsigned long long)i);
  den[i] = fr_from_mont(x);
  den2[i] = fr_from_mont(y);
}

// out[0..2] = a0, b0, i0 (canonical); out[3] = r0 = a0 b0 - i0, from the three Montgomery values
__device__ __forceinline__ void bary3_close(const Fr& a0_m, const Fr& b0_m, const Fr& i0_m, Fr* __restrict__ out) {
  out[0] = fr_from_mont(a0_m);
  out[1] = fr_from_mont(b0_m);
  out[2] = fr_from_mont(i0_m);
  out[3] = fr_from_mont(fr_sub(fr_mul(a0_m, b0_m), i0_m));
}

// partial sums of  y_i * w_i * dinv_i  for y in {a, b, i} over i in [lo, hi)   (dinv = 1/(d_i - alpha), canonical): the whole of D
// in one prover, a rank's slice in the index-sharded challenge phase
__global__ void __launch_bounds__(256)
k_bary3_partial_range(const Fr* __restrict__ E, const Fr* __restrict__ barw_m, const Fr* __restrict__ dinv, uint32_t m, uint32_t lo,
                      uint32_t hi, Fr* __restrict__ partial /* [3][nb] Montgomery */) {
  __shared__ Fr sh[256];
  Fr s[3] = {fr_zero(), fr_zero(), fr_zero()};
  // four products per element (round 6; eight before): barw (Montgomery) times the canonical dinv is the canonical product k, and
  // fr_mul(k, y) of two canonical values is k y / R -- the sums carry one factor 1 / R, which the block's ONE thread that writes
  // the partial takes back out (two products by R^2: x / R -> x -> x R, the Montgomery partial k_bary3_final expects)
  for (uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += gridDim.x * blockDim.x) {
    Fr k = fr_mul(barw_m[i], dinv[i]);
    s[0] = fr_add(s[0], fr_mul(k, E[i]));
    s[1] = fr_add(s[1], fr_mul(k, E[(size_t)m + i]));
    s[2] = fr_add(s[2], fr_mul(k, E[3 * (size_t)m + i]));
  }
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const Fr t = block_sum256(s[v], sh);
    if (threadIdx.x == 0) partial[(size_t)v * gridDim.x + blockIdx.x] = fr_mul(fr_mul(t, fr_r2()), fr_r2());
  }
}
// P(alpha) = -Z(alpha) * sum y w / (d - alpha): block partials -> a0 b0 i0 r0 (bary3_close)
__global__ void __launch_bounds__(256) k_bary3_final(const Fr* __restrict__ partial, uint32_t nb, const Fr* __restrict__ neg_z_alpha_m_p, Fr* __restrict__ out) {
  __shared__ Fr sh[256];
  Fr res[3];
  const Fr neg_z_alpha_m = *neg_z_alpha_m_p;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    Fr s = fr_zero();
    for (uint32_t i = threadIdx.x; i < nb; i += 256) s = fr_add(s, partial[(size_t)v * nb + i]);
    res[v] = fr_mul(block_sum256(s, sh), neg_z_alpha_m);  // Montgomery
  }
  if (threadIdx.x == 0) bary3_close(res[0], res[1], res[2], out);
}

// S = [k_a | k_b | k_r] with k_r interleaved [D_i, D'_i]   (src/proving.rs:619-654)
__global__ void __launch_bounds__(256)
k_kscalars(const Fr* __restrict__ E, const Fr* __restrict__ r2, const Fr* __restrict__ dinv, const Fr* __restrict__ dinv2,
           const Fr* __restrict__ abir0 /* a0,b0,i0,r0 canonical */, uint32_t m, Fr* __restrict__ S) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Fr a0 = abir0[0], b0 = abir0[1], r0 = abir0[3];
  Fr a = E[i], b = E[(size_t)m + i], iv = E[3 * (size_t)m + i];
  Fr di = fr_to_mont(dinv[i]), di2 = fr_to_mont(dinv2[i]);
  S[i] = fr_mul(di, fr_sub(a, a0));
  S[(size_t)m + i] = fr_mul(di, fr_sub(b, b0));
  Fr r = fr_sub(fr_mul(fr_to_mont(a), b), iv);
  S[2 * (size_t)m + 2 * (size_t)i] = fr_mul(di, fr_sub(r, r0));
  S[2 * (size_t)m + 2 * (size_t)i + 1] = fr_mul(di2, fr_sub(r2[i], r0));
}

// ---- index-sharded challenge phase (pointwise / barycentric row): every stage below works on a slice ----
// k_alpha_denoms / _range and k_kscalars / _range stay two kernels each: the first of a pair reads alpha through a pointer (the device
// transcript writes it) and serves both domains, resp. three outputs, per thread; the _range one takes alpha by value and is indexed by
// ONE domain, resp. by output.  Merged, the default path would launch more or do other work per thread.
// den[i] = dom[i] - alpha for i in [lo, hi) of ONE domain (canonical); flags alpha in that slice of the domain
__global__ void __launch_bounds__(256)
k_alpha_denoms_range(const Fr* __restrict__ dom_m, Fr alpha_m, uint32_t lo, uint32_t hi, Fr* __restrict__ den, unsigned long long* __restrict__ hit) {
  uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hi) return;
  Fr x = fr_sub(dom_m[i], alpha_m);
  if (fr_is_zero(x)) atomicMin(hit, (unsigned long long)i);
  den[i] = fr_from_mont(x);
}
// block partials -> one 128-byte record: 3 Montgomery sums (this rank's share of sum y w / (d - alpha), y in {a, b, i}),
// then the rank's alpha-in-domain flag
__global__ void __launch_bounds__(256)
k_bary3_record(const Fr* __restrict__ partial, uint32_t nb, const unsigned long long* __restrict__ hit, Fr* __restrict__ rec) {
  __shared__ Fr sh[256];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    Fr s = fr_zero();
    for (uint32_t i = threadIdx.x; i < nb; i += 256) s = fr_add(s, partial[(size_t)v * nb + i]);
    const Fr t = block_sum256(s, sh);
    if (threadIdx.x == 0) rec[v] = t;
  }
  if (threadIdx.x == 0) {
    Fr f = fr_zero();
    const unsigned long long h = *hit;
    f.v[0] = (uint32_t)h;
    f.v[1] = (uint32_t)(h >> 32);
    rec[3] = f;
  }
}
// n gathered records -> a0, b0, i0, r0 (what k_bary3_final does with block partials) and the combined flag
__global__ void __launch_bounds__(64)
k_bary3_from_records(const Fr* __restrict__ recs /* n x 4 Fr */, uint32_t n, Fr neg_z_alpha_m, Fr* __restrict__ out,
                     unsigned long long* __restrict__ hit) {
  if (threadIdx.x != 0) return;
  Fr res[3];
  unsigned long long h = ~0ull;
#pragma unroll
  for (int v = 0; v < 3; ++v) {  // (unrolled: see block_sum256)
    Fr s = fr_zero();
    for (uint32_t r = 0; r < n; ++r) s = fr_add(s, recs[(size_t)r * 4 + v]);
    res[v] = fr_mul(s, neg_z_alpha_m);
  }
  for (uint32_t r = 0; r < n; ++r) {
    const Fr& f = recs[(size_t)r * 4 + 3];
    h = min(h, (unsigned long long)f.v[0] | ((unsigned long long)f.v[1] << 32));
  }
  bary3_close(res[0], res[1], res[2], out);
  *hit = h;
}
// S[k] for k in [k_lo, k_hi) of S = [k_a | k_b | k_r] (k_kscalars restricted to a range of the OUTPUT index)
__global__ void __launch_bounds__(256)
k_kscalars_range(const Fr* __restrict__ E, const Fr* __restrict__ r2, const Fr* __restrict__ dinv, const Fr* __restrict__ dinv2,
                 const Fr* __restrict__ abir0, uint32_t m, size_t k_lo, size_t k_hi, Fr* __restrict__ S) {
  size_t k = k_lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= k_hi) return;
  if (k < m) {
    S[k] = fr_mul(fr_to_mont(dinv[k]), fr_sub(E[k], abir0[0]));
  } else if (k < 2 * (size_t)m) {
    size_t i = k - m;
    S[k] = fr_mul(fr_to_mont(dinv[i]), fr_sub(E[(size_t)m + i], abir0[1]));
  } else {
    size_t j = k - 2 * (size_t)m, i = j >> 1;
    Fr r0 = abir0[3];
    if (j & 1) {
      S[k] = fr_mul(fr_to_mont(dinv2[i]), fr_sub(r2[i], r0));
    } else {
      Fr r = fr_sub(fr_mul(fr_to_mont(E[i]), E[(size_t)m + i]), E[3 * (size_t)m + i]);
      S[k] = fr_mul(fr_to_mont(dinv[i]), fr_sub(r, r0));
    }
  }
}

// ---- the Fiat-Shamir transcript on the device (round 5) ----------------------------------------------------------------
// Transcript::output (src/proving.rs:164-197) needs four single-chunk BLAKE3 hashes once commit_p exists -- H(commit_p),
// H(public inputs as 29-byte LE), H(H_wc || H_pi), H(H_ct || H_rt); H_ct = H(srs_hash || circuit_hash) is a value the host passes in (dvp_prover::h_ct) --
// and alpha is the result with its top four bytes cleared (:192).  One lane of one wave does that right behind the commitment MSM's
// tail kernel, so dvp_prove_dev has no host round trip between its two MSMs (the host is already enqueueing the second MSM's sort while
// the first one's rounds run).  Written from the BLAKE3 specification like blake3.h (the host flavour, which the phased entries and
// n_public > 35 keep using); the two are compared in tests/ (dvp_debug_transcript_dev).  The
// device BLAKE3 itself (b3d) lives in blake3_dev.cuh, shared with verify.hip.
constexpr uint32_t TRANSCRIPT_DEV_MAX_PUB = 35;  // 35 x 29 bytes = 1015 <= one 1024-byte chunk

// alpha from (commit_p, public inputs), both resident: enc30 = the commitment's 30 bytes (16-byte aligned, the two bytes behind them
// belong to the next encoding), pub = n_pub canonical Fr.  Writes alpha (canonical) and alpha (Montgomery).
__global__ void __launch_bounds__(64) k_transcript(const uint32_t* __restrict__ enc30, const Fr* __restrict__ pub, uint32_t npub, b3d::Words8 h_ct,
                                                   Fr* __restrict__ alpha_canon, Fr* __restrict__ alpha_m) {
  __shared__ uint32_t msg[256];
  for (uint32_t i = threadIdx.x; i < 256; i += 64) msg[i] = 0;
  __syncthreads();
  const uint32_t len = 29u * npub;  // <= 1015
  uint8_t* mb = (uint8_t*)msg;
  for (uint32_t t = threadIdx.x; t < len; t += 64) {
    const uint32_t j = t / 29u, b = t - 29u * j;
    mb[t] = ((const uint8_t*)(pub + j))[b];  // 29-byte LE of a canonical Fr (src/proving.rs:147-150)
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t blk[16], h_wc[8], h_pi[8], h_rt[8], out[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) blk[i] = i < 8 ? enc30[i] : 0u;
  blk[7] &= 0xffffu;  // 30 bytes
  b3d::hash_chunk(blk, 30, h_wc);
  b3d::hash_chunk(msg, len, h_pi);
#pragma unroll
  for (int i = 0; i < 8; ++i) { blk[i] = h_wc[i]; blk[8 + i] = h_pi[i]; }
  b3d::hash_chunk(blk, 64, h_rt);
#pragma unroll
  for (int i = 0; i < 8; ++i) { blk[i] = h_ct.w[i]; blk[8 + i] = h_rt[i]; }
  b3d::hash_chunk(blk, 64, out);
  Fr a;
#pragma unroll
  for (int i = 0; i < 7; ++i) a.v[i] = out[i];
  a.v[7] = 0;  // 224-bit challenge: the top four bytes cleared (src/proving.rs:192), always < p
  *alpha_canon = a;
  *alpha_m = fr_to_mont(a);
}
// -Z_D(alpha) from the isogeny chain (what host_vanish computes on the host): one lane, ~7 log2(m) dependent products -- run on the
// prover's side stream beside the denominators / batch inversion / barycentric partial sums, which do not need it
__global__ void __launch_bounds__(64) k_zalpha(const Fr* __restrict__ alpha_m, const Fr* __restrict__ x0s, const Fr* __restrict__ ts, int kk,
                                               const Fr* __restrict__ ctop, Fr* __restrict__ neg_z_alpha_m) {
  if (threadIdx.x != 0) return;
  *neg_z_alpha_m = fr_neg(vanish_chain(*alpha_m, x0s, ts, kk, ctop[0]));
}

__global__ void __launch_bounds__(256) k_to_mont_vec(const Fr* __restrict__ in, Fr* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fr_to_mont(in[i]);
}
__global__ void __launch_bounds__(256) k_from_mont_vec(const Fr* __restrict__ in, Fr* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fr_from_mont(in[i]);
}

}  // namespace dvp
