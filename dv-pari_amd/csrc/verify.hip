// The designated verifier's check, SRS::verify (src/srs.rs:374-428), for a batch of proofs against one trapdoor: one lane per
// proof, ONE launch per batch (k_verify) once the generator table exists.
//
//   CurvePoint::from_bytes of commit_p / kzg_k   src/srs.rs:380-382       -> codec_decode (codec.cuh, shared with k_decode)
//   Transcript (empty SRS / circuit, pub, P)     src/srs.rs:384-410       -> b3d (blake3_dev.cuh, shared with k_transcript)
//   evaluate_monomial_basis_poly                 src/gnark_r1cs.rs:391-399 -> Horner in Montgomery Fr
//   FrBits::to_fr of a0 / b0                     src/curve.rs:43-59       -> fr_below_p
//   multi_scalar_mul(&[v0, u0], &[K, G]) == P    src/srs.rs:418-424       -> tau-adic v0 K + fixed-base u0 G, compared with P
//
// Per lane: v0 K runs right to left over the tau-adic digits of v0 (tau.cuh: the partial reduction and sixteen digits per step,
// as the one-shot MSM recodes), with the running point tau^i(K) kept AFFINE -- a Frobenius step is two squarings -- and added into
// a Lopez-Dahab accumulator by the complete mixed addition (ld_madd_ip: P = Q, P = -Q and the neutral element on either side, so
// adversarial K and P cannot trip it).  u0 G continues in the same accumulator through the process-wide generator table
// (gen_table: 15 windows of 16 digits, the 15 mixed additions of k_mulgen).  The sum is compared with P by cross-multiplication:
// X == x(P) Z and Y == y(P) Z^2, no inversion.
//
// Public inputs: n_public <= 35 is one BLAKE3 chunk; larger counts are hashed multi-chunk on the device, per lane, with the
// chaining values of complete subtrees kept in registers (VERIFY_B3_LEVELS levels: up to 2^8 chunks = DVP_VERIFY_MAX_PUBLIC
// public inputs).  The 30 bytes of commit_p are hashed as they arrive: a valid encoding is the unique encoding of the point it
// decodes to (codec_decode), so they equal witness_commitment_hash's re-encoding, and an invalid one rejects the proof anyway.
//
// dvp_verify_batch_rlc*: the same verdicts through one random-linear-combination MSM of the whole batch, with k_verify<true> as the
// fallback when that MSM is not O (the section "batch check by one random linear combination" below).
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "blake3.h"
#include "blake3_dev.cuh"
#include "codec.cuh"
#include "common.h"
#include "fr.cuh"
#include "fr_block.cuh"
#include "host_api.h"
#include "k233.cuh"
#include "tau.cuh"
#include "verify_front.cuh"

namespace dvp {

// VerifyConsts, fr_below_p, load29, pub_digest, verify_decode and verify_scalars are verify_front.cuh (simulate.hip uses them too)

// one wave per SIMD: the 256 architectural VGPRs plus accumulation registers for what does not fit (no scratch); at two waves per
// SIMD the tau-adic loop spills ~300 B per lane to scratch.  GATED (the fallback of dvp_verify_batch_rlc*): the launch is always
// enqueued and ends at once when *gate != 0, i.e. when the combined check held or no proof was well formed.
template <bool GATED>
__global__ void __launch_bounds__(256, 1)
k_verify(const uint8_t* __restrict__ proofs, size_t n, const Fr* __restrict__ pub, uint32_t npub, VerifyConsts K, const Aff* __restrict__ tab,
         GfSqrTables T, int rule, uint8_t* __restrict__ verdicts, const uint32_t* __restrict__ gate) {
  if (GATED && *gate) return;
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* pr = proofs + 118 * i;
  const Fr* pi = pub + (size_t)npub * i;
  uint32_t bad = 0;
  Aff P, Kp;
  bool p_inf, k_inf;
  if (!codec_decode(pr, rule, T, L, P, p_inf)) bad |= DVP_VERIFY_BAD_COMMIT_P;
  if (!codec_decode(pr + 30, rule, T, L, Kp, k_inf)) bad |= DVP_VERIFY_BAD_KZG_K;
  const Fr a0 = load29(pr + 60), b0 = load29(pr + 89);
  if (!fr_below_p(a0)) bad |= DVP_VERIFY_BAD_A0;
  if (!fr_below_p(b0)) bad |= DVP_VERIFY_BAD_B0;
#pragma unroll 1
  for (uint32_t j = 0; j < npub; ++j)
    if (!fr_below_p(pi[j])) bad |= DVP_VERIFY_BAD_PUBLIC;
  if (bad) {
    verdicts[i] = (uint8_t)bad;
    return;
  }
  // alpha = Transcript::output: H(H_ct || H(H(commit_p) || H(pub))), top four bytes cleared (src/proving.rs:164-197)
  Fr alpha;
  {
    uint32_t blk[16], h_wc[8], h_pi[8], h_rt[8], out[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) blk[k] = 0;
#pragma unroll
    for (int b = 0; b < 30; ++b) blk[b >> 2] |= (uint32_t)pr[b] << (8 * (b & 3));
    b3d::hash_chunk(blk, 30, h_wc);
    pub_digest((const uint8_t*)pi, npub, h_pi);
#pragma unroll
    for (int k = 0; k < 8; ++k) { blk[k] = h_wc[k]; blk[8 + k] = h_pi[k]; }
    b3d::hash_chunk(blk, 64, h_rt);
#pragma unroll
    for (int k = 0; k < 8; ++k) { blk[k] = K.h_ct.w[k]; blk[8 + k] = h_rt[k]; }
    b3d::hash_chunk(blk, 64, out);
#pragma unroll
    for (int k = 0; k < 7; ++k) alpha.v[k] = out[k];
    alpha.v[7] = 0;  // 224 bits, always < p
  }
  // scalars (canonical throughout: mont_mul(x, c R) = x c)
  const Fr alpha_m = fr_to_mont(alpha);
  Fr i0 = fr_zero();
#pragma unroll 1
  for (uint32_t j = npub; j-- > 0;) i0 = fr_add(fr_mul(i0, alpha_m), pi[j]);  // sum_j pub_j alpha^j by Horner
  const Fr r0 = fr_sub(fr_mul(a0, fr_to_mont(b0)), i0);
  const Fr u0 = fr_mul(fr_add(fr_add(a0, fr_mul(b0, K.delta_m)), fr_mul(r0, K.delta2_m)), K.eps_m);
  const Fr v0 = fr_mul(fr_sub(K.tau, alpha), K.eps_m);

  Ld acc = ld_infinity();
  uint32_t r0t[5], r1t[5];
  // v0 K: sum_i d_i tau^i(K), digits low to high, tau^i(K) affine
  if (!k_inf) {
    tau_partial_reduce(v0.v, r0t, r1t);
    Aff q = Kp;
#pragma unroll 1
    for (int s = 0; s < TAU_DIGITS / 16; ++s) {
      const uint32_t dw = tau_step16(r0t, r1t);
#pragma unroll 1
      for (int t = 0; t < 16; ++t) {
        if ((dw >> t) & 1u) madd_complete(acc, q, L);
        q.x = gf_sqr(q.x);
        q.y = gf_sqr(q.y);
      }
    }
  }
  // + u0 G through the generator table (k_mulgen's loop)
  tau_partial_reduce(u0.v, r0t, r1t);
#pragma unroll 1
  for (int w = 0; w < GEN_W; ++w) {
    const uint32_t d = tau_step16(r0t, r1t);
    if (d) madd_complete(acc, tab[((size_t)w << GEN_C) + d], L);
  }
  bool eq;
  if (ld_is_inf(acc) || p_inf) {
    eq = ld_is_inf(acc) && p_inf;
  } else {
    eq = gf_eq(acc.X, gf_mul(P.x, acc.Z, L)) && gf_eq(acc.Y, gf_mul(P.y, gf_sqr(acc.Z), L));
  }
  verdicts[i] = eq ? 0 : (uint8_t)DVP_VERIFY_EQUATION;
}

// ---- batch check by one random linear combination (dvp_verify_batch_rlc*) ------------------------------------------------------
// For n proofs against one trapdoor, every well-formed proof j (the set W) satisfies v0_j K_j + u0_j G - P_j = O when it is valid.
// With r_j = BLAKE3(key || LE64(j) || proof_j || H(pub_j))[0..16) | 2^127 the n checks become ONE MSM of 2n + 1 points:
//   sum_W (r_j v0_j) K_j + sum_W (p - r_j) P_j + (sum_W r_j u0_j) G == O.
// Layout of the MSM input: [K_0 .. K_{n-1} | P_0 .. P_{n-1} | G]; a proof outside W has zero scalars and infinity flags.
//   k_verify_rlc_prep   one lane per proof: the front half of k_verify, the coefficient, the bases, scalars and r_j u0_j
//   k_rlc_sum_blocks    block partials of sum r_j u0_j (and of |W|)
//   k_rlc_sum_final     one block: the G scalar, the G base (generator table, window 0, digit 1), |W|
//   msm_affine_dev      the one-shot MSM, deferred completion (its scalar-range word stays on the device)
//   k_rlc_check         report word and gate
//   k_verify<true>      the per-lane check over the whole batch, unless the gate says the combination held

// the 190-byte coefficient message, little-endian words: key[0..32) | LE64(j)[32..40) | proof[40..158) | H(pub)[158..190)
__device__ __forceinline__ uint32_t rlc_msg_byte(uint32_t off, const b3d::Words8& key, uint64_t j, const uint8_t* pr, const uint32_t h_pi[8]) {
  if (off < 32) return (key.w[off >> 2] >> (8 * (off & 3))) & 0xffu;
  if (off < 40) return (uint32_t)(j >> (8 * (off - 32))) & 0xffu;
  if (off < 158) return pr[off - 40];
  if (off < 190) return (h_pi[(off - 158) >> 2] >> (8 * ((off - 158) & 3))) & 0xffu;
  return 0;
}

// r_j: the first 16 digest bytes read little-endian, bit 127 set (nonzero, 127 random bits, < p)
__device__ __forceinline__ Fr rlc_coeff(const b3d::Words8& key, uint64_t j, const uint8_t* pr, const uint32_t h_pi[8]) {
  constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  constexpr uint32_t CHUNK_START = 1, CHUNK_END = 2, ROOT = 8;
  uint32_t cv[8], m[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) cv[i] = IV[i];
#pragma unroll
  for (uint32_t b = 0; b < 3; ++b) {  // one chunk of three blocks: 64 + 64 + 62 bytes
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      uint32_t w = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) w |= rlc_msg_byte(64 * b + 4 * k + q, key, j, pr, h_pi) << (8 * q);
      m[k] = w;
    }
    b3d::compress(cv, m, b == 2 ? 62u : 64u, b == 0 ? CHUNK_START : (b == 2 ? CHUNK_END | ROOT : 0u));
  }
  Fr r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.v[k] = cv[k];
  r.v[3] |= 0x80000000u;
#pragma unroll
  for (int k = 4; k < 8; ++k) r.v[k] = 0;
  return r;
}

// one lane per proof, no tau-adic chain: the decode's inversion and the transcript are the cost
__global__ void __launch_bounds__(256, 2)
k_verify_rlc_prep(const uint8_t* __restrict__ proofs, size_t n, const Fr* __restrict__ pub, uint32_t npub, VerifyConsts K, b3d::Words8 key,
                  GfSqrTables T, int rule, Fr* __restrict__ sc, Aff* __restrict__ bases, uint8_t* __restrict__ inf, Fr* __restrict__ ur,
                  uint8_t* __restrict__ verdicts) {
  extern __shared__ char lds_raw[];
  GfLdsK L = gf_ldsk_init(lds_raw);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* pr = proofs + 118 * i;
  const Fr* pi = pub + (size_t)npub * i;
  uint32_t bad;
  {
    Aff P, Kp;
    bool p_inf, k_inf;
    bad = verify_decode(pr, pi, npub, T, L, rule, P, p_inf, Kp, k_inf);
    bases[i] = Kp;  // stored now: the points are not held across the transcript
    bases[n + i] = P;
    inf[i] = (bad || k_inf) ? 1 : 0;
    inf[n + i] = (bad || p_inf) ? 1 : 0;
  }
  Fr sk = fr_zero(), sp = fr_zero(), su = fr_zero();
  if (!bad) {
    VerifyFront f;
    verify_scalars(pr, pi, npub, K, f);
    const Fr r = rlc_coeff(key, (uint64_t)i, pr, f.h_pi);
    const Fr r_m = fr_to_mont(r);
    sk = fr_mul(f.v0, r_m);
    sp = fr_sub(fr_zero(), r);  // p - r: r != 0
    su = fr_mul(f.u0, r_m);
  }
  sc[i] = sk;
  sc[n + i] = sp;
  ur[i] = su;
  verdicts[i] = (uint8_t)bad;
}

constexpr uint32_t RLC_SUM_TPB = 256;
constexpr uint32_t RLC_SUM_BLOCKS = 1024;  // level-1 blocks at most: level 2 is one block over their partials

// sum mod p of a block's values and count of its well-formed proofs; Fr addition is exact and the count is an integer, so the result
// does not depend on the order in which lanes or blocks run
static_assert(RLC_SUM_TPB == 256, "block_sum256");
__device__ __forceinline__ void rlc_block_sum(Fr s, uint32_t w, Fr* out, uint32_t* out_w) {
  __shared__ Fr ls[RLC_SUM_TPB];
  __shared__ uint32_t lw;
  if (threadIdx.x == 0) lw = 0;
  const Fr total = block_sum256(s, ls);  // its barriers put the zero before the additions
  atomicAdd(&lw, w);
  __syncthreads();
  if (threadIdx.x == 0) {
    *out = total;
    *out_w = lw;
  }
}

// level 1: block b sums lanes b, b + B, b + 2B, ... in strides of the whole grid
__global__ void __launch_bounds__(RLC_SUM_TPB)
k_rlc_sum_blocks(const Fr* __restrict__ ur, const uint8_t* __restrict__ verdicts, size_t n, Fr* __restrict__ part, uint32_t* __restrict__ part_w) {
  Fr s = fr_zero();
  uint32_t w = 0;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * RLC_SUM_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * RLC_SUM_TPB) {
    s = fr_add(s, ur[i]);
    w += verdicts[i] == 0 ? 1u : 0u;
  }
  rlc_block_sum(s, w, part + blockIdx.x, part_w + blockIdx.x);
}

// level 2 (one block): the G entry of the MSM -- scalar sum_W r_j u0_j, base G = tab[window 0, digit 1] -- and |W|
__global__ void __launch_bounds__(RLC_SUM_TPB)
k_rlc_sum_final(const Fr* __restrict__ part, const uint32_t* __restrict__ part_w, uint32_t nparts, const Aff* __restrict__ tab, Fr* __restrict__ g_sc,
                Aff* __restrict__ g_base, uint8_t* __restrict__ g_inf, uint32_t* __restrict__ n_w) {
  Fr s = fr_zero();
  uint32_t w = 0;
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < nparts; i += RLC_SUM_TPB) {
    s = fr_add(s, part[i]);
    w += part_w[i];
  }
  rlc_block_sum(s, w, g_sc, n_w);
  if (threadIdx.x == 0) {
    *g_base = tab[1];
    *g_inf = 0;
  }
}

// the MSM is O (and its scalars were in range): COMBINED; else FALLBACK.  No well-formed proof: no bit, the prep verdicts stand.
// gate != 0 skips the fallback launch.
__global__ void __launch_bounds__(64)
k_rlc_check(const uint32_t* __restrict__ out_inf, const unsigned long long* __restrict__ err, const uint32_t* __restrict__ n_w,
            uint32_t* __restrict__ gate, uint32_t* __restrict__ report, uint32_t* __restrict__ user_report) {
  if (threadIdx.x != 0) return;
  const bool any = *n_w != 0;
  const bool held = *out_inf == 1u && *err == ~0ull;
  const uint32_t rep = !any ? 0u : (held ? DVP_VERIFY_RLC_COMBINED : DVP_VERIFY_RLC_FALLBACK);
  *gate = (!any || held) ? 1u : 0u;
  *report = rep;
  if (user_report) *user_report = rep;
}

// dvp_verify_set_binding: the two hashes of the transcript's compile-time half, process-wide like the codec rule.  NULL = BLAKE3(""),
// the reference's value.  verify_consts reads them once per call, under the mutex: a call in flight keeps what it started with.
static std::mutex g_bind_mu;
static bool g_bind_has[2] = {false, false};
static uint8_t g_bind_hash[2][32];
extern "C" int dvp_verify_set_binding(const uint8_t srs_hash[32], const uint8_t circuit_hash[32]) {
  std::lock_guard<std::mutex> g(g_bind_mu);
  const uint8_t* h[2] = {srs_hash, circuit_hash};
  for (int k = 0; k < 2; ++k) {
    g_bind_has[k] = h[k] != nullptr;
    if (h[k]) memcpy(g_bind_hash[k], h[k], 32);
  }
  return DVP_OK;
}
extern "C" int dvp_verify_get_binding(uint8_t srs_hash[32], uint8_t circuit_hash[32]) {
  if (!srs_hash || !circuit_hash) return DVP_EINVAL;
  std::lock_guard<std::mutex> g(g_bind_mu);
  uint8_t* h[2] = {srs_hash, circuit_hash};
  for (int k = 0; k < 2; ++k) {
    if (g_bind_has[k]) memcpy(h[k], g_bind_hash[k], 32);
    else b3::hash(nullptr, 0, h[k]);
  }
  return DVP_OK;
}

int verify_consts(const uint64_t tau[4], const uint64_t delta[4], const uint64_t eps[4], VerifyConsts* c) {
  Fr t, d, e;
  DVP_TRY(load_trapdoor(tau, delta, eps, &t, &d, &e));
  c->tau = t;
  c->delta_m = fr_to_mont(d);
  c->delta2_m = fr_to_mont(fr_mul(c->delta_m, d));  // delta^2 (canonical), then times R
  c->eps_m = fr_to_mont(e);
  uint8_t h[32];
  {
    std::lock_guard<std::mutex> g(g_bind_mu);
    b3::compile_hash(g_bind_has[0] ? g_bind_hash[0] : nullptr, g_bind_has[1] ? g_bind_hash[1] : nullptr, h);
  }
  memcpy(c->h_ct.w, h, 32);
  return DVP_OK;
}

static int verify_enqueue(const VerifyConsts& c, const void* d_pub, uint32_t npub, const void* d_proofs, size_t n, void* d_verdicts,
                          hipStream_t st) {
  const Aff* tab;
  DVP_TRY(gen_table(&tab, st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  DVP_LAUNCH(k_verify<false>, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const uint8_t*)d_proofs, n,
                     (const Fr*)d_pub, npub, c, tab, T, codec_rule_now(), (uint8_t*)d_verdicts, (const uint32_t*)nullptr);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}


// ---- workspaces of the combined check: per device, one per host thread in flight ----------------------------------------------
// A call holds its workspace while it enqueues and then marks the end of its kernels with `ev`; the next call on that workspace
// orders itself behind them on the GPU (hipStreamWaitEvent), so nothing here waits on the host.  Growing happens before the call
// enqueues anything (after the previous kernels on it ended): no hipMalloc / hipFree between enqueued kernels.
struct RlcWs {
  int device = -1;
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  bool used = false;  // ev was recorded
  bool held = false;  // a call is enqueuing on it (under g_rlc_mu)
};
static std::mutex g_rlc_mu;
static std::vector<std::unique_ptr<RlcWs>> g_rlc_ws;

struct RlcHold {
  RlcWs* ws = nullptr;
  hipStream_t st = nullptr;
  bool enqueued = false;
  ~RlcHold() {
    if (!ws) return;
    if (enqueued) ws->used = hipEventRecord(ws->ev, st) == hipSuccess;
    std::lock_guard<std::mutex> g(g_rlc_mu);
    ws->held = false;
  }
};

static int rlc_acquire(size_t need, hipStream_t st, RlcHold& h) {
  int dev;
  DVP_HIP(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> g(g_rlc_mu);
    for (auto& w : g_rlc_ws)
      if (w->device == dev && !w->held) {
        h.ws = w.get();
        break;
      }
    if (!h.ws) {
      g_rlc_ws.emplace_back(new RlcWs);
      h.ws = g_rlc_ws.back().get();
      h.ws->device = dev;
    }
    h.ws->held = true;
  }
  h.st = st;
  RlcWs& w = *h.ws;
  if (!w.ev) DVP_HIP(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  if (w.bytes < need) {
    if (w.used) DVP_HIP(hipEventSynchronize(w.ev));
    if (w.p) (void)hipFree(w.p);
    w.p = nullptr;
    w.bytes = 0;
    w.used = false;
    DVP_HIP(hipMalloc(&w.p, need));
    w.bytes = need;
  } else if (w.used) {
    DVP_HIP(hipStreamWaitEvent(st, w.ev, 0));
  }
  return DVP_OK;
}

// workspace layout for n proofs (N = 2n + 1 MSM entries: 97 B each, plus 32 B per proof for r_j u0_j)
struct RlcLayout {
  size_t sc, bases, inf, ur, part, part_w, ctrl, total;
};
static RlcLayout rlc_layout(size_t n) {
  const size_t N = 2 * n + 1;
  Carver c;
  RlcLayout l;
  l.sc = c.take(32 * N);
  l.bases = c.take(64 * N);
  l.inf = c.take(N);
  l.ur = c.take(32 * n);
  l.part = c.take(32 * (size_t)RLC_SUM_BLOCKS);
  l.part_w = c.take(4 * (size_t)RLC_SUM_BLOCKS);
  l.ctrl = c.take(128);  // MSM x, y [0, 64) | MSM infinity u32 [64] | scalar-range word u64 [72] | |W| [80] | gate [84] | report [88]
  l.total = c.o;
  return l;
}

// key = seed, or BLAKE3("dv-pari verify rlc v1" || tau || delta || epsilon), each as 32 little-endian bytes
static void rlc_key(const uint64_t tau[4], const uint64_t delta[4], const uint64_t eps[4], const uint8_t* seed, uint8_t key[32]) {
  trapdoor_key("dv-pari verify rlc v1", tau, delta, eps, seed, key);
}

static int rlc_enqueue(const VerifyConsts& c, const uint8_t key[32], const void* d_pub, uint32_t npub, const void* d_proofs, size_t n,
                       void* d_verdicts, void* d_report, hipStream_t st) {
  const Aff* tab;
  DVP_TRY(gen_table(&tab, st));
  GfSqrTables T;
  DVP_TRY(gf_sqr_tables(&T, st));
  const RlcLayout lay = rlc_layout(n);
  RlcHold h;
  DVP_TRY(rlc_acquire(lay.total, st, h));
  char* ws = (char*)h.ws->p;
  Fr* sc = (Fr*)(ws + lay.sc);
  Aff* bases = (Aff*)(ws + lay.bases);
  uint8_t* inf = (uint8_t*)(ws + lay.inf);
  Fr* ur = (Fr*)(ws + lay.ur);
  Fr* part = (Fr*)(ws + lay.part);
  uint32_t* part_w = (uint32_t*)(ws + lay.part_w);
  char* ctrl = ws + lay.ctrl;
  uint32_t* out_xy = (uint32_t*)ctrl;
  uint32_t* out_inf = (uint32_t*)(ctrl + 64);
  unsigned long long* err = (unsigned long long*)(ctrl + 72);
  uint32_t* n_w = (uint32_t*)(ctrl + 80);
  uint32_t* gate = (uint32_t*)(ctrl + 84);
  uint32_t* report = (uint32_t*)(ctrl + 88);
  b3d::Words8 kw;
  memcpy(kw.w, key, 32);
  const int rule = codec_rule_now();
  uint8_t* verdicts = (uint8_t*)d_verdicts;
  h.enqueued = true;
  DVP_LAUNCH(k_verify_rlc_prep, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const uint8_t*)d_proofs, n,
                     (const Fr*)d_pub, npub, c, kw, T, rule, sc, bases, inf, ur, verdicts);
  const uint32_t nparts = std::min<uint32_t>(cdiv(n, RLC_SUM_TPB), RLC_SUM_BLOCKS);
  DVP_LAUNCH(k_rlc_sum_blocks, dim3(nparts), dim3(RLC_SUM_TPB), 0, st, (const Fr*)ur, (const uint8_t*)verdicts, n, part, part_w);
  DVP_LAUNCH(k_rlc_sum_final, dim3(1), dim3(RLC_SUM_TPB), 0, st, (const Fr*)part, (const uint32_t*)part_w, nparts, tab, sc + 2 * n,
                     bases + 2 * n, inf + 2 * n, n_w);
  DVP_HIP(hipGetLastError());
  DVP_TRY(msm_affine_dev(sc, bases, inf, 2 * n + 1, MsmOut{out_xy, out_inf, nullptr, nullptr, nullptr, 0, err}, st));
  DVP_LAUNCH(k_rlc_check, dim3(1), dim3(64), 0, st, (const uint32_t*)out_inf, (const unsigned long long*)err, (const uint32_t*)n_w, gate,
                     report, (uint32_t*)d_report);
  DVP_LAUNCH(k_verify<true>, dim3(cdiv(n, 256)), dim3(256), 4 * GF_LDSK_BYTES_PER_WAVE, st, (const uint8_t*)d_proofs, n,
                     (const Fr*)d_pub, npub, c, tab, T, rule, verdicts, (const uint32_t*)gate);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

}  // namespace dvp

using namespace dvp;

// Every flavour checks in this order: the trapdoor, n_public, n == 0 (DVP_OK; the host _rlc flavour also writes *report = 0), then the
// pointers, then the public inputs.
extern "C" int dvp_verify_batch_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                                    uint32_t n_public, const void* d_proofs, size_t n, void* d_verdicts, void* stream) {
  VerifyConsts c;
  DVP_TRY(verify_consts(tau, delta, epsilon, &c));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!d_proofs || !d_verdicts || (n_public && !d_public_inputs)) return DVP_EINVAL;
  return verify_enqueue(c, d_public_inputs, n_public, d_proofs, n, d_verdicts, (hipStream_t)stream);
}

extern "C" int dvp_verify_batch(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                                uint32_t n_public, const uint8_t* proofs, size_t n, uint8_t* verdicts) {
  VerifyConsts c;
  DVP_TRY(verify_consts(tau, delta, epsilon, &c));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!proofs || !verdicts || (n_public && !public_inputs)) return DVP_EINVAL;
  const size_t npub_all = (size_t)n_public * n;
  DVP_TRY(scalars_in_range(public_inputs, npub_all));  // the flat index of the first bad one
  DevBuf dp, dpub, dv;
  DVP_TRY(dp.up(proofs, n * 118));
  DVP_TRY(dpub.up(public_inputs, npub_all * 32));
  DVP_TRY(dv.alloc(n));
  DVP_TRY(verify_enqueue(c, dpub.p, n_public, dp.p, n, dv.p, 0));
  return dv.down(verdicts, n);
}

extern "C" int dvp_verify_batch_rlc_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                                        uint32_t n_public, const void* d_proofs, size_t n, const uint8_t seed[32], void* d_verdicts,
                                        void* d_report, void* stream) {
  VerifyConsts c;
  DVP_TRY(verify_consts(tau, delta, epsilon, &c));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) return DVP_OK;
  if (!d_proofs || !d_verdicts || (n_public && !d_public_inputs) || n > DVP_VERIFY_RLC_MAX_PROOFS) return DVP_EINVAL;
  uint8_t key[32];
  rlc_key(tau, delta, epsilon, seed, key);
  return rlc_enqueue(c, key, d_public_inputs, n_public, d_proofs, n, d_verdicts, d_report, (hipStream_t)stream);
}

extern "C" int dvp_verify_batch_rlc(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                                    uint32_t n_public, const uint8_t* proofs, size_t n, const uint8_t seed[32], uint8_t* verdicts,
                                    uint32_t* report) {
  VerifyConsts c;
  DVP_TRY(verify_consts(tau, delta, epsilon, &c));
  if (n_public > VERIFY_MAX_PUBLIC) return DVP_EINVAL;
  if (!n) {
    if (report) *report = 0;
    return DVP_OK;
  }
  if (!proofs || !verdicts || (n_public && !public_inputs) || n > DVP_VERIFY_RLC_MAX_PROOFS) return DVP_EINVAL;
  const size_t npub_all = (size_t)n_public * n;
  DVP_TRY(scalars_in_range(public_inputs, npub_all));  // the flat index of the first bad one
  uint8_t key[32];
  rlc_key(tau, delta, epsilon, seed, key);
  DevBuf dp, dpub, dv, drep;
  DVP_TRY(dp.up(proofs, n * 118));
  DVP_TRY(dpub.up(public_inputs, npub_all * 32));
  DVP_TRY(dv.alloc(n));
  DVP_TRY(drep.alloc(4));
  DVP_TRY(rlc_enqueue(c, key, dpub.p, n_public, dp.p, n, dv.p, drep.p, 0));
  DVP_TRY(dv.down(verdicts, n));
  uint32_t rep = 0;
  DVP_TRY(drep.down(&rep, 4));
  if (report) *report = rep;
  return DVP_OK;
}

extern "C" int dvp_verify(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                          uint32_t n_public, const uint8_t proof[118], int* accepted, uint32_t* reasons) {
  if (!proof || !accepted) return DVP_EINVAL;
  uint8_t v = 0xff;
  DVP_TRY(dvp_verify_batch(tau, delta, epsilon, public_inputs, n_public, proof, 1, &v));
  *accepted = v == 0;
  if (reasons) *reasons = v;
  return DVP_OK;
}

// sp1_generate_scalar_from_raw_public_input (src/gnark_r1cs.rs:214-229): BLAKE3 of the 8-byte LE raw value, bytes 0..3 of the digest
// cleared, the 32 bytes read BIG-endian -- a value < 2^224 < p (the loop multiplies by 256 per byte, whatever its comment says)
extern "C" int dvp_sp1_public_input(uint64_t raw, uint64_t out[4]) {
  if (!out) return DVP_EINVAL;
  uint8_t le[8], h[32];
  for (int b = 0; b < 8; ++b) le[b] = (uint8_t)(raw >> (8 * b));
  b3::hash(le, 8, h);
  for (int k = 0; k < 4; ++k) {
    uint64_t w = 0;
    for (int b = 0; b < 8; ++b) {
      const int idx = 31 - (8 * k + b);  // byte 8k + b of the little-endian result
      w |= (uint64_t)(idx < 4 ? 0 : h[idx]) << (8 * b);
    }
    out[k] = w;
  }
  return DVP_OK;
}

