// The prover's state: DevCsr, the result block (ProverBlock), SrsSlot, struct dvp_prover, the shared constants, host_vanish, prover_ready.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
#pragma once
#include "prove_kernels.cuh"

struct DevCsr {
  uint32_t* row_ptr = nullptr;
  uint32_t* wire = nullptr;
  uint32_t* coeff = nullptr;
  uint32_t n_rows = 0;
  size_t nnz = 0;
  uint32_t max_coeff_id = 0;  // largest coefficient id stored (re-checked against the table in prover_ready)
};

// the prover's result block on the device; the first FIN_BYTES go to the host (pinned) in ONE copy at the end of a proof
struct ProverBlock {
  Fr abir0[4];                    // a0 b0 i0 r0, canonical
  unsigned long long flags[2];    // [0] unsatisfied row, [1] alpha in D u D'
  uint8_t enc[64];                // commit_p (30) | kzg_k (30) | 4 spare
  Fr alpha;                       // canonical (written by k_transcript; the host flavour keeps its own copy)
  unsigned long long msm_err[2];  // scalar-range words of deferred MSMs: [0] the commitment MSM's
  // the host copy ends here; device only (in the pinned mirror: the staging of the host flavour's challenge), both Montgomery:
  Fr alpha_m, neg_z;              // alpha, -Z_D(alpha)
};
static constexpr size_t FIN_BYTES = offsetof(ProverBlock, alpha_m);
static_assert(offsetof(ProverBlock, flags) == 128 && offsetof(ProverBlock, enc) == 144 && offsetof(ProverBlock, alpha) == 208 &&
              offsetof(ProverBlock, msm_err) == 240 && FIN_BYTES == 256 && offsetof(ProverBlock, neg_z) == 288 && sizeof(ProverBlock) == 320,
              "the layout the one copy per proof has always had: no padding, the host part first");
static constexpr size_t MIX_OFF_INF = 128, MIX_OFF_ERR = 136, MIX_OFF_ERR_OUT = 152, MIX_BYTES = 160;  // dvp_prover::mix
// An SRS slot (prove_slots.cuh): everything of a prover that depends on the SRS -- one verifier's SRS (SRS per Trapdoor,
// src/srs.rs:31-50,177) beside the circuit and the work buffers, which do not.  The prover's own fields of these names ARE the active
// slot, so every entry reads and writes them as it always has; the inactive slots are parked in dvp_prover::slots and selecting one
// swaps these fields on the host.  `live` = false: an index handed out and dropped again, reusable.
struct SrsSlot {
  Aff *bases_a = nullptr, *bases_k = nullptr;
  uint8_t *inf_a = nullptr, *inf_k = nullptr;
  bool have_srs[5] = {false, false, false, false, false};
  MsmFixedCtx* fx[2] = {nullptr, nullptr};
  size_t fx_lo[2] = {0, 0}, fx_hi[2] = {0, 0};
  uint64_t table_budget = UINT64_MAX;
  bool table_refused[2] = {false, false};
  b3d::Words8 h_ct;
  bool live = true;
};
struct dvp_prover {
  uint32_t log_m = 0, m = 0, n_pub = 0, n_wires = 0;
  dvp_ecfft* tree = nullptr;  // 2m leaves (tree2n)
  Fr *dD = nullptr, *dD2 = nullptr, *barw = nullptr, *z2inv = nullptr;  // Montgomery, m each
  DevCsr mat[3];
  Fr* coeffs_m = nullptr;
  uint32_t n_coeffs = 0;
  Aff* bases_a = nullptr;      // [g_m | g_q]        n_wires + m
  uint8_t* inf_a = nullptr;
  Aff* bases_k = nullptr;      // [g_k0 | g_k1 | g_k2] 4m
  uint8_t* inf_k = nullptr;
  bool have_srs[5] = {false, false, false, false, false};
  // stream of the host-pointer seam (dvp_prove / dvp_prove_cache_dir, which carry no stream argument): one per prover, so that
  // two provers driven from two host threads overlap on the GPU instead of meeting on the default stream
  hipStream_t own_stream = nullptr;
  // fixed-base MSM contexts over [g_m | g_q] and [g_k_0 | g_k_1 | g_k_2]: bases pre-rotated by tau^(20 w), built
  // lazily once the SRS is complete (12 x the base storage: 4.8 GB at m = 2^20 -- HBM is not the scarce resource)
  MsmFixedCtx* fx[2] = {nullptr, nullptr};
  size_t fx_lo[2] = {0, 0}, fx_hi[2] = {0, 0};  // index range of the bases the context of MSM `which` was built for
  // dvp_prover_set_table_budget: the most HBM the tables may hold per device (UINT64_MAX = no limit).  Under a limit the table of MSM
  // `which` covers exactly the prefix [0, covered) dvp_table_plan allots it, and the rest of the sum goes through the one-shot MSM
  uint64_t table_budget = UINT64_MAX;
  bool table_refused[2] = {false, false};  // the runtime refused this MSM's table: one-shot until the next dvp_prover_set_table_budget
  // the two halves of a mixed MSM: [prefix point 64 | suffix point 64 | their infinity flags 2 x u32 | their range words 2 x u64 | merged word u64]
  char* mix = nullptr;
  bool last_begin_extended = false;            // dvp_prove_begin_partial(need_extend): q2 / k_r are valid only if true
  uint32_t ext_filled = 0;                     // bit v: extended vector v of this proof is in E2 (extended here, or received and marked)
  // dvp_prover_trace_last (prove_trace.cuh): the buffers hold a COMPLETE proof -- set by trace_mark where a whole proof succeeds, cleared
  // by every entry that writes what the trace reads (SA, E, E2, r2, den, SK, the block, the result points) or replaces a base vector:
  // every begin and staged phase entry, the witness check (it reduces its argument into SA), the SRS setters.
  // challenge_sliced: this proof's challenge phase ran by index slices (den / SK are partial), so finishing it does not set trace_ok.
  // trace_rule: the codec rule the proof's two encodings were written under; a trace under another rule is refused
  bool trace_ok = false, challenge_sliced = false;
  int trace_rule = 0;
  void trace_mark() {
    trace_ok = true;
    trace_rule = codec_rule_now();
  }
  // in-library multi-GPU (dvp_set_devices): one shard per listed device, each with its slice of both base vectors
  struct Shard {
    int device = 0;
    size_t lo[2] = {0, 0}, hi[2] = {0, 0};
    Aff* bases[2] = {nullptr, nullptr};
    uint8_t* inf[2] = {nullptr, nullptr};
    Fr* sc[2] = {nullptr, nullptr};
    MsmFixedCtx* fx[2] = {nullptr, nullptr};
    uint32_t* out = nullptr;  // 2 x (16 words x||y + 1 word flag + pad)
    hipStream_t st = nullptr;
  };
  std::vector<Shard> shards;
  std::vector<int> shard_devices;
  int home_device = 0;
  uint32_t* mg_parts = nullptr;  // home: 64 records of 80 B (packed for msm_sum_points_dev: 64 x 64 B points, then 64 flags)
  // work buffers
  Fr *w = nullptr, *E = nullptr, *E2 = nullptr, *r2 = nullptr, *SA = nullptr /* [w | q2] */, *den = nullptr, *den2 = nullptr,
     *SK = nullptr, *partial = nullptr;
  ProverBlock* blk = nullptr;           // device: results, flags, encodings, challenge (its members are used by address only)
  Aff* pts = nullptr;                   // 2 result points
  uint32_t* pts_inf32 = nullptr;
  uint8_t* pts_inf8 = nullptr;
  bool enc_fused[2] = {false, false};   // blk->enc + 30 * which already holds the encoding of pts[which] (written by the MSM's own tail kernel)
                                        // AND fin_host mirrors the block's host part as of that MSM's end (copied before its final sync)
  Fr ctop_host[2];                      // layer log_m leaves (collapse points of D, D'), Montgomery
  // last-proof intermediates kept for parity tests
  Fr alpha_canon, abir0_host[4];
  Fr neg_z_alpha_m;  // -Z_D(alpha), kept between dvp_prove_challenge_partial and dvp_prove_challenge_finish
  // dvp_prover_debug_force_alpha (tests): this alpha (canonical, Montgomery) instead of the transcript's output
  bool alpha_forced = false;
  Fr alpha_forced_pair[2];
  std::vector<uint64_t> pub_host;
  uint8_t commit_p_host[30];
  ProverBlock* fin_host = nullptr;  // pinned mirror of the block (its device-only part: staging for alpha_m, -Z(alpha)) + a mixed MSM's merged word
  // side stream + events of the device transcript: -Z(alpha) is computed beside the challenge phase's vector kernels
  hipStream_t side = nullptr;
  hipEvent_t ev_alpha = nullptr, ev_negz = nullptr;
  // H(srs_hash || circuit_hash), the compile-time half of the transcript.  Default: both are hashes of empty buffers, as in the
  // reference (src/proving.rs:86-105,113-132); dvp_prover_set_transcript_binding replaces them.  Every path that derives alpha reads it.
  b3d::Words8 h_ct;
  // the SRS slots (prove_slots.cuh): one entry per index ever handed out; slots[active_slot] is a placeholder whose content lives in
  // the fields above (bases_a .. table_refused, h_ct) while it is active
  std::vector<SrsSlot> slots = std::vector<SrsSlot>(1);
  uint32_t active_slot = 0;
};

static const int PT = 256;
static const uint32_t HORNER_MAX_PUB = 48;  // ~ the Fr products per element of one extend pass

static Fr host_vanish(const dvp_prover* p, int which, const Fr& x_m) {
  const dvp_ecfft* c = p->tree;
  int kk = (int)p->log_m;
  Fr u = x_m, v = fr_one_mont();
  for (int d = 0; d < kk; ++d) {
    Fr uv = fr_mul(u, v), vv = fr_sqr(v);
    Fr nu = fr_add(fr_sub(fr_sqr(u), fr_mul(c->x0[d], uv)), fr_mul(c->t[d], vv));
    Fr nv = fr_sub(uv, fr_mul(c->x0[d], vv));
    u = nu;
    v = nv;
  }
  return fr_sub(u, fr_mul(p->ctop_host[which], v));
}

// the half of prover_ready that does not depend on the SRS: coefficients and all three matrices
static bool circuit_ready(const dvp_prover* p) {
  if (!(p->coeffs_m && p->mat[0].row_ptr && p->mat[1].row_ptr && p->mat[2].row_ptr)) return false;
  for (int k = 0; k < 3; ++k)  // whatever order set_coeffs / set_matrix were called in, every stored id must be in the table
    if (p->mat[k].nnz && p->mat[k].max_coeff_id >= p->n_coeffs) return false;
  return true;
}
static bool prover_ready(dvp_prover* p) {
  for (int k = 0; k < 5; ++k)
    if (!p->have_srs[k]) return false;
  return circuit_ready(p);
}
