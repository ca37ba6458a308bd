// Multi-scalar multiplication on sect233k1 for gfx950 -- replaces multi_scalar_mul (src/curve.rs:141-158; call sites
// src/proving.rs:463,512,680), which in the reference is n independent xsk233_mul_frob calls plus an add tree.  Here: a bucket method
// whose buckets are summed by batched-affine pair rounds.  DESIGN.md section 3.1 describes it and says what every stage costs; this is
// the map from a stage to the text that holds it.
//
// ONE translation unit: this file is the host side (below), and it includes the stage headers msm_*.cuh, which hold the kernels and
// the helpers bound to them.  Every kernel is launched from here and counted as "msm.hip:<kernel>" (common.h: DVP_LAUNCH).
//
// The default path, as the prover's fixed-base contexts run it (signed binary windows over rows 2^(o_w) P, all windows sharing ONE
// bucket set; a one-shot MSM has per-window bucket sets and tau-adic digits, see the flavours below):
//
//  recode      msm_recode.cuh.  A scalar becomes one entry word per window (FXW_*: valid | sign | table row | bucket key).  By default
//              nothing is written: level 1 of the sort recomputes the words from the scalars (fx_recode_signed_each; "fused level 1",
//              k_part_hist_signed / k_part_scatter_signed in msm_sort.cuh).
//  sort        msm_sort.cuh, scans in msm_scan.cuh.  Two-level counting sort of the entries by key (FxBits: high bits, then low
//              bits), both levels LDS-staged scatters, no global atomics.  Every bucket starts at an even position of the item list,
//              so the list read as pairs is the first pair round's descriptor array.
//  bookkeeping msm_rounds.cuh: k_mscan_local / _bsums / _add, k_round_desc_all.  One scan behind the sort's counts yields the counts,
//              offsets and descriptors of ALL pair rounds, the item offsets, the padding of odd buckets and the largest bucket.
//  pair rounds msm_rounds.cuh: k_affine_round<FIRST, TRACE, DENSE>.  One round halves every bucket in affine coordinates; a thread owns
//              B slots (aff_slots_per_thread, AFF_BMAX) and shares one inversion among them.  The inversion between the two passes is
//              private to a wave, or shared by the workgroup through LDS (AFF_SHARE_INV, aff_x_put / aff_x_get) in rounds that
//              plan at least a chip-full of additions (aff_share_plan, below).  Host side: PairRounds, below.
//  leftovers   MsmRun::reduce_leftovers, below; the four routes the stage capture names (include/dvpari_internal.h): a gather alone
//              (k_bucket_gather_items / k_bucket_gather_aff, msm_rounds.cuh), k_bucket_pairs + k_bucket_rest, the fan-in-K reducer with
//              the exception-free first level (k_accum_affine_fast + k_accum_affine_rest), or with the general one (msm_reduce.cuh).
//  merge       msm_merge.cuh: k_merge<GROUP, FIRST>.  Sum over k of k x bucket k by a pruned sum-over-subsets tree in lambda-projective
//              coordinates, 1 / 4 / 16 lanes per addition by level size.
//  tail        msm_merge.cuh: k_tail<true>, one workgroup, a row of 16 lanes per point: doublings, add tree, projective -> affine and
//              the optional 30-byte encoding; it resets the control words for the next MSM.
//
// Fixed-base tables: msm_table.cuh (k_dbl_table; k_frob_table for the tau-adic rows), built by msm_fixed_build below.  The inversion's
// multi-squaring tables: gf_sqr_tables, msm_reduce.cuh.  Sums of partial points (k_sum_points, k_join_points): msm_merge.cuh.
// Test-only and microbenchmark C entries: msm_debug.cuh, included among the C entries at the end of this file.
//
// Superseded flavours that knobs still select:
//  - tau-adic aligned windows (DVP_MSM_ALIGNED_SIGNED=0, and every one-shot MSM): k_recode<DIGIT>, rows tau^(o_w) P, Frobenius tail
//    (k_tail_groups + k_tail<false>); a one-shot MSM sorts with k_hist_local / k_hist_scan / k_scatter_local.
//  - unfused recode (DVP_MSM_SORT_FUSED=0): k_recode_signed writes the entry words to HBM before the sort reads them.
//  - per-round bookkeeping (DVP_MSM_ROUND_PIPELINE=0, and small MSMs): k_post_sort, then scan_exclusive_div + k_round_desc between rounds.
//  - the general reducer (DVP_MSM_ACCUM_FAST=0): k_accum_affine with its exceptional branches as the fan-in-K reducer's first level.
//  - DVP_MSM_MODE=proj: no pair rounds, the fan-in-K reducer on the sorted items (k_accum_affine, then k_accum_proj levels).
//
// In this file: the workspace, the stage capture and HeavyGate; MsmPlan / msm_plan and MsmFixedCtx; MsmLayout, MsmBuffers, msm_carve;
// MsmRun (sort, prepare_rounds, merge_and_tail, complete), PairRounds, reduce_leftovers, msm_core; the fixed-base contexts, the
// table-budget planner and the product C entries.
//
// All of it runs on the VALU (no MFMA: there is no dense contraction in this algorithm, and gfx950 has no carry-less multiplier --
// see gf233.cuh).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#include "k233.cuh"
#include "tau.cuh"
#include "codec.cuh"
#include "host_api.h"
#include "msm_recode.cuh"
#include "msm_scan.cuh"
#include "msm_sort.cuh"
#include "msm_table.cuh"
#include "msm_reduce.cuh"
#include "msm_rounds.cuh"
#include "msm_merge.cuh"

namespace dvp {

// wave trace of the pair rounds (dvp_debug_wave_trace): device buffer, record capacity, launch tag (counts traced launches)
// (buffer, capacity) are published together under a mutex: an MSM in flight on another thread takes one consistent snapshot per launch
static std::mutex g_wave_trace_mu;
static unsigned long long* g_wave_trace_buf = nullptr;
static uint32_t g_wave_trace_cap = 0;
static std::atomic<uint32_t> g_wave_trace_tag{0};
static void wave_trace_snapshot(unsigned long long** buf, uint32_t* cap) {
  std::lock_guard<std::mutex> g(g_wave_trace_mu);
  *buf = g_wave_trace_buf;
  *cap = g_wave_trace_cap;
}

// ---- workspace -----------------------------------------------------------------------------------
struct MsmWorkspace {
  std::mutex mu;
  void* p = nullptr;
  size_t bytes = 0;
  int device = -1;
  // side channel for the one number the host needs mid-MSM (largest bucket): pinned word + its own stream, so the copy
  // overtakes the first pair round that is already enqueued on the caller's stream
  hipStream_t aux = nullptr;
  hipEvent_t ev = nullptr;
  hipEvent_t ev_heavy = nullptr;  // end of this workspace's last run of pair rounds (HeavyGate)
  // a DEFERRED MSM (msm_core, d_err_defer) returns with its kernels still in flight: ev_busy marks their end on busy_stream.  A later
  // call on the same stream is ordered behind them by the stream itself; a call on another stream waits for the event ON THE GPU
  // (and the slot choice prefers a workspace that is idle, so that two provers in flight keep to a workspace each)
  hipEvent_t ev_busy = nullptr;
  hipStream_t busy_stream = nullptr;
  bool busy_valid = false;
  bool ctrl_clean = false;  // the control words at the head of the workspace are as an MSM expects them (msm_core)
  bool busy_for(hipStream_t st) { return busy_valid && busy_stream != st && hipEventQuery(ev_busy) == hipErrorNotReady; }
  uint32_t* pinned = nullptr;
  // round bookkeeping (counts, offsets, descriptors of the later pair rounds) runs on a side stream while the first round fills
  // the chip: ev_pre = the first round's offsets are in place, ev_side[r] = round r may start
  hipStream_t side = nullptr;
  hipEvent_t ev_pre = nullptr;
  std::vector<hipEvent_t> ev_side;
  int ensure_side(size_t rounds) {
    if (!side) {
      DVP_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
      DVP_HIP(hipEventCreateWithFlags(&ev_pre, hipEventDisableTiming));
    }
    while (ev_side.size() < rounds) {
      hipEvent_t b = nullptr;
      DVP_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
      ev_side.push_back(b);
    }
    return DVP_OK;
  }
  int ensure_aux() {
    if (aux) return DVP_OK;
    DVP_HIP(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
    DVP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    DVP_HIP(hipEventCreateWithFlags(&ev_heavy, hipEventDisableTiming));
    DVP_HIP(hipEventCreateWithFlags(&ev_busy, hipEventDisableTiming));
    DVP_HIP(hipHostMalloc((void**)&pinned, 64, hipHostMallocDefault));
    return DVP_OK;
  }
  // `need` is raised to the largest size any workspace of this device was ever asked for: which of the two slots a call gets
  // depends on timing, and a slot that had only seen the smaller MSM of a prover would otherwise be freed and re-allocated
  // (a device-wide synchronisation plus a multi-GB hipMalloc) in the middle of a later proof
  int ensure(size_t need, std::atomic<size_t>& dev_max) {
    size_t seen = dev_max.load();
    while (seen < need && !dev_max.compare_exchange_weak(seen, need)) {}
    if (seen > need) need = seen;
    int dev;
    DVP_HIP(hipGetDevice(&dev));
    if (p && (dev != device || bytes < need)) {
      // a deferred MSM's kernels may still be running in this allocation (the first proof: the K MSM is larger than the commitment
      // MSM in flight): wait for them explicitly rather than lean on hipFree's implicit device-wide synchronisation
      // (busy_valid was already consumed by the caller's hipStreamWaitEvent: the event itself is what says whether they ended)
      if (ev_busy) (void)hipEventSynchronize(ev_busy);
      (void)hipFree(p);
      p = nullptr;
      bytes = 0;
    }
    if (!p) {
      DVP_HIP(hipMalloc(&p, need));
      ctrl_clean = false;
      bytes = need;
      device = dev;
    }
    return DVP_OK;
  }
};
// grow-only workspaces, MSM_WS_SLOTS PER DEVICE: MSMs on different GPUs (in-library multi-GPU: one host thread per device,
// prove.hip) run concurrently, and so do up to MSM_WS_SLOTS MSMs on the SAME GPU (two provers on two host threads and two
// streams: the latency-bound stretches of one proof -- merge levels, tail, small rounds, host round trips -- are filled by the
// other's kernels); a further caller waits for slot 0.  The second slot allocates only when two calls do overlap.
constexpr int MSM_WS_SLOTS = 2;
static MsmWorkspace g_ws_dev[DVP_MAX_DEVICES][MSM_WS_SLOTS];
// where the calling thread's last MSM ran (dvp_debug_msm_rest_len)
struct LastMsm {
  int dev = -1, slot = 0;
  hipStream_t st = nullptr;
};
static thread_local LastMsm g_last_msm;
static std::atomic<size_t> g_ws_need[DVP_MAX_DEVICES];

// ---- stage capture (TEST ONLY: dvp_debug_msm_capture_arm / _fetch, include/dvpari_internal.h) -------------------------------------
// A thread arms the capture for its NEXT MSM.  That MSM runs msm_core as it always does and, at the stage boundaries, enqueues
// device-to-device copies of the arrays one stage hands to the next on its own stream: no kernel, no event, no wait.  The host does not
// know the lengths the device settled on (off[nkeys], a round's total) when it enqueues, so every copy takes the region's upper bound
// and the fetch, which waits for the stream, cuts the blob to the lengths the captured offsets name.  A copy that does not fit the
// arena is not made and the fetch then fails as a whole.  An MSM of a thread that has not armed pays one null check per stage.
// Behind the buckets the lengths are the host's own: the whole bucket array after every merge level, bucket 0 as level 0 kept it aside,
// the group sums of k_tail_groups (copied BEFORE k_tail reuses their memory as its ping-pong buffer) and what the last tail kernel wrote.
constexpr uint32_t CAPTURE_MAGIC = 0x43505644u, CAPTURE_VERSION = 2, CAPTURE_HDR_WORDS = 136, CAPTURE_MAX_ROUNDS = 40, CAPTURE_MAX_LEVELS = 24;
enum CaptureHdr {  // word indices of the blob's header
  CH_MAGIC = 0, CH_VERSION, CH_HDR_WORDS, CH_FLAVOUR /* bit 0: fixed-base, bit 1: signed digits */, CH_C, CH_W, CH_N_NARROW, CH_NKEYS, CH_SIGN_MASK,
  CH_N_TOTAL, CH_I0, CH_N, CH_RA, CH_RA_PLAN, CH_DENSE, CH_PIPELINE /* 0: per round, 1: side stream, 2: caller's stream */, CH_TPB, CH_AFF_CAP,
  CH_BMAX, CH_BMIN, CH_ROUTE, CH_K, CH_MAX_CNT, CH_ITEMS_LEN, CH_SHARE /* [40] */, CH_TOTAL = CH_SHARE + CAPTURE_MAX_ROUNDS /* [40] */,
  // version 2: the merge tree and the tail
  CH_LEVELS = CH_TOTAL + CAPTURE_MAX_ROUNDS, CH_TAIL /* CaptureTail */, CH_NPARTS, CH_ENC /* an encoding was written */, CH_RULE /* its codec rule */,
  CH_GROUP = CH_LEVELS + 8 /* [24]: lanes per addition of level j */
};
static_assert(CH_LEVELS == 104 && CH_GROUP + CAPTURE_MAX_LEVELS == CAPTURE_HDR_WORDS, "capture header layout");
enum CaptureRoute { CR_GATHER_ITEMS = 0, CR_GATHER_AFF, CR_BUCKET_PAIRS, CR_REDUCER_FAST, CR_REDUCER_GENERAL };
enum CaptureTail { CT_HEX_SIGNED = 0 /* k_tail<true>, -3 */, CT_QUAD_SIGNED /* k_tail<false>, -3 */, CT_FROBENIUS /* k_tail<false> alone */,
                   CT_GROUPS /* k_tail_groups + k_tail<false>, -4 */ };
struct MsmCapture {
  struct Sec { size_t at, bytes; };  // a region of the arena
  struct Round { Sec ocnt, ooff, desc, pts; };
  bool armed = false, taken = false;
  int dev = -1;
  hipStream_t st = nullptr;
  char* arena = nullptr;
  size_t cap = 0, used = 0, wanted = 0;  // wanted: what the MSM asked for, whether it fitted or not
  hipError_t copy_err = hipSuccess;
  uint32_t hdr[CAPTURE_HDR_WORDS] = {0};
  Sec cnt = {0, 0}, off = {0, 0}, items = {0, 0}, bkt = {0, 0};
  Round rounds[CAPTURE_MAX_ROUNDS] = {};
  uint32_t nrounds = 0;
  // behind bkt: the bucket array after every merge level, bucket 0 as kept aside, k_tail_groups' sums, what the last tail kernel wrote
  Sec levels[CAPTURE_MAX_LEVELS] = {}, save0 = {0, 0}, parts = {0, 0}, res_xy = {0, 0}, res_inf = {0, 0}, res_enc = {0, 0};
  uint32_t nlevels = 0;
  bool result = false;
  Sec grab(const void* src, size_t bytes, hipStream_t s) {
    const size_t at = Carver::align(wanted);
    wanted = at + bytes;
    if (wanted > cap) return Sec{0, 0};  // (the fetch sees wanted > cap)
    if (!bytes) return Sec{at, 0};
    const hipError_t e = hipMemcpyAsync(arena + at, src, bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess && copy_err == hipSuccess) copy_err = e;
    used = wanted;
    return Sec{at, bytes};
  }
  void release() {
    if (arena) (void)hipFree(arena);
    arena = nullptr;
    cap = used = wanted = 0;
    armed = taken = result = false;
    nrounds = nlevels = 0;
    copy_err = hipSuccess;
  }
};
static thread_local MsmCapture g_capture;

// Two MSMs on one device overlap everything EXCEPT their pair rounds: those fill the chip on their own (two of them side by side
// only contend: measured 4 % slower than taking turns), while everything around them -- sort, reducer, merge levels, tail, the
// prover's Fr stages and host round trips -- leaves lanes idle.  So the pair rounds of the second MSM wait ON THE GPU
// (hipStreamWaitEvent, no host block beyond the enqueue) for the end of the first one's, which staggers two provers that
// started in lockstep by themselves.
struct HeavyGate {
  std::mutex mu;
  hipEvent_t last = nullptr;
};
static HeavyGate g_heavy[DVP_MAX_DEVICES];

struct MsmPlan {
  uint32_t n;
  int c, W, n_narrow;
  uint32_t K, nkeys;
  size_t e_max, t1_max, t2_max;
};

static MsmPlan msm_plan(size_t n, const struct MsmFixedCtx* fx);
// The window split every flavour shares: the 234 real digits go into ceil(234 / c) windows (the return value) whose widths differ by
// at most one, the *n_narrow LOW windows being c - 1 digits wide.  What a flavour adds above them (overflow windows) is its own.
static int window_split(int c, int* n_narrow) {
  const int w_main = (234 + c - 1) / c;
  *n_narrow = w_main * c - 234;
  return w_main;
}
// Windows of the fixed-base mode. tau-adic expansions of reduced scalars are at most 234 digits long (measured: 229-233
// typical) and their top 3-4 digits are mostly zero.  A uniform split leaves a short top window (234 mod c digits) whose
// entries pile into a few hundred buckets of the shared set -- n/2^7 entries per bucket for c = 16 -- and the reducer
// then runs 15-long serial chains.  So the 234 digits are split into W_main = ceil(234/c) windows whose widths differ by
// at most one (the n_narrow low windows are c-1 digits wide, the entropy-poor top windows c), plus one overflow window
// for digits >= 234 that exists only for completeness (the recode flags anything longer than it covers).
struct MsmFixedCtx {
  Aff* table = nullptr;  // [W][n_total]
  uint32_t n_total = 0;
  int c = FX_C_MAX, W = TAU_DIGITS / FX_C_MAX, n_narrow = 0;
  void set_c(int cc) {
    c = cc;
    W = window_split(cc, &n_narrow) + 1;
  }
  bool signed_digits = false;    // aligned windows with digits in [-2^(c-1), 2^(c-1)] over the scalar's BINARY digits (k_recode_signed,
                                 // table rows 2^(o_w) P from k_dbl_table): 2^(c-1) buckets.  false = the tau-adic aligned windows
                                 // (k_recode, table rows tau^(o_w) P from k_frob_table)
  // 234 bits (a canonical scalar < 2^232, the last carry, one spare so that the top digit stays positive) in W = ceil(234 / c)
  // windows whose widths differ by at most one: the n_narrow LOW windows are c - 1 wide.  A request whose windows would all be
  // narrow is the next smaller c.
  void set_c_signed(int cc) {
    for (;; --cc) {
      W = window_split(cc, &n_narrow);
      if (n_narrow < W || cc <= 2) break;
    }
    c = cc;
    signed_digits = true;
  }
  int rows() const { return W; }
  int key_bits() const { return signed_digits ? c - 1 : c; }
  int hi_bits = -1;  // level-1 partition bits of the sort (set at creation)
  FxBits bits() const { FxBits b; b.hi = hi_bits; b.lo = key_bits() - b.hi; return b; }
};
static MsmPlan msm_plan(size_t n, const MsmFixedCtx* fx) {
  const bool fixed = fx != nullptr;
  MsmPlan p;
  p.n = (uint32_t)n;
  // cost model: W(c) * (8.4 n + 28 * 2^c) field multiplications.  Windows are evened out as in the fixed-base mode
  // (see MsmFixedCtx): the 234 real digits go into ceil(234/c) windows of c or c-1 digits (narrow ones first), the
  // digits above them (never seen beyond 236) into overflow windows.  A uniform 240/c split left a short top window
  // whose entries all fell into a few dozen buckets and serialised the reducer.
  auto windows = [](int c, int* n_narrow) { return window_split(c, n_narrow) + (TAU_DIGITS - 234 + c - 1) / c; };
  double best = 1e300;
  p.c = 4;
  int nn;
  for (int c = 4; c <= 15; ++c) {  // <= 15: the sort keeps 2^c u32 cursors in LDS
    int W = windows(c, &nn);
    double cost = W * (8.4 * (double)n + 28.0 * (double)(1u << c));
    if (cost < best) { best = cost; p.c = c; }
  }
  // 2^15 .. 2^17 points are latency all the way (config #2: ~45 dependent launches): with the round-4 chains (lambda-projective merge,
  // 16 lanes per product in the deep levels and the tail) two merge levels fewer beat the model's window -- tools/small_msm_sweep.py,
  // c = 10 / K = 8 against the model's c = 12 / K = 4: 1.43 against 1.63 ms at 2^16, 1.82 against 2.02 ms at 2^17 (2^14 and 2^18: no difference)
  // Round 6 (tools/small_msm_ck.py, after the tail's group sums and the reducer's cheaper levels): the same holds at 2^18 (c = 10 / K = 8:
  // 2.04 against 2.21 ms), and 2^19 points want c = 13 where the model says 14 (3.17 against 3.43 ms); 2^14 and 2^20 are flat
  const bool small_latency = !fixed && n >= ((size_t)1 << 15) && n <= ((size_t)1 << 18);
  if (small_latency) p.c = 10;
  if (!fixed && n > ((size_t)1 << 18) && n <= ((size_t)1 << 19)) p.c = 13;
  if (tune().msm_c >= 2 && tune().msm_c <= 15) p.c = (int)tune().msm_c;
  p.W = windows(p.c, &p.n_narrow);
  p.nkeys = (uint32_t)p.W << p.c;
  if (fixed) {  // all windows share one bucket set (bases pre-rotated by tau^(c w))
    p.c = fx->c;
    p.W = fx->W;
    p.n_narrow = fx->n_narrow;
    p.nkeys = 1u << fx->key_bits();
  }
  p.e_max = n * (size_t)p.W;
  // fan-in: keep >= ~256k level-1 tasks in flight when the input allows it
  uint32_t K = (uint32_t)(p.e_max / 262144);
  if (K < 8) K = 8;
  if (K > 16) K = 16;
  // small inputs (config #2's 2^16 points: ~1.5 M entries) are chain latency in the reducer as well: 2^16 .. 2^18 points run
  // 5-10 % faster with three additions per task than with seven (tools/small_msm_sweep.py)
  if (!fixed && n <= ((size_t)1 << 18)) K = 4;
  if (small_latency) K = 8;
  if (!fixed && n > ((size_t)1 << 18) && n <= ((size_t)1 << 19)) K = 8;
  // fixed-base mode: the reducer only sees what the pair rounds leave (<= ~20 entries in the fullest buckets) and is pure
  // chain latency there: two levels of <= 7 additions beat one of <= 15 (2^20 prove: 24.26 against 24.58 ms)
  if (fixed) K = 8;
  if (tune().msm_k >= 2 && tune().msm_k <= 64) K = (uint32_t)tune().msm_k;
  p.K = K;
  p.t1_max = p.e_max / K + p.nkeys + 1;
  p.t2_max = p.t1_max / K + p.nkeys + 1;
  return p;
}

// dynamic-LDS limits are a per-device property of a kernel: set them once on every device that runs an MSM
static int msm_set_lds_limits(int dev) {
  static std::mutex attr_mu;
  static bool attr_done[DVP_MAX_DEVICES] = {false};
  std::lock_guard<std::mutex> ga(attr_mu);
  if (attr_done[dev]) return DVP_OK;
  const struct { const void* f; int bytes; } sort_lim[] = {
      {(const void*)k_scatter_local, 131072}, {(const void*)k_hist_local, 65536}, {(const void*)k_scatter_local2, 131072},
      {(const void*)k_hist_local2, 65536}, {(const void*)k_part_scatter_staged, (int)FX_STAGE1_LDS},
      {(const void*)k_part_scatter_signed<true>, (int)FX_STAGE1_LDS}, {(const void*)k_scatter_local2_staged, (int)FX_STAGE2_LDS}};
  const void* ec[] = {(const void*)k_accum_affine<true, false>, (const void*)k_accum_affine<false, false>, (const void*)k_accum_affine<true, true>,
                      (const void*)k_accum_affine<false, true>, (const void*)k_accum_proj<1>, (const void*)k_accum_proj<4>, (const void*)k_accum_proj<16>,
                      (const void*)k_accum_affine_fast<true, false>, (const void*)k_accum_affine_fast<false, false>, (const void*)k_accum_affine_fast<true, true>,
                      (const void*)k_accum_affine_fast<false, true>, (const void*)k_accum_affine_rest<true>, (const void*)k_accum_affine_rest<false>,
                      (const void*)k_tail_groups, (const void*)k_merge<1, false>, (const void*)k_merge<4, false>, (const void*)k_merge<16, false>, (const void*)k_merge<1, true>, (const void*)k_merge<4, true>, (const void*)k_merge<16, true>,
                      (const void*)k_affine_round<true, false>, (const void*)k_affine_round<false, false>, (const void*)k_affine_round<true, true>,
                      (const void*)k_affine_round<false, true>, (const void*)k_affine_round<false, false, true>, (const void*)k_affine_round<false, true, true>,
                      (const void*)k_sum_points, (const void*)k_tail<false>, (const void*)k_tail<true>,
                      (const void*)k_bucket_pairs, (const void*)k_bucket_rest};
  for (const auto& l : sort_lim) DVP_HIP(hipFuncSetAttribute(l.f, hipFuncAttributeMaxDynamicSharedMemorySize, l.bytes));
  // (the pair rounds ask for EC_LDS plus the exchange area of their shared inversion: inside the same limit)
  static_assert(EC_LDS + aff_exchange_bytes(EC_TPB / 64) <= EC_LDS_Q, "k_affine_round's dynamic LDS exceeds the limit set here");
  for (const void* f : ec) DVP_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, EC_LDS_Q));
  attr_done[dev] = true;
  return DVP_OK;
}

// a run-time flag or value as a template argument: f receives std::true_type / std::false_type, or the lanes per bucket of a
// descriptor kernel (by the average bucket size of the round) as a std::integral_constant
template <class F> static void with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static void with_lpk(size_t per_key, F&& f) {
  if (per_key >= 48) f(std::integral_constant<int, 64>{});
  else if (per_key >= 8) f(std::integral_constant<int, 16>{});
  else f(std::integral_constant<int, 4>{});
}

// ---- the workspace of one MSM, described once ------------------------------------------------------------------------------
// MsmLayout = every decision that shapes the workspace, from (n, plan, context, knobs) alone: no HIP call.  MsmBuffers = its regions,
// typed; msm_carve is the ONE place that gives a region its size, its position and its pointer (256-byte aligned, in this order).
struct MsmLayout {
  FxBits fb;                // the fixed-base sort's split of the key bits ({0, 0} for a one-shot MSM)
  bool fused1;              // signed flavour: level 1 of the sort reads the scalars themselves (k_part_hist_signed), a block per fx_S scalars
  uint32_t fx_S, fx_nblk, fx_nch;  // fx_nch: chunks of the level-1 scan (k_part_scan_chunks)
  size_t sort_cells, affA_n, affB_n;
  bool affine_mode;
  // pair rounds the SIZE rule allows (ra_plan; the largest bucket, which only the device knows, may stop them sooner): rounds run while
  // a round still carries >= aff_min additions of the e_est entries that really exist (the overflow windows are empty in practice)
  size_t aff_min, e_est;
  int ra_plan;
  // bookkeeping of ALL later rounds behind the sort (prepare_rounds): every round keeps its own counts / offsets / descriptors,
  // so nothing the bookkeeping writes is ever read by a round still in flight
  bool pipelined, side_stream;
  bool dense;               // that bookkeeping lays a round out densely (additions first, leftovers behind them), two descriptor words per slot
  size_t desc_at[41], desc_n;  // round r's descriptors start at gdesc + desc_at[r] (r >= 1; even: uint2 on the dense path)
  // k_bucket_pairs' list of buckets that met an exceptional pair (<= nkeys), or k_accum_affine_fast's list of such TASKS (chunks of K entries)
  // (sized by the reducer's own bound on its first-level tasks at its largest, no pair round run: (e_max + nkeys) / K + nkeys + 1)
  size_t rest_cap;
  uint32_t tail_groups;     // k_tail_groups: workgroups of 16 points
  size_t bytes;             // the whole workspace
  // pipelined bookkeeping on the caller's stream: the scan of all rounds also yields the item offsets, the odd buckets' padding and the
  // largest bucket (k_mscan_add)
  bool sort_done_by_mscan() const { return pipelined && !side_stream; }
};
struct MsmBuffers {
  unsigned long long* err;  // err (u64) | d_max, rest_n (u32 each) | err_out (u64): the tail kernel's copy of err for the host | the tail kernel's copy of (d_max, rest_n)
  uint32_t *d_max, *rest_n;  // the largest bucket; entries of the rest list
  uint16_t *digits, *plo, *hist16;
  uint32_t *digits32, *pid, *phist, *pbase, *ctot, *pstart, *cstart, *pcount, *chunk_off;
  uint32_t *cnt, *off, *ntask, *toff, *cnt2, *off2, *bsum, *items, *rest_list;
  Ld *bufA, *bufB, *bkt, *tail;
  Aff *affA, *affB;
  Gf* prefix;
  uint32_t* gdesc;  // one word per output slot (rounds after the first; dense: two)
  uint32_t* rp;     // (counts, offsets) of rounds 1 .. ra_plan
  uint32_t* bsum2;  // scan scratch of the all-rounds bookkeeping: a row of block sums per round
};
// the regions over `base`, and their total (with base = 0 the only thing of use)
static MsmBuffers msm_carve(size_t n, const MsmPlan& p, const MsmFixedCtx* fx, const MsmLayout& L, void* base, size_t* bytes = nullptr) {
  Carver c{(uintptr_t)base};
  MsmBuffers b;
  const uint32_t FX_NP = L.fb.np();
  const size_t keys4 = ((size_t)p.nkeys + 1) * 4;
  b.err = c.take<unsigned long long>(32);
  b.d_max = (uint32_t*)(b.err + 1);
  b.rest_n = b.d_max + 1;
  b.digits = c.take<uint16_t>(fx ? 16 : (size_t)p.W * n * 2);
  b.digits32 = c.take<uint32_t>(fx && !L.fused1 ? p.e_max * 4 : 16);
  b.plo = c.take<uint16_t>(fx ? p.e_max * 2 : 16);
  b.pid = c.take<uint32_t>(fx ? p.e_max * 4 : 16);
  for (uint32_t** r : {&b.phist, &b.pbase}) *r = c.take<uint32_t>(fx ? (size_t)L.fx_nblk * FX_NP * 4 : 16);
  b.ctot = c.take<uint32_t>(fx ? (size_t)FX_NP * L.fx_nch * 4 : 16);
  b.pstart = c.take<uint32_t>((FX_NP_MAX + 1) * 4 * 3);
  b.cstart = b.pstart + FX_NP_MAX + 1;
  b.pcount = b.cstart + FX_NP_MAX + 1;
  for (uint32_t** r : {&b.cnt, &b.off, &b.ntask, &b.toff, &b.cnt2, &b.off2}) *r = c.take<uint32_t>(keys4);
  b.bsum = c.take<uint32_t>(((size_t)p.nkeys / SCAN_BLK + 8) * 4);
  b.items = c.take<uint32_t>((p.e_max + (size_t)p.nkeys + 2) * 4);  // odd buckets are padded to even (k_post_sort)
  b.hist16 = c.take<uint16_t>(L.sort_cells * 2);
  b.chunk_off = c.take<uint32_t>(L.sort_cells * 4);
  b.bufA = c.take<Ld>(p.t1_max * sizeof(Ld));
  b.bufB = c.take<Ld>(p.t2_max * sizeof(Ld));
  b.affA = c.take<Aff>(L.affine_mode ? L.affA_n * sizeof(Aff) : 16);
  b.affB = c.take<Aff>(L.affine_mode ? L.affB_n * sizeof(Aff) : 16);
  b.prefix = c.take<Gf>(L.affine_mode ? (L.affA_n + 256) * sizeof(Gf) : 16);  // one prefix product per output slot (+ the B - 1 <= 254 slots the last thread's rows may overhang)
  b.gdesc = c.take<uint32_t>(L.affine_mode ? L.desc_n * sizeof(uint32_t) : 16);
  b.rp = c.take<uint32_t>(L.pipelined ? (size_t)L.ra_plan * 2 * keys4 : 16);
  b.bsum2 = c.take<uint32_t>(((size_t)((L.ra_plan > 0 ? L.ra_plan : 1) + 1) * ((size_t)p.nkeys / SCAN_BLK + 1) + 8) * 4);
  b.bkt = c.take<Ld>((size_t)p.nkeys * sizeof(Ld));
  b.rest_list = c.take<uint32_t>(L.rest_cap * 4);
  b.tail = c.take<Ld>(((size_t)2 * p.W * p.c + 1 + 2 * (size_t)L.tail_groups) * sizeof(Ld));
  if (bytes) *bytes = c.o;
  return b;
}
static MsmLayout msm_layout(size_t n, const MsmPlan& p, const MsmFixedCtx* fx, const Tune& tn) {
  MsmLayout L{};
  L.fb = fx ? fx->bits() : FxBits{0, 0};
  L.fused1 = fx && fx->signed_digits && tn.msm_sort_fused != 0;
  L.fx_S = L.fused1 ? (FX_CHUNK / (uint32_t)p.W > 0 ? FX_CHUNK / (uint32_t)p.W : 1u) : 0u;
  L.fx_nblk = L.fused1 ? cdiv(n, L.fx_S) : cdiv(p.e_max, FX_CHUNK);
  L.fx_nch = cdiv(L.fx_nblk, FX_SCAN_CB);
  L.sort_cells = fx ? ((size_t)(L.fx_nblk + L.fb.np() + 1) << L.fb.lo) : ((size_t)p.W * cdiv(n, SORT_CHUNK) << p.c);
  L.affine_mode = !tn.msm_proj;
  L.affA_n = p.e_max / 2 + p.nkeys + 1;
  L.affB_n = p.e_max / 4 + p.nkeys + 1;
  L.aff_min = (size_t)(tn.msm_aff_min > 0 ? tn.msm_aff_min : 1);
  L.e_est = (size_t)n * (size_t)((fx && fx->signed_digits) ? p.W : (234 + p.c - 1) / p.c);
  while (L.affine_mode && L.ra_plan < 40 && (L.e_est >> (L.ra_plan + 1)) >= L.aff_min) ++L.ra_plan;
  L.pipelined = L.affine_mode && tn.msm_round_pipeline != 0 && L.ra_plan >= 2 && L.e_est >= 4 * (size_t)p.nkeys;
  L.side_stream = L.pipelined && tn.msm_round_pipeline == 1;
  L.dense = L.pipelined && tn.msm_round_dense != 0;
  L.desc_n = L.affA_n + 64;
  if (L.pipelined) {
    size_t cap_r = p.e_max + p.nkeys, at = 0;
    for (int r = 0; r < L.ra_plan; ++r) {
      const size_t out_max = cap_r / 2 + p.nkeys + 1;
      if (r >= 1) { L.desc_at[r] = at; at += (L.dense ? 2 : 1) * (out_max + 64); }
      cap_r = out_max;
    }
    if (at > L.desc_n) L.desc_n = at;
  }
  L.rest_cap = (size_t)p.nkeys + 2 + (p.e_max + (size_t)p.nkeys) / (size_t)(p.K > 0 ? p.K : 1);
  L.tail_groups = ((uint32_t)(p.W * p.c) + 15u) / 16u;
  (void)msm_carve(n, p, fx, L, nullptr, &L.bytes);
  return L;
}

// the workspace this call runs in, held through `g` until the call returns: a slot nobody holds AND whose last deferred MSM (if any)
// is finished or sits on this very stream, else any free slot, else a wait for slot 0; then large enough for `bytes`
static int msm_acquire_workspace(int dev, hipStream_t st, int ws_slots, size_t bytes, std::unique_lock<std::mutex>& g, MsmWorkspace** out) {
  int ws_slot = 0;
  for (int pass = 0; pass < 2 && !g.owns_lock(); ++pass)
    for (int sl = 0; sl < ws_slots && !g.owns_lock(); ++sl) {
      g = std::unique_lock<std::mutex>(g_ws_dev[dev][sl].mu, std::try_to_lock);
      if (g.owns_lock() && pass == 0 && g_ws_dev[dev][sl].busy_for(st)) g.unlock();
      if (g.owns_lock()) ws_slot = sl;
    }
  if (!g.owns_lock()) g = std::unique_lock<std::mutex>(g_ws_dev[dev][0].mu);
  MsmWorkspace& ws = g_ws_dev[dev][ws_slot];
  g_last_msm = LastMsm{dev, ws_slot, st};
  if (ws.busy_valid) {  // kernels of a deferred MSM may still be using this workspace
    if (ws.busy_stream != st) DVP_HIP(hipStreamWaitEvent(st, ws.ev_busy, 0));
    ws.busy_valid = false;
  }
  DVP_TRY(ws.ensure(bytes, g_ws_need[dev]));
  *out = &ws;
  return DVP_OK;
}

// One MSM: the call, its plan and layout, the workspace it holds -- what every stage reads -- and the stages, in the order msm_core
// runs them.  A stage only enqueues; what one stage hands to the next lives in the workspace (b) or in PairRounds.
struct PairRounds;
struct MsmRun {
  const uint32_t* scalars;
  const uint8_t* inf;
  const Aff* bases0;  // the one-shot MSM's bases, or the context's pre-rotated table
  size_t n;
  const MsmFixedCtx* fx;
  uint32_t i0, sign_mask;  // sign_mask: signed flavours keep the sign in bit 31 of an item
  hipStream_t st;
  int dev, ws_slots;
  Tune tn;
  MsmPlan p;
  MsmLayout L;
  MsmBuffers b;
  MsmWorkspace* ws;
  GfSqrTables Tsq;
  MsmCapture* cap;  // the calling thread's armed stage capture, else nullptr (every MSM but a test's)
  int reduce_leftovers(const PairRounds& pr) const;
  // the end of reduce_leftovers, whichever route it took: the bucket array as the merge tree will read it
  int leftovers_done(int route) const {
    if (cap) {
      cap->hdr[CH_ROUTE] = (uint32_t)route;
      cap->bkt = cap->grab(b.bkt, (size_t)p.nkeys * sizeof(Ld), st);
    }
    return DVP_OK;
  }
  // the largest bucket goes to the host on the aux stream while the caller's stream carries on
  int read_max() const {
    DVP_TRY(ws->ensure_aux());
    DVP_HIP(hipEventRecord(ws->ev, st));
    DVP_HIP(hipStreamWaitEvent(ws->aux, ws->ev, 0));
    DVP_HIP(hipMemcpyAsync(ws->pinned, b.d_max, 4, hipMemcpyDeviceToHost, ws->aux));
    return DVP_OK;
  }
  // Round bookkeeping in one piece.  A pair round's counts, offsets and slot descriptors depend on the bucket COUNTS only, never on the
  // points, so all rounds are prepared at once -- arrays per round, four launches (k_mscan_*, k_round_desc_all) -- as soon as the sort
  // has its counts (cnt final on the caller's stream), and the rounds then follow each other back to back (three 5 us scan launches and a
  // descriptor kernel per round sit between them otherwise).  Where the four launches run (Tune::msm_round_pipeline):
  //   2 (default)  on the caller's stream, before the sort's last scatter;
  //   1            on a side stream beside that scatter (HBM-bound).  One proof at a time the two are equal within noise (bench.py's
  //                configuration: 21.0-21.2 ms either way; only with every proof on the NULL stream did the side stream measure
  //                0.1-0.17 ms better), and with two proofs in flight the side stream costs 1 ms per proof (21.0 against 19.4):
  //                its workgroups land in the OTHER proof's pair rounds.  NEVER beside this MSM's own first round: a round is an
  //                exact number of chip-fulls, and a few foreign workgroups holding wave slots when it is dispatched push some of
  //                its workgroups into an extra pass (measured: +0.4 ms per MSM).
  int prepare_rounds() const {
    if (!L.pipelined) return DVP_OK;
    const uint32_t nk = p.nkeys;
    hipStream_t bk = st;
    if (L.side_stream) {
      DVP_TRY(ws->ensure_side(1));
      DVP_HIP(hipEventRecord(ws->ev_pre, st));
      DVP_HIP(hipStreamWaitEvent(ws->side, ws->ev_pre, 0));
      bk = ws->side;
    }
    // (c_r, o_r), r = 1 .. ra_plan, in one three-launch scan (round 0's outputs included: its even-aligned buckets make the sorted
    // item list the descriptor array, and the scan of ceil(c_0 / 2) is that list's offsets halved), then every round's descriptors
    const uint32_t nb = cdiv(nk, SCAN_BLK);
    // (the caller's stream only: the side-stream flavour keeps the sort's own scan, padding and maximum)
    uint32_t* off0 = L.side_stream ? nullptr : b.off;
    DVP_LAUNCH(k_mscan_local, dim3(nb), dim3(SCAN_TPB), 0, bk, b.cnt, nk, L.ra_plan, b.rp, b.bsum2);
    DVP_LAUNCH(k_mscan_bsums, dim3(L.ra_plan), dim3(SCAN_TPB), 0, bk, b.bsum2, nb, nk, b.rp, off0, off0 ? b.d_max : (uint32_t*)nullptr);
    if (off0) DVP_TRY(read_max());  // the largest bucket is on its way to the host before the descriptors and the last scatter run
    DVP_LAUNCH(k_mscan_add, dim3(nb), dim3(SCAN_TPB), 0, bk, b.rp, b.bsum2, nk, L.ra_plan, (const uint32_t*)b.cnt, off0, b.items);
    DescPlan plan;
    for (int q = 0; q < 40; ++q) plan.at[q] = q < L.ra_plan ? L.desc_at[q] : 0;
    with_lpk((L.e_est >> 2) / nk /* round 1's outputs per bucket */, [&](auto lpk) {
      with_bool(L.dense, [&](auto dense) {
        constexpr int LPK = decltype(lpk)::value;
        DVP_LAUNCH((k_round_desc_all<LPK, decltype(dense)::value>), dim3(cdiv((size_t)nk * LPK, 1024)), dim3(1024), 0, bk, b.rp, nk, L.ra_plan, plan, b.gdesc);
      });
    });
    if (L.side_stream) DVP_HIP(hipEventRecord(ws->ev_side[0], ws->side));
    DVP_HIP(hipGetLastError());
    return DVP_OK;
  }
  // control words, recode, counting sort: the items of every bucket side by side (b.items, b.cnt, b.off) and the largest bucket on its
  // way to the host.  The all-rounds bookkeeping is enqueued as soon as the counts exist, before the last scatter.
  int sort() const {
    const FxBits fb = L.fb;
    const uint32_t nk = p.nkeys;
    ProfScope ps_sort(PROF_MSM_SORT, st);  // recode + counting sort
    // the control words [err | d_max, rest_n | err_out]: every MSM's tail kernel leaves err = ~0 and d_max = rest_n = 0 behind for the
    // next one (two memset nodes per MSM, ~6 us each plus their dispatch gaps, sat on the critical path); a fresh allocation, or a call
    // that returned before its tail kernel was enqueued, resets them here
    if (!ws->ctrl_clean) {
      DVP_HIP(hipMemsetAsync(b.err, 0xff, 8, st));
      DVP_HIP(hipMemsetAsync(b.err + 1, 0, 8, st));
    }
    ws->ctrl_clean = false;
    if (L.fused1)
      ;  // no entry words in HBM: both level-1 kernels recompute them
    else if (fx && fx->signed_digits)
      DVP_LAUNCH(k_recode_signed, dim3(cdiv(n, 256)), dim3(256), 0, st, scalars, inf, n, p.c, p.W, p.n_narrow, b.digits32, b.err);
    else if (fx)
      DVP_LAUNCH((k_recode<uint32_t>), dim3(cdiv(n, 256)), dim3(256), 0, st, scalars, inf, n, p.c, p.W, p.n_narrow, b.digits32, b.err);
    else
      DVP_LAUNCH((k_recode<uint16_t>), dim3(cdiv(n, 256)), dim3(256), 0, st, scalars, inf, n, p.c, p.W, p.n_narrow, b.digits, b.err);
    if (fx) {
      const uint32_t FX_NP = fb.np(), fx_nblk = L.fx_nblk, fx_nch = L.fx_nch;
      const uint32_t gmax = fx_nblk + FX_NP;  // upper bound on the number of level-2 chunks
      if (L.fused1)
        DVP_LAUNCH(k_part_hist_signed, dim3(fx_nblk), dim3(SORT_TPB), 0, st, scalars, inf, n, p.c, p.W, p.n_narrow, L.fx_S, fb, b.phist, b.err);
      else
        DVP_LAUNCH(k_part_hist, dim3(fx_nblk), dim3(SORT_TPB), 0, st, b.digits32, p.e_max, fb, b.phist);
      DVP_LAUNCH(k_part_scan_chunks, dim3(fx_nch), dim3(256), 0, st, b.phist, fx_nblk, fb, b.pbase, b.ctot, fx_nch);
      DVP_LAUNCH(k_part_scan_totals, dim3(cdiv((size_t)FX_NP * 64, 256)), dim3(256), 0, st, b.ctot, fx_nch, fb, b.pcount);
      DVP_LAUNCH(k_part_starts, dim3(1), dim3(FX_NP_MAX), 0, st, b.pcount, fb, b.pstart, b.cstart);
      const bool staged1 = FX_NP >= 64;           // few partitions: direct stores already coalesce
      const bool staged2 = fb.lo <= 10;           // one bin per thread in the block scan
      if (L.fused1 && staged1)
        DVP_LAUNCH(k_part_scatter_signed<true>, dim3(fx_nblk), dim3(SORT_TPB), FX_STAGE1_LDS, st, scalars, inf, n, p.c, p.W, p.n_narrow, L.fx_S,
                   fx->n_total, i0, fb, b.phist, b.pbase, b.ctot, fx_nch, b.pstart, b.plo, b.pid);
      else if (L.fused1)
        DVP_LAUNCH(k_part_scatter_signed<false>, dim3(fx_nblk), dim3(SORT_TPB), (2 * FX_NP_MAX + SORT_TPB) * 4, st, scalars, inf, n, p.c, p.W,
                   p.n_narrow, L.fx_S, fx->n_total, i0, fb, b.phist, b.pbase, b.ctot, fx_nch, b.pstart, b.plo, b.pid);
      else if (staged1)
        DVP_LAUNCH(k_part_scatter_staged, dim3(fx_nblk), dim3(SORT_TPB), FX_STAGE1_LDS, st, b.digits32, p.e_max, n, fx->n_total, i0, fb, b.phist,
                   b.pbase, b.ctot, fx_nch, b.pstart, b.plo, b.pid);
      else
        DVP_LAUNCH(k_part_scatter, dim3(fx_nblk), dim3(SORT_TPB), 0, st, b.digits32, p.e_max, n, fx->n_total, i0, fb, b.pbase, b.ctot, fx_nch,
                   b.pstart, b.plo, b.pid);
      DVP_LAUNCH(k_hist_local2, dim3(gmax), dim3(SORT_TPB), (1u << fb.lo) * 2, st, b.plo, b.pstart, b.cstart, fb, b.hist16);
      DVP_LAUNCH(k_hist_scan2, dim3(cdiv(nk, 256)), dim3(256), 0, st, b.hist16, b.cstart, fb, b.chunk_off, b.cnt);
      DVP_TRY(prepare_rounds());  // needs the counts only
      if (!L.sort_done_by_mscan()) DVP_TRY(scan_exclusive_pad2(b.cnt, b.off, nk, b.bsum, st));
      if (staged2)
        DVP_LAUNCH(k_scatter_local2_staged, dim3(gmax), dim3(SORT_TPB), FX_STAGE2_LDS, st, b.plo, b.pid, b.pstart, b.cstart, fb, b.off, b.chunk_off,
                   b.hist16, b.items);
      else
        DVP_LAUNCH(k_scatter_local2, dim3(gmax), dim3(SORT_TPB), (1u << fb.lo) * 4, st, b.plo, b.pid, b.pstart, b.cstart, fb, b.off, b.chunk_off, b.items);
    } else {
      const uint32_t nchunks = cdiv(n, SORT_CHUNK), nb = 1u << p.c;
      DVP_LAUNCH(k_hist_local, dim3(nchunks, p.W), dim3(SORT_TPB), (nb >> 1) * 4, st, b.digits, n, p.c, b.hist16);
      DVP_LAUNCH(k_hist_scan, dim3(cdiv(nk, 256)), dim3(256), 0, st, b.hist16, nchunks, p.c, p.W, b.chunk_off, b.cnt);
      DVP_TRY(prepare_rounds());  // needs the counts only
      if (!L.sort_done_by_mscan()) DVP_TRY(scan_exclusive_pad2(b.cnt, b.off, nk, b.bsum, st));
      DVP_LAUNCH(k_scatter_local, dim3(nchunks, p.W), dim3(SORT_TPB), nb * 4, st, b.digits, n, p.c, b.off, b.chunk_off, b.items);
    }
    ps_sort.stop();
    if (!L.sort_done_by_mscan()) {
      // odd buckets' NONE, the first round's counts / offsets (into the ring's next pair, where PairRounds::run(0) expects them) and the
      // largest bucket in one launch (d_max: zeroed by the previous MSM's tail kernel)
      DVP_LAUNCH(k_post_sort, dim3(cdiv(nk + 1, 256)), dim3(256), 0, st, b.items, b.cnt, b.off, nk, b.ntask, b.toff, b.d_max);
      DVP_TRY(read_max());
    }
    return DVP_OK;
  }
  // one level of the merge tree with G lanes per addition
  template <int G> void launch_merge(int j, uint32_t total, size_t lds, Ld* save0) const {
    with_bool(j == 0, [&](auto first) {
      DVP_LAUNCH((k_merge<G, decltype(first)::value>), dim3(cdiv((size_t)G * total, EC_TPB)), dim3(EC_TPB), lds, st, b.bkt, j, total, save0);
    });
  }
  // merge tree, Frobenius tail, final add tree: the result (and the control words for the next MSM) from the buckets
  void merge_and_tail(const MsmOut& out) const {
    ProfScope ps_tail(PROF_MSM_TAIL, st);
    const int merge_levels = fx ? fx->key_bits() : p.c;
    // bucket 0 (digits of magnitude 2^(c-1)) is kept aside by the first merge level, before it turns slot 0 into the total: k_tail weighs
    // it by 2^(c-1) (a 96-byte device-to-device copy node of its own cost 14 us per MSM)
    Ld* save0 = sign_mask ? b.tail + 2 * (size_t)p.c : nullptr;
    const uint32_t quad_max = tn.msm_quad_max > 0 ? (uint32_t)tn.msm_quad_max : MERGE_QUAD_MAX;
    const uint32_t hex_max = tn.msm_hex_max >= 0 ? (uint32_t)tn.msm_hex_max : MERGE_HEX_MAX;
    for (int j = 0; j < merge_levels; ++j) {
      const uint32_t total = (p.nkeys >> (j + 1)) * (uint32_t)(j + 1);
      const uint32_t group = total <= hex_max ? 16u : (total <= quad_max ? 4u : 1u);
      if (group == 16) launch_merge<16>(j, total, EC_LDS_Q, save0);
      else if (group == 4) launch_merge<4>(j, total, EC_LDS_Q, save0);
      else launch_merge<1>(j, total, EC_LDS, save0);
      if (cap && j < (int)CAPTURE_MAX_LEVELS) {  // the whole bucket array as this level left it; bucket 0 as level 0 kept it aside
        cap->hdr[CH_GROUP + j] = group;
        cap->levels[j] = cap->grab(b.bkt, (size_t)p.nkeys * sizeof(Ld), st);
        if (j == 0 && save0) cap->save0 = cap->grab(save0, sizeof(Ld), st);
        cap->nlevels = (uint32_t)j + 1;
      }
    }
    const int w_tail = fx ? 1 : p.W;  // fixed-base mode has a single bucket set
    const uint32_t cntT = (uint32_t)(w_tail * p.c);
    Ld* ta = b.tail;  // 2 * cntT entries: the two halves of k_tail's ping-pong
    uint32_t *o_xy = (uint32_t*)out.d_out_xy, *o_inf = (uint32_t*)out.d_out_inf;
    uint8_t* o_enc = (uint8_t*)out.d_out_enc;
    const int rule = o_enc ? dvp_codec_get_rule() : 0;
    uint32_t tail_shape = CT_FROBENIUS, nparts_cap = 0;
    if (sign_mask && tn.msm_hex_max != 0) {  // c points: one row of 16 lanes each
      tail_shape = CT_HEX_SIGNED;
      DVP_LAUNCH(k_tail<true>, dim3(1), dim3(EC_TPB), EC_LDS_Q, st, b.bkt, p.c, w_tail, -3, Tsq, ta, o_xy, o_inf, o_enc, rule, b.err, out.d_err_defer);
    } else if (!sign_mask && cntT > 32 && tn.msm_tail_groups != 0) {
      // many points (the one-shot MSM's W x c): group sums on cdiv(cntT, 16) workgroups first, then the single-workgroup tail on those
      Ld* part = b.tail + 2 * (size_t)cntT + 1;
      const int nparts = (int)cdiv(cntT, 16);
      DVP_LAUNCH(k_tail_groups, dim3(nparts), dim3(EC_TPB), EC_LDS_Q, st, b.bkt, p.c, w_tail, fx ? 0 : p.n_narrow, Tsq, ta, part);
      tail_shape = CT_GROUPS;
      nparts_cap = (uint32_t)nparts;
      if (cap) cap->parts = cap->grab(part, (size_t)nparts * sizeof(Ld), st);  // before k_tail's ping-pong overwrites them
      DVP_LAUNCH(k_tail<false>, dim3(1), dim3(EC_TPB), EC_LDS_Q, st, b.bkt, nparts, 1, -4, Tsq, part, o_xy, o_inf, o_enc, rule, b.err, out.d_err_defer);
    } else {
      if (sign_mask) tail_shape = CT_QUAD_SIGNED;
      DVP_LAUNCH(k_tail<false>, dim3(1), dim3(EC_TPB), EC_LDS_Q, st, b.bkt, p.c, w_tail, sign_mask ? -3 : (fx ? 0 : p.n_narrow), Tsq, ta, o_xy, o_inf,
                 o_enc, rule, b.err, out.d_err_defer);
    }
    if (cap) {  // what the last tail kernel wrote
      uint32_t* h = cap->hdr;
      h[CH_LEVELS] = (uint32_t)merge_levels; h[CH_TAIL] = tail_shape; h[CH_NPARTS] = nparts_cap; h[CH_ENC] = o_enc ? 1u : 0u; h[CH_RULE] = (uint32_t)rule;
      cap->res_xy = cap->grab(o_xy, 64, st);
      cap->res_inf = cap->grab(o_inf, 4, st);
      if (o_enc) cap->res_enc = cap->grab(o_enc, 30, st);
      cap->result = true;
    }
    ps_tail.stop();
  }
  // deferred completion: the workspace stays in use until this point of the stream; nothing here touches the host
  int complete_deferred() const {
    DVP_HIP(hipEventRecord(ws->ev_busy, st));
    ws->busy_stream = st;
    ws->busy_valid = true;
    return DVP_OK;
  }
  // the scalar-range flag is the only thing that needs the host: into the workspace's pinned words (a pageable destination makes the
  // runtime stage the copy and take a host round trip of its own between the two copies: 60 us per MSM)
  int complete(const MsmOut& out) const {
    volatile unsigned long long* h_err = (volatile unsigned long long*)(ws->pinned + 2);
    if (out.h_copy) DVP_HIP(hipMemcpyAsync(out.h_copy, out.d_copy, out.copy_bytes, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipMemcpyAsync((void*)h_err, b.err + 2, 8, hipMemcpyDeviceToHost, st));  // err_out
    DVP_HIP(hipStreamSynchronize(st));
    count_host_wait(0);
    const unsigned long long e = *h_err;
    if (e != ~0ull) {
      g_last_error_index = (int64_t)(e & 0xffffffffull);
      return DVP_EINVAL;
    }
    return DVP_OK;
  }
};

// whether a pair round takes its inversion once per workgroup (a pure host function; dvp_aff_share_plan exposes it to the tests).
// mode = Tune::msm_aff_share_inv, tpb = the rounds' workgroup size, planned = the additions the round plans (e_est >> (r + 1)),
// share_min = Tune::msm_aff_share_min, chip_full = resident threads x fewest slots per thread: the threshold when share_min is 0
static bool aff_share_plan(long long mode, uint32_t tpb, uint64_t planned, uint64_t share_min, uint64_t chip_full) {
  if (tpb != 128 && tpb != 256) return false;  // one wave: nothing to share with
  if (mode == 1) return true;
  if (mode != 2) return false;
  return planned >= (share_min ? share_min : chip_full);
}

// ---- bucket accumulation: batched-affine pair rounds while a round still carries >= aff_min additions, then the projective
// fan-in-K reducer on what is left (it has a short critical path and balances skew)
struct PairRounds {
  const MsmRun& m;
  uint32_t *pc[3], *po[3];  // ring of (counts, offsets): the sort's, then each stage's outputs
  int cur = 0;         // index of the live (cnt, off) pair
  const Aff* pts_in;   // the live points
  size_t cap;          // upper bound on the entries of the live array (incl. the even padding of the buckets)
  int launched = 0, ra = 0;  // rounds enqueued ahead of the largest-bucket read; rounds in all
  uint32_t max_cnt = 0;      // the largest bucket, as the sort left it
  uint32_t aff_tpb = 0, aff_lds = 0, aff_cap = 0, aff_bmax_only = 0, aff_bmax = 0, aff_bmin = 0, wt_cap = 0;
  unsigned long long* wt_buf = nullptr;  // the wave trace's buffer (wt_cap records), if one is set
  std::unique_lock<std::mutex> heavy;  // HeavyGate: held from the first pair round's enqueue to the last one's (released on every return)
  explicit PairRounds(const MsmRun& m_)
      : m(m_), pc{m_.b.cnt, m_.b.ntask, m_.b.cnt2}, po{m_.b.off, m_.b.toff, m_.b.off2}, pts_in(m_.bases0), cap(m_.p.e_max + m_.p.nkeys) {}
  // (rc(r), ro(r)) = counts / offsets of round r's INPUT under the all-rounds bookkeeping; round 0's are the sort's
  uint32_t* rc(int r) const { return r == 0 ? m.b.cnt : m.b.rp + (size_t)(2 * (r - 1)) * ((size_t)m.p.nkeys + 1); }
  uint32_t* ro(int r) const { return r == 0 ? m.b.off : m.b.rp + (size_t)(2 * (r - 1) + 1) * ((size_t)m.p.nkeys + 1); }
  int init() {
    const Tune& tn = m.tn;
    // resident threads of k_affine_round on this device (3 blocks of 256 per CU on MI355X: 196 608)
    int n_cu = 256, blk_per_cu = 3;
    DVP_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, m.dev));
    // workgroup size of the pair rounds (Tune::msm_aff_tpb): the kernel has no block-level synchronisation (LDS tables are per wave),
    // so smaller workgroups only change how soon a finished wave's slot is handed to the next workgroup
    aff_tpb = (tn.msm_aff_tpb == 64 || tn.msm_aff_tpb == 128 || tn.msm_aff_tpb == 256) ? (uint32_t)tn.msm_aff_tpb : (uint32_t)EC_TPB;
    // (with the exchange area of the shared inversion behind the table regions: 32 + 12 KB at 256 threads, still three workgroups per CU)
    aff_lds = (aff_tpb / 64) * GF_LDSK_BYTES_PER_WAVE + aff_exchange_bytes(aff_tpb / 64);
    // (asked of one instantiation for all of them: amdgpu_waves_per_eu(3, 3) pins every flavour -- first, later, dense, traced -- to three waves per SIMD)
    DVP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blk_per_cu, (const void*)k_affine_round<false, false>, (int)aff_tpb, aff_lds));
    if (blk_per_cu < 1) blk_per_cu = 1;
    aff_cap = (uint32_t)n_cu * (uint32_t)blk_per_cu * aff_tpb;
    aff_bmax_only = tn.msm_aff_bmax >= 1 && tn.msm_aff_bmax <= 255 ? (uint32_t)tn.msm_aff_bmax : AFF_BMAX;
    aff_bmin = tn.msm_aff_bmin >= 1 && (uint32_t)tn.msm_aff_bmin <= aff_bmax_only ? (uint32_t)tn.msm_aff_bmin : 1u;
    aff_bmax = aff_bmax_only | (aff_bmin << 8);
    wave_trace_snapshot(&wt_buf, &wt_cap);  // one snapshot per MSM: every round of it traces into the same buffer or none does
    return DVP_OK;
  }
  // round r: its bookkeeping where that is per round, then the round itself over d_total = the scanned output count (ooff[nkeys]) and
  // dsc = one (a, b) descriptor per output slot
  int run(int r) {
    const MsmLayout& L = m.L;
    const MsmBuffers& b = m.b;
    const uint32_t nk = m.p.nkeys;
    hipStream_t st = m.st;
    const int nxt = (cur + 1) % 3;
    const uint32_t *d_total, *dsc = r == 0 ? b.items : b.gdesc;
    if (L.pipelined) {  // r < ra_plan always (ra <= ra_plan); everything a round needs was prepared behind the sort
      if (r == 0 && L.side_stream) DVP_HIP(hipStreamWaitEvent(st, m.ws->ev_side[0], 0));
      d_total = ro(r + 1) + nk;
      if (r > 0) dsc = b.gdesc + L.desc_at[r];
    } else {
      // (r == 0: cur == 0 and k_post_sort has left the first round's counts / offsets in pc[1] / po[1] -- an MSM that is not pipelined
      // always runs it.)  r > 0: counts / offsets of the round's outputs from those of its inputs, and its slot descriptors
      if (r > 0) {
        DVP_TRY(scan_exclusive_div(pc[cur], 2u, pc[nxt], po[nxt], nk, b.bsum, st));
        with_lpk((L.e_est >> (r + 1)) / nk, [&](auto lpk) {
          constexpr int LPK = decltype(lpk)::value;
          DVP_LAUNCH((k_round_desc<LPK>), dim3(cdiv((size_t)nk * LPK, 256)), dim3(256), 0, st, pc[cur], po[cur], po[nxt], nk, b.gdesc);
        });
      }
      d_total = po[nxt] + nk;
    }
    const size_t out_max = cap / 2 + nk + 1;
    Aff* outp = (r & 1) ? b.affB : b.affA;
    // grid: upper bound on the threads the device-side choice of B can ask for (R chip-fulls, see k_affine_round)
    const uint32_t r_max = cdiv(cdiv(out_max, aff_cap), aff_bmax_only);
    const uint32_t grid = r_max * (aff_cap / aff_tpb) + 1;
    // r == 0 is the dominant kernel (it gathers the bases) and is timed launch by launch; the later rounds share ONE scope (finish()):
    // an event pair around every round put ~10 us of packet processing between two rounds that otherwise follow each other back to
    // back (kernel trace: 10-13 us gaps after every round, none between the merge levels)
    const bool share = aff_share_plan(m.tn.msm_aff_share_inv, aff_tpb, (uint64_t)(L.e_est >> (r + 1)),
                                      m.tn.msm_aff_share_min > 0 ? (uint64_t)m.tn.msm_aff_share_min : 0, (uint64_t)aff_cap * aff_bmin);
    const uint32_t bmax_arg = aff_bmax | (share ? AFF_SHARE_INV : 0u);
    ProfScope ps0(r == 0 ? PROF_MSM_ACCUM_AFFINE : -1, st, (uint64_t)m.n);
    WaveTrace wt{wt_buf, wt_cap, g_wave_trace_tag.fetch_add(wt_buf ? 1u : 0u)};
    with_bool(r == 0, [&](auto first) {
      with_bool(wt.buf != nullptr, [&](auto trace) {
        with_bool(r > 0 && L.dense, [&](auto dense) {
          constexpr bool FIRST = decltype(first)::value, TRACE = decltype(trace)::value, DENSE = decltype(dense)::value;
          if constexpr (!(FIRST && DENSE))  // a first round is never dense: no such kernel
            DVP_LAUNCH((k_affine_round<FIRST, TRACE, DENSE>), dim3(grid), dim3(aff_tpb), aff_lds, st, pts_in, (const uint2*)(const void*)dsc, d_total,
                       aff_cap, bmax_arg, m.Tsq, b.prefix, outp, FIRST ? m.sign_mask : 0u, wt);
        });
      });
    });
    ps0.stop();
    if (r > 0) count_later_round(L.dense);
    count_round_inv(share);
    if (MsmCapture* c = m.cap; c && r < (int)CAPTURE_MAX_ROUNDS) {
      // the round's output counts / offsets, its descriptors as the kernel read them (round 0: the item list, captured behind the sort)
      // and its output points, before round r + 1 reuses the descriptors (per-round bookkeeping) and round r + 2 the points; each
      // region at the bound the workspace gives it
      const bool dense_r = r > 0 && L.dense;
      const size_t pts_n = std::min(out_max, (r & 1) ? L.affB_n : L.affA_n);
      const size_t desc_n = r == 0 ? 0 : (L.pipelined ? (dense_r ? 2 : 1) * (out_max + 64) : std::min(out_max, L.desc_n));
      MsmCapture::Round& cr = c->rounds[r];
      cr.ocnt = c->grab(L.pipelined ? rc(r + 1) : pc[nxt], (size_t)nk * 4, st);
      cr.ooff = c->grab(L.pipelined ? ro(r + 1) : po[nxt], ((size_t)nk + 1) * 4, st);
      cr.desc = c->grab(dsc, desc_n * 4, st);
      cr.pts = c->grab(outp, pts_n * sizeof(Aff), st);
      c->hdr[CH_SHARE + r] = share ? 1u : 0u;
      c->nrounds = (uint32_t)r + 1;
    }
    pts_in = outp;
    cap = out_max;
    if (!L.pipelined) cur = nxt;
    return DVP_OK;
  }
  // The number of rounds depends on the largest bucket, which only the device knows.  When the average bucket already
  // holds >= 4 entries the first round is certain to be needed, so it is enqueued BEFORE the host waits for that number:
  // the round trip (and the launch ramp after it) hides behind ~5 ms of round 0 instead of idling the GPU mid-MSM.
  int begin() {
    const MsmLayout& L = m.L;
    if (m.ws_slots > 1 && L.affine_mode) {
      HeavyGate& hg = g_heavy[m.dev];
      heavy = std::unique_lock<std::mutex>(hg.mu);
      if (hg.last && hg.last != m.ws->ev_heavy) DVP_HIP(hipStreamWaitEvent(m.st, hg.last, 0));
    }
    if (L.affine_mode && (L.e_est >> 1) >= L.aff_min && L.e_est >= 4 * (size_t)m.p.nkeys) {
      DVP_TRY(run(0));
      launched = 1;
    }
    DVP_HIP(hipStreamSynchronize(m.ws->aux));  // the caller's stream keeps running round 0 meanwhile
    count_host_wait(launched ? 1 : 0);
    max_cnt = *m.ws->pinned;
    if (L.affine_mode)
      while (((uint64_t)1 << ra) < max_cnt && (L.e_est >> (ra + 1)) >= L.aff_min) ++ra;
    if (ra < launched) ra = launched;  // a first round over single-entry buckets only passes them through
    return DVP_OK;
  }
  int gate_event() {
    DVP_HIP(hipEventRecord(m.ws->ev_heavy, m.st));
    g_heavy[m.dev].last = m.ws->ev_heavy;
    return DVP_OK;
  }
  // the rounds begin() did not enqueue; afterwards (pc[cur], po[cur], pts_in, cap) describe what the rounds left
  int finish() {
    // the gate's event goes after the last round that still fills the chip several times over (>= Tune::msm_gate_min additions):
    // the late rounds are latency-bound and are exactly what the next MSM's first round should overlap
    int r_evt = -1;
    if (heavy.owns_lock() && ra > 0) {
      const size_t gate_min = m.tn.msm_gate_min > 0 ? (size_t)m.tn.msm_gate_min : 1;
      r_evt = 0;
      while (r_evt + 1 < ra && (m.L.e_est >> (r_evt + 2)) >= gate_min) ++r_evt;
    }
    if (r_evt >= 0 && r_evt < launched) DVP_TRY(gate_event());
    int r = launched;
    if (r == 0 && ra > 0) {  // (small MSMs: the first round was not enqueued ahead of the largest-bucket read)
      DVP_TRY(run(0));
      if (r_evt == 0) DVP_TRY(gate_event());
      r = 1;
    }
    ProfScope ps_rest(ra > r ? PROF_MSM_AFFINE_REST : -1, m.st, (uint64_t)(ra > r ? ra - r : 0));
    for (; r < ra; ++r) {
      DVP_TRY(run(r));
      if (r == r_evt) DVP_TRY(gate_event());
    }
    ps_rest.stop();
    if (m.L.pipelined) {
      // what the rounds left is described by the arrays of round `ra`: they head the ring of three the reducer works in
      // (a pipelined MSM always starts its first round early, so the side stream's bookkeeping has been waited for)
      pc[0] = rc(ra);
      po[0] = ro(ra);
      cur = 0;
    }
    if (heavy.owns_lock()) heavy.unlock();
    return DVP_OK;
  }
};

// what the pair rounds left, down to one point per bucket (b.bkt), by one of three routes
int MsmRun::reduce_leftovers(const PairRounds& pr) const {
  const uint32_t nk = p.nkeys;
  uint32_t *const *pc = pr.pc, *const *po = pr.po;
  int cur = pr.cur;
  const uint64_t rem_max = ((uint64_t)pr.max_cnt + ((uint64_t)1 << pr.ra) - 1) >> pr.ra;  // largest bucket after the affine rounds
  if (rem_max <= 1) {
    if (pr.ra == 0)
      DVP_LAUNCH(k_bucket_gather_items, dim3(cdiv(nk, 256)), dim3(256), 0, st, bases0, b.items, b.cnt, b.off, nk, b.bkt, sign_mask);
    else
      DVP_LAUNCH(k_bucket_gather_aff, dim3(cdiv(nk, 256)), dim3(256), 0, st, pr.pts_in, pc[cur], po[cur], nk, b.bkt);
    return leftovers_done(pr.ra == 0 ? CR_GATHER_ITEMS : CR_GATHER_AFF);
  }
  if (pr.ra > 0 && rem_max <= (uint64_t)(tn.msm_bucket_pairs_max >= 0 ? tn.msm_bucket_pairs_max : 0)) {
    // a handful of points per bucket left: one thread per bucket; buckets that meet an exceptional pair are redone from a list
    DVP_LAUNCH(k_bucket_pairs, dim3(cdiv(nk, EC_TPB)), dim3(EC_TPB), EC_LDS, st, pr.pts_in, pc[cur], po[cur], nk, b.bkt, b.rest_n, b.rest_list);
    DVP_LAUNCH(k_bucket_rest, dim3(cdiv(nk, EC_TPB)), dim3(EC_TPB), EC_LDS, st, pr.pts_in, pc[cur], po[cur], b.rest_n, b.rest_list, b.bkt);
    return leftovers_done(CR_BUCKET_PAIRS);
  }
  // the fan-in-K reducer.  Level 1: mixed additions from affine inputs (IND: the items index the bases; else the pair rounds' outputs)
  int nxt = (cur + 1) % 3;
  DVP_TRY(scan_exclusive_div(pc[cur], p.K, pc[nxt], po[nxt], nk, b.bsum, st));
  size_t tmax = pr.cap / p.K + nk + 1;
  const size_t accum_quad_max = tn.msm_accum_quad_max > 0 ? (size_t)tn.msm_accum_quad_max : ACCUM_QUAD_MAX;
  const size_t accum_hex_max = tn.msm_accum_hex_max >= 0 ? (size_t)tn.msm_accum_hex_max : ACCUM_HEX_MAX;
  // tmax is an upper bound on the tasks (the real count sits on the device); quads when even the bound fits one chip-full
  // (the rest list holds task numbers: tmax of them at most, and rest_cap is sized from tmax at its largest, so the list always fits;
  // the comparison stays as the bound's witness.  Tune::msm_accum_fast = 0: the general kernel)
  const bool accum_fast = tn.msm_accum_fast != 0 && tmax <= L.rest_cap;
  ProfScope ps0(pr.ra == 0 ? PROF_MSM_ACCUM_AFFINE : -1, st);  // small inputs: no pair rounds, this is the dominant kernel
  with_bool(pr.ra == 0, [&](auto ind) {
    with_bool(tmax <= accum_quad_max, [&](auto quad) {
      constexpr bool IND = decltype(ind)::value, QUAD = decltype(quad)::value;
      const dim3 grid(cdiv((QUAD ? 4 : 1) * tmax, EC_TPB)), grid1(cdiv(tmax, EC_TPB));
      const size_t lds = QUAD ? EC_LDS_Q : EC_LDS;
      if (accum_fast) {
        DVP_LAUNCH((k_accum_affine_fast<IND, QUAD>), grid, dim3(EC_TPB), lds, st, pr.pts_in, b.items, pc[cur], po[cur], po[nxt], nk, p.K, b.bufA,
                   sign_mask, b.rest_n, b.rest_list);
        DVP_LAUNCH((k_accum_affine_rest<IND>), grid1, dim3(EC_TPB), EC_LDS, st, pr.pts_in, b.items, pc[cur], po[cur], po[nxt], nk, p.K, b.bufA,
                   sign_mask, b.rest_n, b.rest_list);
      } else
        DVP_LAUNCH((k_accum_affine<IND, QUAD>), grid, dim3(EC_TPB), lds, st, pr.pts_in, b.items, pc[cur], po[cur], po[nxt], nk, p.K, b.bufA, sign_mask);
    });
  });
  ps0.stop();
  cur = nxt;
  size_t cap = tmax;
  Ld *in = b.bufA, *outb = b.bufB;
  for (uint64_t left = (rem_max + p.K - 1) / p.K; left > 1; left = (left + p.K - 1) / p.K) {
    nxt = (cur + 1) % 3;
    DVP_TRY(scan_exclusive_div(pc[cur], p.K, pc[nxt], po[nxt], nk, b.bsum, st));
    tmax = cap / p.K + nk + 1;
    // the LAST level of a small MSM (every bucket ends with one task of at most K partial sums, typically one or two): rows of 16
    // lanes when the tasks fit ACCUM_HEX_MAX (measured at 2^16 points)
    if (left <= p.K && tmax <= accum_hex_max)
      DVP_LAUNCH(k_accum_proj<16>, dim3(cdiv(16 * tmax, EC_TPB)), dim3(EC_TPB), EC_LDS_Q, st, in, pc[cur], po[cur], po[nxt], nk, p.K, outb);
    else if (tmax <= accum_quad_max)
      DVP_LAUNCH(k_accum_proj<4>, dim3(cdiv(4 * tmax, EC_TPB)), dim3(EC_TPB), EC_LDS_Q, st, in, pc[cur], po[cur], po[nxt], nk, p.K, outb);
    else
      DVP_LAUNCH(k_accum_proj<1>, dim3(cdiv(tmax, EC_TPB)), dim3(EC_TPB), EC_LDS, st, in, pc[cur], po[cur], po[nxt], nk, p.K, outb);
    cap = tmax;
    cur = nxt;
    std::swap(in, outb);
  }
  DVP_LAUNCH(k_bucket_gather, dim3(cdiv(nk, 256)), dim3(256), 0, st, in, pc[cur], po[cur], nk, b.bkt);
  return leftovers_done(accum_fast ? CR_REDUCER_FAST : CR_REDUCER_GENERAL);
}

// n == 0: the point at infinity.  The two flavours differ on purpose: the deferred one must not touch the host.
static int msm_empty(const MsmOut& out, hipStream_t st) {
  DVP_HIP(hipMemsetAsync(out.d_out_xy, 0, 64, st));
  if (out.d_out_enc) DVP_HIP(hipMemsetAsync(out.d_out_enc, 0, 30, st));
  if (out.d_err_defer) {
    DVP_HIP(hipMemsetAsync(out.d_out_inf, 0, 4, st));
    DVP_HIP(hipMemsetAsync(out.d_out_inf, 1, 1, st));  // little-endian u32 1
    DVP_HIP(hipMemsetAsync(out.d_err_defer, 0xff, 8, st));
    return DVP_OK;
  }
  if (out.h_copy) DVP_HIP(hipMemcpyAsync(out.h_copy, out.d_copy, out.copy_bytes, hipMemcpyDeviceToHost, st));
  uint32_t one = 1;
  DVP_HIP(hipMemcpyAsync(out.d_out_inf, &one, 4, hipMemcpyHostToDevice, st));
  DVP_HIP(hipStreamSynchronize(st));
  return DVP_OK;
}

// fx == nullptr: one-shot MSM over (d_scalars, d_bases).  fx != nullptr: fixed-base mode, the scalars
// d_scalars[0..n) belong to bases i0 .. i0+n of the pre-rotated table and d_inf is already offset by i0.
static int msm_core(const void* d_scalars, const void* d_bases, const void* d_inf, size_t n, const MsmFixedCtx* fx, uint32_t i0, const MsmOut& out,
                    hipStream_t st) {
  if (n == 0) return msm_empty(out, st);
  if (n > (1u << 27)) return DVP_EINVAL;
  MsmRun m{(const uint32_t*)d_scalars, (const uint8_t*)d_inf, fx ? fx->table : (const Aff*)d_bases, n, fx, i0, (fx && fx->signed_digits) ? ITEM_NEG : 0u, st};
  m.p = msm_plan(n, fx);
  {  // entry positions and pre-rotated table indices are 32-bit (0xffffffff = "no partner" in a slot descriptor)
    const uint64_t tab = fx ? (uint64_t)fx->rows() * fx->n_total : (uint64_t)n;
    if ((uint64_t)m.p.e_max >= 0xfffffff0ull || tab >= (m.sign_mask ? 0x7ffffff0ull : 0xfffffff0ull)) return DVP_EINVAL;
  }
  DVP_HIP(hipGetDevice(&m.dev));
  if (m.dev < 0 || m.dev >= DVP_MAX_DEVICES) return DVP_EINVAL;
  DVP_TRY(msm_set_lds_limits(m.dev));
  m.tn = tune();
  m.ws_slots = m.tn.msm_ws_slots >= 1 && m.tn.msm_ws_slots <= MSM_WS_SLOTS ? (int)m.tn.msm_ws_slots : 1;
  m.L = msm_layout(n, m.p, fx, m.tn);
  std::unique_lock<std::mutex> g;  // the workspace is this call's until it returns
  DVP_TRY(msm_acquire_workspace(m.dev, st, m.ws_slots, m.L.bytes, g, &m.ws));
  m.b = msm_carve(n, m.p, fx, m.L, m.ws->p);
  if (g_capture.armed) {  // a test armed this thread's stage capture: this MSM is the one it takes
    m.cap = &g_capture;
    m.cap->armed = false;
    m.cap->dev = m.dev;
    m.cap->st = st;
  }
  ProfScope ps_total(PROF_MSM_TOTAL, st);
  DVP_TRY(m.sort());
  if (MsmCapture* c = m.cap) {  // the sort's result; the rounds only read it (a first round the sort's stage did not wait for included)
    c->cnt = c->grab(m.b.cnt, (size_t)m.p.nkeys * 4, st);
    c->off = c->grab(m.b.off, ((size_t)m.p.nkeys + 1) * 4, st);
    c->items = c->grab(m.b.items, (m.p.e_max + (size_t)m.p.nkeys + 2) * 4, st);
  }
  DVP_TRY(gf_sqr_tables(&m.Tsq, st));
  PairRounds pr(m);
  DVP_TRY(pr.init());
  DVP_TRY(pr.begin());   // the first round where it is certain, then the host learns the largest bucket and settles the number of rounds
  DVP_TRY(pr.finish());  // the other rounds
  DVP_TRY(m.reduce_leftovers(pr));
  if (MsmCapture* c = m.cap) {
    uint32_t* h = c->hdr;
    h[CH_MAGIC] = CAPTURE_MAGIC; h[CH_VERSION] = CAPTURE_VERSION; h[CH_HDR_WORDS] = CAPTURE_HDR_WORDS;
    h[CH_FLAVOUR] = (fx ? 1u : 0u) | ((fx && fx->signed_digits) ? 2u : 0u);
    h[CH_C] = (uint32_t)m.p.c; h[CH_W] = (uint32_t)m.p.W; h[CH_N_NARROW] = (uint32_t)m.p.n_narrow; h[CH_NKEYS] = m.p.nkeys;
    h[CH_SIGN_MASK] = m.sign_mask; h[CH_N_TOTAL] = fx ? fx->n_total : (uint32_t)n; h[CH_I0] = i0; h[CH_N] = (uint32_t)n;
    h[CH_RA] = (uint32_t)pr.ra; h[CH_RA_PLAN] = (uint32_t)m.L.ra_plan; h[CH_DENSE] = m.L.dense ? 1u : 0u;
    h[CH_PIPELINE] = m.L.pipelined ? (m.L.side_stream ? 1u : 2u) : 0u;
    h[CH_TPB] = pr.aff_tpb; h[CH_AFF_CAP] = pr.aff_cap; h[CH_BMAX] = pr.aff_bmax_only; h[CH_BMIN] = pr.aff_bmin;
    h[CH_K] = m.p.K; h[CH_MAX_CNT] = pr.max_cnt;
    c->taken = true;
  }
  m.merge_and_tail(out);
  ps_total.stop();
  DVP_HIP(hipGetLastError());
  m.ws->ctrl_clean = true;  // the tail kernel is enqueued: it resets the control words
  return out.d_err_defer ? m.complete_deferred() : m.complete(out);
}

// d_pts: n affine points `pt_stride_bytes` apart (>= 64, a multiple of 16), d_inf32: n flags (u32, `inf_stride` words apart) -> their sum
int msm_sum_points_dev(const void* d_pts, uint32_t pt_stride_bytes, const void* d_inf32, uint32_t n, uint32_t inf_stride, void* d_out_xy,
                       void* d_out_inf, hipStream_t st) {
  GfSqrTables Tsq;
  DVP_TRY(gf_sqr_tables(&Tsq, st));
  DVP_LAUNCH(k_sum_points, dim3(1), dim3(64), GF_LDS_BYTES_PER_WAVE, st, (const char*)d_pts, pt_stride_bytes, (const uint32_t*)d_inf32, n,
                     inf_stride, Tsq, (uint32_t*)d_out_xy, (uint32_t*)d_out_inf);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

// the join of a mixed MSM (k_join_points), enqueued on `st`: d_a / d_b = the two partial points, each with its u32 infinity flag and
// its scalar-range word; d_out_enc (optional) receives the sum's 30-byte encoding, d_err_out the merged range word
int msm_join_points_dev(const void* d_a_xy, const void* d_a_inf, const unsigned long long* d_a_err, const void* d_b_xy, const void* d_b_inf,
                        const unsigned long long* d_b_err, uint32_t covered, void* d_out_xy, void* d_out_inf, void* d_out_enc,
                        unsigned long long* d_err_out, hipStream_t st) {
  GfSqrTables Tsq;
  DVP_TRY(gf_sqr_tables(&Tsq, st));
  DVP_LAUNCH(k_join_points, dim3(1), dim3(64), GF_LDS_BYTES_PER_WAVE, st, (const Aff*)d_a_xy, (const uint32_t*)d_a_inf, d_a_err, (const Aff*)d_b_xy,
                     (const uint32_t*)d_b_inf, d_b_err, covered, Tsq, (uint32_t*)d_out_xy, (uint32_t*)d_out_inf, (uint8_t*)d_out_enc,
                     d_out_enc ? dvp_codec_get_rule() : 0, d_err_out);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

int msm_affine_dev(const void* d_scalars, const void* d_bases, const void* d_inf, size_t n, const MsmOut& out, hipStream_t st) {
  return msm_core(d_scalars, d_bases, d_inf, n, nullptr, 0, out, st);
}

// ---- fixed-base contexts (the prover's SRS vectors) -----------------------------------------------
// range_hint = number of bases a typical call will cover (the per-GPU shard): the shared window size c
// minimises an empirical cost in field multiplications (pair additions + a per-bucket term, see below)
// Table flavours: the default is aligned windows of SIGNED binary digits over W rows 2^(o_w) P (768 B per base at W = 12: 4.8 GB for
// both SRS vectors of a 2^20-constraint prover); DVP_MSM_ALIGNED_SIGNED = 0 selects round 1-2's aligned tau-adic windows over rows
// tau^(o_w) P instead (one window and twice the buckets more: 24.6 against 23.5 ms per proof in round 3) -- kept because it shares
// its recode, merge and Frobenius tail with the one-shot MSM and is the independent cross-check of the signed flavour in the tests.
// window size, window count and sort split of a context that typically serves `range_hint` bases per call -- everything about a
// context that does not need the device (the table-budget planner reads the row count from here)
static void msm_fixed_settle(MsmFixedCtx* c, size_t range_hint) {
  double best = 1e300;
  int best_c = 8;
  const bool signed_aligned = tune().msm_aligned_signed != 0;
  // pair additions at ~5.6 product-equivalents + a per-bucket term for merge/reducer/sort; measured on MI355X at 2^20
  // constraints: 2^18 buckets beat 2^16, 2^17, 2^19 and 2^20 for every shard from 0.26 M to 4.2 M pairs of the tau-adic aligned
  // windows (2^20 wins from ~8 M pairs); the signed windows run the same model over their own entry and bucket counts
  // (ceil(234 / c) entries, 2^(c-1) buckets)
  // entries per scalar (windows that carry digits) and key bits -> cost
  auto cost_of = [range_hint](int windows, int kb) {
    return (double)windows * (double)range_hint * 5.6 + 10.0 * (double)(1u << kb) + (kb > 18 ? 25.0 * (double)((1u << kb) - (1u << 18)) : 0.0);
  };
  const int c_top = signed_aligned ? FX_C_MAX + 1 : FX_C_MAX;
  for (int cc = 8; cc <= c_top; ++cc) {
    MsmFixedCtx probe;
    if (signed_aligned) probe.set_c_signed(cc);
    if (signed_aligned && probe.c != cc) continue;  // all windows narrow: the same plan as cc - 1
    const double cost = signed_aligned ? cost_of(probe.W, cc - 1) : cost_of((234 + cc - 1) / cc, cc);
    if (cost < best) { best = cost; best_c = cc; }
  }
  if (tune().msm_fixed_c >= 8 && tune().msm_fixed_c <= c_top) best_c = (int)tune().msm_fixed_c;
  if (signed_aligned) c->set_c_signed(best_c); else c->set_c(best_c);
  const int kb = c->key_bits();
  c->hi_bits = kb / 2;  // even split: both levels have <= 2^10 bins and use the LDS-staged scatters
  if (int h = (int)tune().fx_hi; h >= 0 && h <= 10 && kb - h <= 15 && kb - h >= 1) c->hi_bits = h;
}
// rows of the table msm_fixed_build would settle on for a context of `count` bases used whole (range_hint = count)
int msm_fixed_rows_for(size_t count) {
  MsmFixedCtx probe;
  msm_fixed_settle(&probe, count);
  return probe.rows();
}
static int msm_fixed_build(const Aff* d_bases, uint32_t n_total, size_t range_hint, MsmFixedCtx** out, hipError_t* alloc_err) {
  MsmFixedCtx* c = new MsmFixedCtx();
  c->n_total = n_total;
  msm_fixed_settle(c, range_hint);
  // DVP_MSM_TABLE_REFUSE = 1 (tests): as if the runtime had refused the table, without asking it
  hipError_t e = tune().msm_table_refuse == 1 ? hipErrorOutOfMemory : hipMalloc((void**)&c->table, (size_t)c->rows() * n_total * sizeof(Aff));
  *alloc_err = e;
  if (e == hipSuccess) {
    if (c->signed_digits) {
      GfSqrTables Tsq;
      int rc_t = gf_sqr_tables(&Tsq, 0);
      if (rc_t != DVP_OK) { msm_fixed_destroy(c); return rc_t; }
      e = hipFuncSetAttribute((const void*)k_dbl_table, hipFuncAttributeMaxDynamicSharedMemorySize, EC_LDS);
      Gf* scratch = nullptr;  // Z snapshots + prefix products of the shared inversion, (W - 1) x n each
      const size_t per = (size_t)(c->W > 1 ? c->W - 1 : 1) * n_total;
      if (e == hipSuccess) e = hipMalloc((void**)&scratch, 2 * per * sizeof(Gf));
      if (e == hipSuccess) {
        DVP_LAUNCH(k_dbl_table, dim3(cdiv(n_total, 256)), dim3(256), EC_LDS, 0, d_bases, n_total, c->c, c->W, c->n_narrow, Tsq, c->table,
                           scratch, scratch + per);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
      }
      if (scratch) (void)hipFree(scratch);
    } else
      DVP_LAUNCH(k_frob_table, dim3(cdiv(n_total, 256)), dim3(256), 0, 0, d_bases, n_total, c->c, c->W, c->n_narrow, c->table);
    if (e == hipSuccess) e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    c->table = *alloc_err == hipSuccess ? c->table : nullptr;
    msm_fixed_destroy(c);
    return hip_fail(e, "msm_fixed_create", __FILE__, __LINE__);  // DVP_ENOMEM for a refused table or scratch allocation
  }
  *out = c;
  return DVP_OK;
}
int msm_fixed_create(const Aff* d_bases, uint32_t n_total, size_t range_hint, MsmFixedCtx** out) {
  if ((uint64_t)n_total * 32 >= 0xfffffff0ull) return DVP_EINVAL;  // W <= 31 windows of pre-rotated copies, 32-bit indices
  hipError_t alloc_err = hipSuccess;
  return msm_fixed_build(d_bases, n_total, range_hint, out, &alloc_err);
}
int msm_fixed_info(const MsmFixedCtx* c, int* cbits, int* windows) {
  if (!c) return DVP_EINVAL;
  *cbits = c->c;
  *windows = c->W;
  return DVP_OK;
}
// bytes of the pre-rotated table; *signed_flavour = 1 for the signed binary windows (the default), 0 for the tau-adic aligned windows
const void* msm_fixed_table_ptr(const MsmFixedCtx* c) { return c ? (const void*)c->table : nullptr; }
uint64_t msm_fixed_table_bytes(const MsmFixedCtx* c, int* signed_flavour) {
  if (signed_flavour) *signed_flavour = c && c->signed_digits ? 1 : 0;
  return c ? (uint64_t)c->rows() * c->n_total * sizeof(Aff) : 0;
}
void msm_fixed_destroy(MsmFixedCtx* c) {
  if (!c) return;
  if (c->table) (void)hipFree(c->table);
  delete c;
}
// partial sum over bases [lo, hi) of the context; d_scalars / d_inf point at element lo (what `out` may ask for: host_api.h, MsmOut)
int msm_fixed_dev(const MsmFixedCtx* c, const void* d_scalars, const void* d_inf, uint32_t lo, uint32_t hi, const MsmOut& out, hipStream_t st) {
  if (!c || lo > hi || hi > c->n_total) return DVP_EINVAL;
  return msm_core(d_scalars, nullptr, d_inf, hi - lo, c, lo, out, st);
}

}  // namespace dvp

using namespace dvp;

// the pair rounds' choice between one inversion per workgroup and one per wave (include/dvpari_internal.h)
extern "C" int dvp_aff_share_plan(long long mode, uint32_t tpb, uint64_t planned, uint64_t share_min, uint64_t chip_full) {
  return aff_share_plan(mode, tpb, planned, share_min, chip_full) ? 1 : 0;
}

// ---- the table-budget planner (include/dvpari_internal.h: dvp_table_plan) ------------------------------------------------------
// largest count <= total whose table -- rows x count x 64 bytes, rows as msm_fixed_build settles them for THAT count -- fits `budget`;
// 0 when that is fewer than fixed_min bases.  rows(count) only falls as count grows (more bases favour wider windows), so from an
// upper bound the iteration n <- budget / (64 rows(n)) comes down onto the largest fixed point; the final test holds whatever
// rows() does.
static size_t table_max_prefix(size_t total, uint64_t budget, size_t fixed_min, uint64_t* bytes) {
  *bytes = 0;
  if (total == 0 || total < fixed_min || total >= ((size_t)1 << 27)) return 0;
  size_t n = total;
  for (int it = 0; it < 64 && n > 0; ++it) {
    const uint64_t per = (uint64_t)msm_fixed_rows_for(n) * sizeof(Aff);
    const uint64_t fit = budget / per;
    if (fit >= n) break;
    n = (size_t)fit;
  }
  while (n > 0 && (uint64_t)msm_fixed_rows_for(n) * n * sizeof(Aff) > budget) --n;  // never taken when rows() is monotone
  if (n < fixed_min || n == 0) return 0;
  *bytes = (uint64_t)msm_fixed_rows_for(n) * n * sizeof(Aff);
  return n;
}
extern "C" int dvp_table_plan(size_t size0, size_t size1, uint64_t budget_bytes, size_t covered[2], uint64_t bytes[2]) {
  if (!covered || !bytes) return DVP_EINVAL;
  const size_t fixed_min = (size_t)(tune().msm_fixed_min > 0 ? tune().msm_fixed_min : 1);
  covered[0] = 0;
  bytes[0] = 0;
  covered[1] = table_max_prefix(size1, budget_bytes, fixed_min, &bytes[1]);  // the K MSM (4m terms) first
  // the commitment MSM only once the K MSM is served whole (or takes no table at any budget): at most one of the two is partly covered
  if (covered[1] == size1 || size1 < fixed_min || size1 >= ((size_t)1 << 27))
    covered[0] = table_max_prefix(size0, budget_bytes - bytes[1], fixed_min, &bytes[0]);
  return DVP_OK;
}

extern "C" int dvp_msm_affine_dev(const void* d_scalars, const void* d_bases_xy, const void* d_bases_inf, size_t n,
                                  void* d_out_xy, void* d_out_inf, void* stream) {
  if ((n && (!d_scalars || !d_bases_xy)) || !d_out_xy || !d_out_inf) return DVP_EINVAL;
  return msm_affine_dev(d_scalars, d_bases_xy, d_bases_inf, n, MsmOut{d_out_xy, d_out_inf}, (hipStream_t)stream);
}

// sum of n partial points laid out as n records of 80 bytes: x || y (64 B) + u32 infinity flag + pad -- the record a rank
// all-gathers (dv-pari_amd/distributed.py) and the one the in-library device threads hand back
extern "C" int dvp_points_sum_dev(const void* d_records, uint32_t n, void* d_out_xy, void* d_out_inf, void* stream) {
  if (!d_records || !n || !d_out_xy || !d_out_inf) return DVP_EINVAL;
  // the kernel walks the 80-byte records in place (point at +0, flag at +64): no staging buffer, nothing to wait for
  return msm_sum_points_dev(d_records, 80, (const char*)d_records + 64, n, 20, d_out_xy, d_out_inf, (hipStream_t)stream);
}

#include "msm_debug.cuh"  // dvp_debug_* and dvp_ubench_*: they read the host state above, hence here and not at the top

extern "C" int dvp_msm_affine(const uint64_t* scalars, const uint64_t* bases_xy, const uint8_t* bases_inf, size_t n,
                              uint64_t out_xy[8], int* out_is_infinity) {
  if ((n && (!scalars || !bases_xy)) || !out_xy || !out_is_infinity) return DVP_EINVAL;
  DevBuf ds, db, di;
  MsmResult sum;
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(db.up(bases_xy, n * 64));
  DVP_TRY(di.up_opt(bases_inf, n));
  DVP_TRY(sum.init());
  DVP_TRY(points_check_strict(db.p, di.p, n, 0));
  DVP_TRY(msm_affine_dev(ds.p, db.p, di.p, n, sum.out(), 0));
  return sum.down(out_xy, out_is_infinity);
}

// ---- public fixed-base MSM context: many MSMs over one base vector (an SRS) -----------------------------
struct dvp_msm_ctx {
  MsmFixedCtx* fx = nullptr;
  uint8_t* d_inf = nullptr;
  size_t n = 0;
};

extern "C" int dvp_msm_ctx_create(const uint64_t* bases_xy, const uint8_t* bases_inf, size_t n, size_t range_hint, dvp_msm_ctx** out) {
  if (!bases_xy || !out || !n || n >= ((size_t)1 << 27)) return DVP_EINVAL;
  if (!range_hint || range_hint > n) range_hint = n;
  DevBuf db;
  DVP_TRY(db.up(bases_xy, n * sizeof(Aff)));
  dvp_msm_ctx* c = new dvp_msm_ctx();
  c->n = n;
  auto fail = [&](int rc) { dvp_msm_ctx_destroy(c); return rc; };
  hipError_t e = hipMalloc((void**)&c->d_inf, n);
  if (e == hipSuccess) e = bases_inf ? hipMemcpy(c->d_inf, bases_inf, n, hipMemcpyHostToDevice) : hipMemset(c->d_inf, 0, n);
  if (e != hipSuccess) return fail(hip_fail(e, "dvp_msm_ctx_create", __FILE__, __LINE__));
  int rc = points_check_strict(db.p, c->d_inf, n, 0);
  if (rc != DVP_OK) return fail(rc);
  rc = msm_fixed_create(db.as<Aff>(), (uint32_t)n, range_hint, &c->fx);
  if (rc != DVP_OK) return fail(rc);
  *out = c;
  return DVP_OK;
}
extern "C" void dvp_msm_ctx_destroy(dvp_msm_ctx* c) {
  if (!c) return;
  msm_fixed_destroy(c->fx);
  if (c->d_inf) (void)hipFree(c->d_inf);
  delete c;
}
extern "C" int dvp_msm_ctx_plan(const dvp_msm_ctx* c, int* c_bits, int* windows) {
  if (!c || !c_bits || !windows) return DVP_EINVAL;
  return msm_fixed_info(c->fx, c_bits, windows);
}
extern "C" uint64_t dvp_msm_ctx_table_bytes(const dvp_msm_ctx* c, int* signed_windows) { return c ? msm_fixed_table_bytes(c->fx, signed_windows) : 0; }
// sum_{i in [lo,hi)} scalars[i - lo] * base[i]; d_scalars holds hi - lo canonical scalars (device)
extern "C" int dvp_msm_ctx_run_dev(dvp_msm_ctx* c, const void* d_scalars, size_t lo, size_t hi, void* d_out_xy, void* d_out_inf, void* stream) {
  if (!c || !d_scalars || !d_out_xy || !d_out_inf || lo > hi || hi > c->n) return DVP_EINVAL;
  return msm_fixed_dev(c->fx, d_scalars, c->d_inf + lo, (uint32_t)lo, (uint32_t)hi, MsmOut{d_out_xy, d_out_inf}, (hipStream_t)stream);
}
extern "C" int dvp_msm_ctx_run(dvp_msm_ctx* c, const uint64_t* scalars, size_t lo, size_t hi, uint64_t out_xy[8], int* out_is_infinity) {
  if (!c || !scalars || !out_xy || !out_is_infinity || lo > hi || hi > c->n) return DVP_EINVAL;
  DevBuf ds;
  MsmResult sum;
  DVP_TRY(ds.up(scalars, (hi - lo) * 32));
  DVP_TRY(sum.init());
  DVP_TRY(msm_fixed_dev(c->fx, ds.p, c->d_inf + lo, (uint32_t)lo, (uint32_t)hi, sum.out(), 0));
  return sum.down(out_xy, out_is_infinity);
}

// TEST ONLY (include/dvpari_internal.h; here and not in msm_debug.cuh because it reads dvp_msm_ctx): one MSM whose tail kernel also
// writes the 30-byte encoding, as a prover's commitment MSMs ask it to -- over the context's bases [lo, hi), or, without a context, a
// one-shot MSM over bases_xy[0 .. hi)
extern "C" int dvp_debug_msm_enc(dvp_msm_ctx* c, const uint64_t* scalars, const uint64_t* bases_xy, size_t lo, size_t hi, uint64_t out_xy[8],
                                 int* out_is_infinity, uint8_t out_enc[30]) {
  if (!scalars || !out_xy || !out_is_infinity || !out_enc || lo >= hi || (c ? hi > c->n : (lo != 0 || !bases_xy))) return DVP_EINVAL;
  DevBuf ds, db, denc;
  MsmResult sum;
  DVP_TRY(ds.up(scalars, (hi - lo) * 32));
  DVP_TRY(denc.alloc(32));
  DVP_TRY(sum.init());
  MsmOut out = sum.out();
  out.d_out_enc = denc.p;
  if (c)
    DVP_TRY(msm_fixed_dev(c->fx, ds.p, c->d_inf + lo, (uint32_t)lo, (uint32_t)hi, out, 0));
  else {
    DVP_TRY(db.up(bases_xy, hi * 64));
    DVP_TRY(msm_affine_dev(ds.p, db.p, nullptr, hi, out, 0));
  }
  DVP_TRY(denc.down(out_enc, 30));
  return sum.down(out_xy, out_is_infinity);
}
