// Shared host-side plumbing for libdvpari_hip.so: status codes, HIP error capture, scoped buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <typeinfo>
#include <vector>

#include "../../include/dvpari_internal.h"
#include "fr.cuh"
#include "host_api.h"

namespace dvp {

extern thread_local hipError_t g_last_hip_error;

inline int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  g_last_hip_error = e;
  fprintf(stderr, "[dvpari] HIP error %d (%s) at %s:%d: %s\n", (int)e, hipGetErrorString(e), file, line, what);
  // out of memory is the one HIP error a host can act on (a smaller table budget, fewer provers): it gets its own status.  A refused
  // allocation is an answer, not a fault: the runtime's sticky last-error is cleared, so that the hipGetLastError() check behind the
  // next kernel launch of this thread does not report it a second time (g_last_hip_error keeps it)
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return DVP_ENOMEM;
  }
  return DVP_EHIP;
}

#define DVP_HIP(call)                                                        \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess) return ::dvp::hip_fail(_e, #call, __FILE__, __LINE__); \
  } while (0)

#define DVP_TRY(call)        \
  do {                       \
    int _s = (call);         \
    if (_s != DVP_OK) return _s; \
  } while (0)

// RAII device buffer (host-side convenience for the host-pointer flavours of the ABI)
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int alloc(size_t n) {
    release();
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
    }
    bytes = n;
    return DVP_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
  // ---- staging of the host-pointer flavours: allocate and copy up (0 bytes allocates 16 and copies nothing), copy down ----
  int up(const void* host, size_t n) {
    DVP_TRY(alloc(n));
    if (n) DVP_HIP(hipMemcpy(p, host, n, hipMemcpyHostToDevice));
    return DVP_OK;
  }
  // an optional input, which is what every `inf` argument is: a null host pointer leaves p null
  int up_opt(const void* host, size_t n) { return host ? up(host, n) : DVP_OK; }
  int down(void* host, size_t n) const {
    DVP_HIP(hipMemcpy(host, p, n, hipMemcpyDeviceToHost));
    return DVP_OK;
  }
};

// the host range check of an entry's n scalars (32 little-endian bytes each, any alignment): DVP_EINVAL with g_last_error_index = the
// first one that is not below p
inline int scalars_in_range(const void* le32, size_t n) {
  const size_t bad = fr_first_noncanonical(le32, n);
  if (bad == n) return DVP_OK;
  g_last_error_index = (int64_t)bad;
  return DVP_EINVAL;
}

// a caller's trapdoor (tau, delta, epsilon): DVP_EINVAL for a null pointer or a value that is not below p.  Zero passes here: the
// verifier takes it as it takes any scalar, and the setup refuses it itself (setup.hip: setup_check_trapdoor)
inline int load_trapdoor(const uint64_t tau[4], const uint64_t delta[4], const uint64_t eps[4], Fr* t, Fr* d, Fr* e) {
  if (!tau || !delta || !eps) return DVP_EINVAL;
  return fr_load(tau, t) && fr_load(delta, d) && fr_load(eps, e) ? DVP_OK : DVP_EINVAL;
}

// the 80-byte result of an MSM: x || y (64 bytes), then the infinity flag as a u32 that holds 0 or 1
struct MsmResult : DevBuf {
  int init() { return alloc(80); }
  void* inf() const { return (char*)p + 64; }
  MsmOut out() const { return MsmOut{p, inf()}; }
  const uint8_t* inf8() const { return (const uint8_t*)inf(); }  // little-endian: the flag's first byte is the byte mask the codec kernels take
  int down(uint64_t out_xy[8], int* out_is_infinity) const {
    uint32_t r[20];
    DVP_TRY(DevBuf::down(r, sizeof r));
    memcpy(out_xy, r, 64);
    *out_is_infinity = (int)r[16];
    return DVP_OK;
  }
};

// a caller's 16-byte summary {u64 first bad index, u64 how many} as a checking kernel expects it: {~0, 0}
inline int summary_reset(void* d_summary, hipStream_t st) {
  DVP_HIP(hipMemsetAsync(d_summary, 0xff, 8, st));
  DVP_HIP(hipMemsetAsync((char*)d_summary + 8, 0, 8, st));
  return DVP_OK;
}
// The "first bad index" word of a call that owns it: armed to ~0 on the stream, lowered by the kernel's atomicMin, read by verdict().
// It is the first word of a summary, so a kernel that counts (k_points_check) gets the whole of one: reset it with summary_reset.
struct ErrWord : DevBuf {
  int arm(hipStream_t st) {
    DVP_TRY(alloc(16));
    DVP_HIP(hipMemsetAsync(p, 0xff, 8, st));
    return DVP_OK;
  }
  unsigned long long* word() const { return as<unsigned long long>(); }
  // waits for `st`: DVP_OK, or `code` with g_last_error_index = the index; count (optional) receives the summary's second word
  int verdict(hipStream_t st, int code, size_t* count = nullptr) const {
    unsigned long long s[2] = {~0ull, 0};
    DVP_HIP(hipMemcpyAsync(s, p, count ? 16 : 8, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipStreamSynchronize(st));
    if (count) *count = (size_t)s[1];
    if (s[0] == ~0ull) return DVP_OK;
    g_last_error_index = (int64_t)s[0];
    return code;
  }
};

// 256-byte carving of a workspace: take(bytes) gives the next region's offset, take<T>(bytes) its pointer over `base`; o is the total
struct Carver {
  uintptr_t base = 0;
  size_t o = 0;
  static size_t align(size_t v) { return (v + 255) & ~(size_t)255; }
  size_t take(size_t bytes) {
    const size_t at = o;
    o = align(o + bytes);
    return at;
  }
  template <class T>
  T* take(size_t bytes) {
    return (T*)(base + take(bytes));
  }
};

// one table per device, built at its first use on that device and kept for the life of the process (gen_table, gf_sqr_tables)
constexpr int DVP_MAX_DEVICES = 16;
template <class T>
struct PerDevice {
  std::mutex mu;
  T* tab[DVP_MAX_DEVICES] = {nullptr};
  // build(T** out): allocate and fill the current device's table, and wait for it
  template <class F>
  int get(T** out, F&& build) {
    int dev;
    DVP_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= DVP_MAX_DEVICES) return DVP_EINVAL;
    std::lock_guard<std::mutex> g(mu);
    if (!tab[dev]) {
      T* t = nullptr;
      DVP_TRY(build(&t));
      tab[dev] = t;
    }
    *out = tab[dev];
    return DVP_OK;
  }
};

// median of `reps` (odd, at most 99) timed runs of `launch` on the null stream after one warm-up run, by device events (dvp_ubench_*)
template <class F>
int median_ms(int reps, const char* what, F&& launch, double* out_ms) {
  hipEvent_t e0, e1;
  DVP_HIP(hipEventCreate(&e0));
  DVP_HIP(hipEventCreate(&e1));
  float t[99];
  hipError_t err = hipSuccess;
  int rc = DVP_OK;
  for (int r = -1; r < reps && err == hipSuccess && rc == DVP_OK; ++r) {
    (void)hipEventRecord(e0, 0);
    rc = launch();
    err = hipGetLastError();
    (void)hipEventRecord(e1, 0);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    if (r >= 0) t[r] = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != DVP_OK) return rc;
  if (err != hipSuccess) return hip_fail(err, what, __FILE__, __LINE__);
  std::sort(t, t + reps);
  *out_ms = t[reps / 2];
  return DVP_OK;
}

// Tuning knobs (tools/README.md).  Defaults are the measured optima; the environment (DVP_MSM_C, ...) is read ONCE, at
// the first use, and dvp_tune_set / dvp_tune_reset (include/dvpari.h) change a knob at run time -- that is how the tests
// force every window size / sort flavour / round shape, and how tools/ sweep.  Never read on a hot path.  Every field is a long long
// and has one row of kKnobs (capi.cpp), which gives it its name: a field without a row does not compile.
struct Tune {
  long long msm_c = 0;          // DVP_MSM_C: one-shot window bits (0 = cost model)
  long long msm_k = 0;          // DVP_MSM_K: fan-in of the projective reducer (0 = default)
  long long msm_fixed_c = 0;    // DVP_MSM_FIXED_C: fixed-base window bits (0 = cost model)
  long long fx_hi = -1;         // DVP_FX_HI: level-1 partition bits of the fixed-base sort (-1 = c/2)
  long long msm_proj = 0;       // DVP_MSM_MODE=proj: skip the batched-affine rounds
  long long msm_aff_min = 1ll << 19;   // DVP_MSM_AFF_MIN: pair rounds run while a round has this many additions
  long long msm_gate_min = 1;   // DVP_MSM_GATE_MIN: pair rounds with at least this many additions take turns between concurrent MSMs (HeavyGate); smaller ones overlap
  long long msm_ws_slots = 2;   // DVP_MSM_WS_SLOTS: MSMs that may run at the same time on one device (1 or 2 workspaces; their pair rounds still take turns, HeavyGate)
  long long cache_replicas = 1;  // DVP_CACHE_REPLICAS: provers dvp_prove_cache_dir may hold per cache_dir (1 = callers take turns on one prover, the default since the end of round 4: with the witness in host memory a second prover's latency chains land in the first one's pair rounds and two callers got 23.3-23.8 ms per proof where taking turns gives 21.2-21.4; 2 = a second one is opened when two callers overlap)
  long long msm_aff_tpb = 256;  // DVP_MSM_AFF_TPB: workgroup size of the pair rounds (64, 128 or 256)
  long long msm_aff_bmin = 8;   // DVP_MSM_AFF_BMIN: fewest slots a round thread owns (small rounds then use fewer threads, each sharing its inversion among more additions)
  long long msm_aff_share_inv = 2;  // DVP_MSM_AFF_SHARE_INV: the pair rounds' inversion once per WORKGROUP instead of once per wave (msm_rounds.cuh: AFF_SHARE_INV): 0 = never, 1 = whenever the workgroup has more than one wave, 2 = in rounds of at least DVP_MSM_AFF_SHARE_MIN planned additions
  long long msm_aff_share_min = 0;  // DVP_MSM_AFF_SHARE_MIN: with DVP_MSM_AFF_SHARE_INV=2 a round shares when it plans this many additions (0 = one chip-full at DVP_MSM_AFF_BMIN slots per thread); smaller rounds keep the private inversions, which have less latency
  long long msm_aff_bmax = 136; // DVP_MSM_AFF_BMAX: most slots (additions per shared inversion) a round thread owns (48 through round 4; msm_rounds.cuh: AFF_BMAX)
  long long ecfft_radix4 = 3;   // DVP_ECFFT_RADIX4: the unfused top of an extend: 3 = up to nine layers in ONE LDS-tiled launch (k_extend_top; what is above them as under 2), 2 = three layers per pass (k_butterfly8, then k_butterfly4 / k_butterfly for what is left), 1 = two, 0 = one
  long long ecfft_fold = 1;     // DVP_ECFFT_FOLD: enter / exit fold their pointwise stages into the first / last pass of their extends (0 = the separate launches of rounds 1-5: the parity tests run both)
  long long msm_accum_fast = 1;  // DVP_MSM_ACCUM_FAST: the fan-in-K reducer's first level without exceptional branches, exceptional tasks redone from a list (0 = the general kernel of rounds 1-5)
  long long msm_tail_groups = 1; // DVP_MSM_TAIL_GROUPS: a one-shot MSM's W x c tail points are first summed in groups of 16 on many workgroups (k_tail_groups; 0 = the single-workgroup tail alone)
  long long msm_accum_hex_max = -1;  // DVP_MSM_ACCUM_HEX_MAX: the fan-in reducer's LAST level uses a row of 16 lanes per task up to this many tasks (-1 = default, 0 = never)
  long long gf_inv_tabs = 1;     // DVP_GF_INV_TABS: squaring runs of the GF(2^233) inversion taken as table passes beyond the three long ones: 0 = none (rounds 1-5), 1 = the run of 14, 2 = the runs of 14 and 7
  long long msm_accum_quad_max = 0;    // DVP_MSM_ACCUM_QUAD_MAX: reducer launches with at most this many tasks (upper bound) use a quad of lanes per task (0 = default)
  long long msm_bucket_pairs_max = 12;  // DVP_MSM_BUCKET_PAIRS_MAX: what the pair rounds leave goes through k_bucket_pairs / k_bucket_rest (one thread per bucket) when no bucket holds more points than this; above it, and with 0, through the fan-in-K reducer
  long long msm_sort_fused = 1;  // DVP_MSM_SORT_FUSED: level 1 of the signed flavour's sort recomputes the entry words from the scalars (0 = k_recode_signed writes them to HBM first)
  long long msm_round_pipeline = 2;  // DVP_MSM_ROUND_PIPELINE: bookkeeping of the pair rounds (counts / offsets / descriptors): 2 = all rounds at once, four launches on the caller's stream before the first round (default); 1 = the same on a side stream behind the sort's last scatter (equal one proof at a time, 1 ms slower with two in flight); 0 = per round, between the rounds
  long long msm_round_dense = 0;     // DVP_MSM_ROUND_DENSE: 1 = with the all-rounds bookkeeping (DVP_MSM_ROUND_PIPELINE 1 / 2) a later pair round holds its additions in slots [0, A) and its odd leftovers behind them, two descriptor words per slot: the rows of leftovers copy and multiply nothing.  0 (default) = bucket order, one word per slot, as the per-round bookkeeping always does: alone the dense order measured 0.11-0.17 ms per 2^20 proof, within the parent's own spread (recorded negatives)
  long long msm_hex_max = -1;   // DVP_MSM_HEX_MAX: merge levels up to this many additions use a row of 16 lanes each (-1 = default, 0 = never)
  long long msm_quad_max = 0;   // DVP_MSM_QUAD_MAX: merge levels up to this many additions use a quad of lanes each (0 = default)
  long long msm_fixed_min = 1ll << 16; // DVP_MSM_FIXED_MIN: smallest shard the prover sends through the fixed-base tables
  long long fr_bi_shape = 6;           // DVP_FR_BI_SHAPE: workgroup x elements per thread of k_batch_inverse: 0 = 512 x 16 (rounds 3-4), 1 = 256 x 8, 2 = 256 x 4, 3 = 512 x 8, 4 = 128 x 8, 5 = 128 x 4, 6 = 256 x 16 (default: 2^21 elements 128 us against 139), 7 = 1024 x 8
  long long horner_max_pub = -1;       // DVP_HORNER_MAX_PUB: public-input count up to which i(X) on D' is evaluated by Horner (-1 = default)
  long long prove_host_transcript = 0; // DVP_PROVE_HOST_TRANSCRIPT: 1 = dvp_prove_dev waits for the commitment MSM and hashes the transcript on the host (rounds 1-4); 0 = on the device, one stream wait per proof
  long long table_budget_bytes = -1;   // DVP_TABLE_BUDGET_BYTES: HBM per device the fixed-base tables of a NEW prover may hold (-1 = no limit; dvp_prover_set_table_budget changes it per prover)
  long long msm_table_refuse = 0;      // DVP_MSM_TABLE_REFUSE: TEST ONLY, 1 = msm_fixed_build behaves as if its table allocation had returned hipErrorOutOfMemory, without asking the runtime
  long long points_mul_w = 3;          // DVP_POINTS_MUL_W: window width of dvp_points_mul's tau-NAF (3, 4 or 5; anything else = the default)
  long long msm_seg_piece = 4;         // DVP_MSM_SEG_PIECE: operands one lane of dvp_msm_segments' reduction sums per level, the piece length P (2 ..= 64; anything else = the default)
  long long circuit_hash_window = 0;   // DVP_CIRCUIT_HASH_WINDOW: 1 KiB chunks of the staging window dvp_prover_circuit_hash generates its stream into (0 or less = the default, 61440 chunks = 60 MiB, the SRS hash's window; at most 2^21); the digest does not depend on it
  long long msm_aligned_signed = 1;   // DVP_MSM_ALIGNED_SIGNED: the aligned-window tables hold 2^(c w) P and the windows are signed binary digits (0 = the tau-adic aligned windows over rows tau^(o_w) P)
  long long fr_digest_window = 0;     // DVP_FR_DIGEST_WINDOW: 1 KiB chunks of the staging window dvp_fr_vec_digest packs its stream into (0 or less = the default, 61440 chunks = 60 MiB; at most 2^21; never more than the stream has); the digest does not depend on it
};
Tune& tune();

// devices of the in-library multi-GPU mode (dvp_set_devices); empty = single device (whatever is current)
std::vector<int> mgpu_devices();
// provers that hold more than one SRS slot (prove_slots.cuh): while there is one, dvp_set_devices refuses a list of more than one device
void multi_slot_provers_add(int delta);

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// ---- per-kernel HIP-event timers (bench.py's roofline leg; off by default) ------------------------
// A timed launch records two events on the launch stream; prof_collect() (called where the host
// already synchronises) folds the elapsed times into named slots readable through dvp_profile_read.
enum ProfSlot { PROF_MSM_ACCUM_AFFINE = 0, PROF_MSM_TOTAL, PROF_EXTEND_TOTAL, PROF_PROVE_TOTAL, PROF_MSM_AFFINE_REST, PROF_MSM_SORT, PROF_MSM_TAIL, PROF_NSLOTS };
extern bool g_prof_enabled;
struct ProfScope {
  int slot;
  hipStream_t st;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint64_t key = 0;  // launch shape (first pair rounds: the MSM's pair count), see dvp_profile_round0_shapes
  ProfScope(int slot_, hipStream_t st_, uint64_t key_ = 0);
  void stop();
};
void prof_collect();
// host waits on the proof path, counted always (dvp_profile_read "host_waits_stream" / "host_waits_side"): kind 0 = a synchronisation
// of the caller's stream (the GPU idles until the host has reacted), kind 1 = the largest-bucket read of an MSM, taken on a side
// stream while the first pair round runs (the host waits, the GPU does not)
void count_host_wait(int kind);
// launches of the pair rounds after the first, counted always, by descriptor form (dvp_profile_read "later_rounds_word" /
// "later_rounds_dense"): the tests read which form ran
void count_later_round(bool dense);
// launches of ALL pair rounds, counted always, by the form of their inversion (dvp_profile_read "rounds_inv_shared" /
// "rounds_inv_private"): one per workgroup or one per wave
void count_round_inv(bool shared);

// ---- launch census: every kernel launch of the library is counted per variant, always -------------------------------------
// A variant is one kernel with its instantiated template arguments; its name is "<file>:<kernel><args>" as the compiler spells the
// instantiation, blanks removed ("msm.hip:k_merge<16,false>"), so a launch inside templated host code carries the arguments it was
// instantiated with.  The counter of a variant is a static member of a template over the kernel's address: sites that launch the same
// variant share it, and it registers its name when the library is loaded, so dvp_debug_launch_names (dvpari_internal.h) knows every
// variant host code can launch without launching anything.  dvp_profile_read("launch:<name>") reads a count, dvp_profile_reset
// zeroes them all.  The wrapper adds one relaxed host increment to a launch: no HIP call, no event, no synchronisation.
struct LaunchCounter {
  std::atomic<uint64_t> n{0};
};
LaunchCounter* census_register(const char* file, const char* tag_type);  // capi.cpp; tag_type = typeid(LaunchTag<&kernel<args>>).name()
template <auto K>
struct LaunchTag {};  // its mangled type name spells the kernel with every template argument; the registry demangles it
template <auto K>
struct LaunchSite {
  static LaunchCounter* const counter;
};
template <auto K>
LaunchCounter* const LaunchSite<K>::counter = census_register(__BASE_FILE__, typeid(LaunchTag<K>).name());
template <auto K>
struct Launch;
template <class... P, void (*K)(P...)>
struct Launch<K> {  // the kernel's own parameter types: arguments convert at the call, as they would in a direct launch
  static void go(dim3 grid, dim3 block, size_t lds, hipStream_t st, P... p) {
    LaunchSite<K>::counter->n.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(K, grid, block, (unsigned)lds, st, p...);
  }
};
#define DVP_LAUNCH(kernel, grid, block, lds, stream, ...) ::dvp::Launch<(kernel)>::go(grid, block, lds, stream, __VA_ARGS__)

}  // namespace dvp
