// Library-wide C ABI pieces: status strings, device selection, last-error bookkeeping.
#include "common.h"

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <cstring>
#include <cstdlib>
#include <climits>
#include <cxxabi.h>

namespace dvp {
thread_local int64_t g_last_error_index = -1;
thread_local hipError_t g_last_hip_error = hipSuccess;

bool g_prof_enabled = false;
static unsigned g_prof_mask = ~0u;  // which scopes record events (dvp_profile_enable: 1 = all, 2 = the dominant kernel's only)
static std::mutex g_prof_mu;
static double g_prof_ms[PROF_NSLOTS] = {0};
static uint64_t g_prof_n[PROF_NSLOTS] = {0};
struct Pending { int slot; hipEvent_t e0, e1; uint64_t key; };
struct Shape { double ms = 0; uint64_t n = 0; };
static std::map<uint64_t, Shape> g_prof_round0;  // first pair rounds by launch shape (key = (scalar, base) pairs of the MSM)
static std::vector<Pending> g_prof_pending;
static const char* kProfNames[PROF_NSLOTS] = {"msm_affine_round0", "msm_total", "extend_total", "prove_total", "msm_affine_rest", "msm_sort", "msm_tail"};

ProfScope::ProfScope(int slot_, hipStream_t st_, uint64_t key_) : slot(slot_), st(st_), key(key_) {
  if (!g_prof_enabled || slot_ < 0 || !((g_prof_mask >> slot_) & 1u)) return;  // slot -1: a scope that times nothing
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { e0 = e1 = nullptr; return; }
  (void)hipEventRecord(e0, st);
}
void ProfScope::stop() {
  if (!e0) return;
  (void)hipEventRecord(e1, st);
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_prof_pending.push_back({slot, e0, e1, key});
  e0 = e1 = nullptr;
}
void prof_collect() {
  std::lock_guard<std::mutex> g(g_prof_mu);
  for (auto& p : g_prof_pending) {
    float ms = 0;
    if (hipEventSynchronize(p.e1) == hipSuccess && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
      g_prof_ms[p.slot] += ms;
      g_prof_n[p.slot] += (p.slot == PROF_MSM_AFFINE_REST && p.key) ? p.key : 1;  // the later pair rounds of an MSM share one scope: key = their number
      if (p.slot == PROF_MSM_ACCUM_AFFINE && p.key) { Shape& sh = g_prof_round0[p.key]; sh.ms += ms; sh.n += 1; }
    }
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  g_prof_pending.clear();
}

static std::atomic<uint64_t> g_host_waits[2];
void count_host_wait(int kind) { g_host_waits[kind & 1].fetch_add(1, std::memory_order_relaxed); }
static std::atomic<uint64_t> g_later_rounds[2];
void count_later_round(bool dense) { g_later_rounds[dense ? 1 : 0].fetch_add(1, std::memory_order_relaxed); }
static std::atomic<uint64_t> g_rounds_inv[2];
void count_round_inv(bool shared) { g_rounds_inv[shared ? 1 : 0].fetch_add(1, std::memory_order_relaxed); }

// the launch census (common.h): name -> counter, filled while the library is loaded (the counters' own static initialisers call
// census_register, so the registry is built on first use) and only read afterwards
struct Census {
  std::mutex mu;
  std::map<std::string, LaunchCounter*> by_name;
};
static Census& census() {
  static Census* c = new Census;  // never destroyed: launches may still be counted while the process exits
  return *c;
}
LaunchCounter* census_register(const char* file, const char* tag_type) {
  // "dvp::LaunchTag<&(void dvp::k_merge<16, true>(Ld*, int, unsigned int, Ld*))>" or "dvp::LaunchTag<&dvp::k_post_sort>"
  // -> "k_merge<16,true>", "k_post_sort"; the file without its directories
  int st = 0;
  char* dm = abi::__cxa_demangle(tag_type ? tag_type : "", nullptr, nullptr, &st);
  std::string v = (st == 0 && dm) ? dm : (tag_type ? tag_type : "");
  free(dm);
  for (size_t at; (at = v.find("(anonymous namespace)::")) != std::string::npos;) v.erase(at, 23);
  size_t a = v.find("<&");
  if (a != std::string::npos) v = v.substr(a + 2);
  if (!v.empty() && v[0] == '(') v = v.substr(1);
  if (!v.compare(0, 5, "void ")) v = v.substr(5);
  std::string name;
  int depth = 0;
  for (size_t i = 0; i < v.size(); ++i) {  // the qualified name and its balanced template arguments, up to the parameter list
    const char ch = v[i];
    if (ch == '<') ++depth;
    if (depth == 0 && (ch == '(' || ch == ')' || ch == '>')) break;
    if (ch == '>') --depth;
    if (ch == ' ' && i > 0 && v[i - 1] == ',') continue;
    name.push_back(ch);
  }
  const size_t lt = name.find('<');
  const size_t ns = name.rfind("::", lt);  // kernels live in a namespace: the bare name
  if (ns != std::string::npos) name = name.substr(ns + 2);
  std::string f = file ? file : "";
  size_t sl = f.find_last_of("/\\");
  if (sl != std::string::npos) f = f.substr(sl + 1);
  name = f + ":" + name;
  Census& c = census();
  std::lock_guard<std::mutex> g(c.mu);
  LaunchCounter*& slot = c.by_name[name];
  if (!slot) slot = new LaunchCounter;
  return slot;
}

// Every knob once: its name and its field of Tune (common.h holds the fields, their defaults and what they do).  The environment, dvp_tune_set,
// dvp_tune_get and dvp_tune_reset all go through this table, in the order of the fields; a field without a row does not compile.
struct Knob {
  const char* name;
  long long Tune::*field;
};
static constexpr Knob kKnobs[] = {
    {"DVP_MSM_C", &Tune::msm_c},
    {"DVP_MSM_K", &Tune::msm_k},
    {"DVP_MSM_FIXED_C", &Tune::msm_fixed_c},
    {"DVP_FX_HI", &Tune::fx_hi},
    {"DVP_MSM_PROJ", &Tune::msm_proj},  // settable under this name; from the environment only as DVP_MSM_MODE=proj
    {"DVP_MSM_AFF_MIN", &Tune::msm_aff_min},
    {"DVP_MSM_GATE_MIN", &Tune::msm_gate_min},
    {"DVP_MSM_WS_SLOTS", &Tune::msm_ws_slots},
    {"DVP_CACHE_REPLICAS", &Tune::cache_replicas},
    {"DVP_MSM_AFF_TPB", &Tune::msm_aff_tpb},
    {"DVP_MSM_AFF_BMIN", &Tune::msm_aff_bmin},
    {"DVP_MSM_AFF_SHARE_INV", &Tune::msm_aff_share_inv},
    {"DVP_MSM_AFF_SHARE_MIN", &Tune::msm_aff_share_min},
    {"DVP_MSM_AFF_BMAX", &Tune::msm_aff_bmax},
    {"DVP_ECFFT_RADIX4", &Tune::ecfft_radix4},
    {"DVP_ECFFT_FOLD", &Tune::ecfft_fold},
    {"DVP_MSM_ACCUM_FAST", &Tune::msm_accum_fast},
    {"DVP_MSM_TAIL_GROUPS", &Tune::msm_tail_groups},
    {"DVP_MSM_ACCUM_HEX_MAX", &Tune::msm_accum_hex_max},
    {"DVP_GF_INV_TABS", &Tune::gf_inv_tabs},
    {"DVP_MSM_ACCUM_QUAD_MAX", &Tune::msm_accum_quad_max},
    {"DVP_MSM_BUCKET_PAIRS_MAX", &Tune::msm_bucket_pairs_max},
    {"DVP_MSM_SORT_FUSED", &Tune::msm_sort_fused},
    {"DVP_MSM_ROUND_PIPELINE", &Tune::msm_round_pipeline},
    {"DVP_MSM_ROUND_DENSE", &Tune::msm_round_dense},
    {"DVP_MSM_HEX_MAX", &Tune::msm_hex_max},
    {"DVP_MSM_QUAD_MAX", &Tune::msm_quad_max},
    {"DVP_MSM_FIXED_MIN", &Tune::msm_fixed_min},
    {"DVP_FR_BI_SHAPE", &Tune::fr_bi_shape},
    {"DVP_HORNER_MAX_PUB", &Tune::horner_max_pub},
    {"DVP_PROVE_HOST_TRANSCRIPT", &Tune::prove_host_transcript},
    {"DVP_TABLE_BUDGET_BYTES", &Tune::table_budget_bytes},
    {"DVP_MSM_TABLE_REFUSE", &Tune::msm_table_refuse},
    {"DVP_POINTS_MUL_W", &Tune::points_mul_w},
    {"DVP_MSM_SEG_PIECE", &Tune::msm_seg_piece},
    {"DVP_CIRCUIT_HASH_WINDOW", &Tune::circuit_hash_window},
    {"DVP_MSM_ALIGNED_SIGNED", &Tune::msm_aligned_signed},
    {"DVP_FR_DIGEST_WINDOW", &Tune::fr_digest_window},
};
static_assert(sizeof(Tune) == sizeof(kKnobs) / sizeof(kKnobs[0]) * sizeof(long long), "every field of Tune needs exactly one row of kKnobs");

static void tune_from_env(Tune& t) {
  t = Tune();
  for (const Knob& k : kKnobs) {
    if (k.field == &Tune::msm_proj) continue;  // a variable DVP_MSM_PROJ is ignored: the mode below sets the field
    const char* e = getenv(k.name);
    if (!e) continue;
    if (k.field == &Tune::table_budget_bytes) {  // the full u64 range: UINT64_MAX and anything above LLONG_MAX read as "no limit"
      const unsigned long long v = strtoull(e, nullptr, 10);
      t.*k.field = v > (unsigned long long)LLONG_MAX ? -1 : (long long)v;
    } else {
      t.*k.field = atoll(e);
    }
  }
  const char* m = getenv("DVP_MSM_MODE");
  t.msm_proj = (m && !strcmp(m, "proj")) ? 1 : 0;
}
static std::mutex g_dev_mu;
static std::vector<int> g_devices;
std::vector<int> mgpu_devices() {
  std::lock_guard<std::mutex> g(g_dev_mu);
  return g_devices;
}
static int g_multi_slot_provers = 0;  // under g_dev_mu, as the list it excludes
void multi_slot_provers_add(int delta) {
  std::lock_guard<std::mutex> g(g_dev_mu);
  g_multi_slot_provers += delta;
}
Tune& tune() {
  static Tune t = [] { Tune x; tune_from_env(x); return x; }();
  return t;
}
}  // namespace dvp

static long long* tune_slot(const char* name) {
  dvp::Tune& t = dvp::tune();
  for (const dvp::Knob& k : dvp::kKnobs)
    if (!strcmp(name, k.name)) return &(t.*k.field);
  return nullptr;
}
extern "C" int dvp_tune_set(const char* name, long long value) {
  long long* v = name ? tune_slot(name) : nullptr;
  if (!v) return DVP_EINVAL;
  *v = value;
  return DVP_OK;
}
extern "C" int dvp_tune_get(const char* name, long long* value) {
  long long* v = name ? tune_slot(name) : nullptr;
  if (!v || !value) return DVP_EINVAL;
  *value = *v;
  return DVP_OK;
}
extern "C" void dvp_tune_reset(void) { dvp::tune_from_env(dvp::tune()); }

// on = 1: every stage scope; on = 2: only the first pair rounds' (the dominant kernel: two events per MSM) -- an event pair is a packet of
// its own on the stream and puts ~10 us between two kernels that otherwise follow back to back, so the stage breakdown of a proof
// (seven scopes per MSM) is measured in a pass of its own, not in a timed loop
extern "C" void dvp_profile_enable(int on) {
  dvp::g_prof_mask = on == 2 ? (1u << dvp::PROF_MSM_ACCUM_AFFINE) : ~0u;
  dvp::g_prof_enabled = on != 0;
}
extern "C" void dvp_profile_reset(void) {
  dvp::prof_collect();
  std::lock_guard<std::mutex> g(dvp::g_prof_mu);
  for (int i = 0; i < dvp::PROF_NSLOTS; ++i) { dvp::g_prof_ms[i] = 0; dvp::g_prof_n[i] = 0; }
  dvp::g_prof_round0.clear();
  dvp::g_host_waits[0] = 0;
  dvp::g_host_waits[1] = 0;
  dvp::g_later_rounds[0] = 0;
  dvp::g_later_rounds[1] = 0;
  dvp::g_rounds_inv[0] = 0;
  dvp::g_rounds_inv[1] = 0;
  dvp::Census& c = dvp::census();
  std::lock_guard<std::mutex> gc(c.mu);
  for (auto& e : c.by_name) e.second->n.store(0, std::memory_order_relaxed);
}
// the census' names, one "file:variant" per line; returns the bytes needed (terminating NUL included), touches no device
extern "C" int dvp_debug_launch_names(char* buf, size_t cap) {
  dvp::Census& c = dvp::census();
  std::lock_guard<std::mutex> g(c.mu);
  std::string all;
  for (auto& e : c.by_name) { all += e.first; all += '\n'; }
  if (buf && cap) {
    const size_t k = all.size() < cap - 1 ? all.size() : cap - 1;
    memcpy(buf, all.data(), k);
    buf[k] = 0;
  }
  return (int)(all.size() + 1);
}
// the "msm_affine_round0" slot split by launch shape: one entry per distinct MSM size seen since the last reset
extern "C" int dvp_profile_round0_shapes(uint64_t* pairs, double* total_ms, uint64_t* launches, int cap) {
  if (cap < 0 || (cap > 0 && (!pairs || !total_ms || !launches))) return DVP_EINVAL;
  dvp::prof_collect();
  std::lock_guard<std::mutex> g(dvp::g_prof_mu);
  int k = 0;
  for (auto& e : dvp::g_prof_round0) {
    if (k < cap) { pairs[k] = e.first; total_ms[k] = e.second.ms; launches[k] = e.second.n; }
    ++k;
  }
  return k;
}
extern "C" int dvp_profile_read(const char* name, double* total_ms, uint64_t* launches) {
  if (!name || !total_ms || !launches) return DVP_EINVAL;
  if (!strcmp(name, "host_waits_stream") || !strcmp(name, "host_waits_side")) {  // counts since the last dvp_profile_reset
    *total_ms = 0;
    *launches = dvp::g_host_waits[name[11] == 's' && name[12] == 'i' ? 1 : 0].load();
    return DVP_OK;
  }
  if (!strcmp(name, "later_rounds_word") || !strcmp(name, "later_rounds_dense")) {  // launches since the last dvp_profile_reset
    *total_ms = 0;
    *launches = dvp::g_later_rounds[name[13] == 'd' ? 1 : 0].load();
    return DVP_OK;
  }
  if (!strcmp(name, "rounds_inv_private") || !strcmp(name, "rounds_inv_shared")) {  // launches since the last dvp_profile_reset
    *total_ms = 0;
    *launches = dvp::g_rounds_inv[name[11] == 's' ? 1 : 0].load();
    return DVP_OK;
  }
  if (!strncmp(name, "launch:", 7)) {  // the launch census: launches of one variant since the last dvp_profile_reset
    dvp::Census& c = dvp::census();
    std::lock_guard<std::mutex> g(c.mu);
    auto it = c.by_name.find(name + 7);
    if (it == c.by_name.end()) return DVP_EINVAL;
    *total_ms = 0;
    *launches = it->second->n.load(std::memory_order_relaxed);
    return DVP_OK;
  }
  dvp::prof_collect();
  std::lock_guard<std::mutex> g(dvp::g_prof_mu);
  for (int i = 0; i < dvp::PROF_NSLOTS; ++i)
    if (!strcmp(name, dvp::kProfNames[i])) { *total_ms = dvp::g_prof_ms[i]; *launches = dvp::g_prof_n[i]; return DVP_OK; }
  return DVP_EINVAL;
}

extern "C" const char* dvp_strerror(int s) {
  switch (s) {
    case DVP_OK: return "ok";
    case DVP_EINVAL: return "invalid argument (size, null pointer or non-canonical field element)";
    case DVP_EDECODE: return "invalid xsk233 point encoding";
    case DVP_EUNSAT: return "R1CS constraint not satisfied by the witness";
    case DVP_EHIP: return "HIP runtime error";
    case DVP_EIO: return "I/O error";
    case DVP_ENOMEM: return "out of memory";
    case DVP_ECHALLENGE: return "Fiat-Shamir challenge lies in the evaluation domain";
    case DVP_EPOINT: return "affine point unreduced, off the curve or outside the prime-order subgroup";
    default: return "unknown status";
  }
}

extern "C" int dvp_version(void) { return 100; }

extern "C" int dvp_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return DVP_EHIP;
  return n;
}

// In-library multi-GPU: the devices dvp_prove / dvp_prove_dev / dvp_prove_cache_dir spread the two MSMs of a proof over
// (one host thread per entry).  ids[0] should be the device the prover was created on (its "home"); an id may repeat
// (that is how the path is tested on a one-GPU box).  n <= 1 (or ids == NULL) switches back to single-device proving.
// A list of more than one device while a prover holds a second SRS slot is DVP_EINVAL (the shards hold per-device slices of ONE SRS).
extern "C" int dvp_set_devices(const int* ids, int n) {
  int cnt = 0;
  DVP_HIP(hipGetDeviceCount(&cnt));
  if (n < 0 || n > 64 || (n > 0 && !ids)) return DVP_EINVAL;
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= cnt) return DVP_EINVAL;
  std::lock_guard<std::mutex> g(dvp::g_dev_mu);
  if (n > 1 && dvp::g_multi_slot_provers > 0) return DVP_EINVAL;
  dvp::g_devices.assign(ids, ids + (n > 1 ? n : 0));
  return DVP_OK;
}

extern "C" int dvp_set_device(int id) {
  DVP_HIP(hipSetDevice(id));
  return DVP_OK;
}

extern "C" int64_t dvp_last_error_index(void) { return dvp::g_last_error_index; }
