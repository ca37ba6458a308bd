// The reference's on-disk formats and the cache-dir flavour of Proof::prove (host code, no kernels).
//
//   Fr vector file      u64-LE n || n x 29 B canonical LE      src/io_utils.rs:42-70,122-179
//   point vector file   u64-LE n || n x 30 B xsk233 encoding   src/io_utils.rs:83-111,187-239
//   witness file        u32-BE n || n x 32 B big-endian        src/gnark_r1cs.rs:58-77,188-198
//   R1CS dump           u32-LE nCoeffs || nCoeffs x 32 B BE || u32-LE nRows || rows of
//                       (nL, nR, nO: u32-LE) + (wire_id, coeff_id: u32-LE) terms
//                                                              src/gnark_r1cs.rs:84-91,121-185
//   file names          src/artifacts.rs:18-83
//
// dvp_prover_open_cache_dir is the loading half of Proof::prove (src/proving.rs:435-470,509-511,666-672): the R1CS
// dump and the five SRS vectors are parsed / decoded ONCE and stay in HBM; dvp_prove_cache_dir keeps the opened
// contexts in a process-wide table so that repeated prove(cache_dir, ..) calls only pay for the proof.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <tuple>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/dvpari.h"
#include "../../include/dvpari_internal.h"  // dvp_tune_get (DVP_CACHE_REPLICAS)
#include "fr.cuh"                           // fr_first_noncanonical: the range check of the 29-byte files
#include "fr_wire.cuh"                      // fr_from_be32_words: every 32-byte big-endian element
#include "host_api.h"
#include "mapped_file.h"

namespace {

// from_be_bytes_mod_order on 32 big-endian bytes at any address (gnark_element_to_fr): fr_wire.cuh's reduction, on the host
inline void be32_to_fr(const uint8_t* be, uint64_t out[4]) {
  uint32_t w[8], r[8];
  memcpy(w, be, 32);
  dvp::fr_from_be32_words(w, r);
  memcpy(out, r, 32);
}

using dvp::MappedFile;
using dvp::rd32le;
using dvp::rd64le;

// u64-LE count || count x elt bytes: returns the payload
int counted_payload(const MappedFile& f, size_t elt, const uint8_t** payload, size_t* n) {
  if (f.len < 8) return DVP_EIO;  // "File too short for length prefix"
  uint64_t cnt = rd64le(f.p);
  if (cnt > (f.len - 8) / elt) return DVP_EIO;  // "File too short for expected point data"
  *payload = f.p + 8;
  *n = (size_t)cnt;
  return DVP_OK;
}

int write_counted(const char* path, const uint8_t* payload, size_t n, size_t elt, const std::vector<uint8_t>* packed) {
  FILE* f = fopen(path, "wb");
  if (!f) return DVP_EIO;
  uint64_t cnt = n;
  bool ok = fwrite(&cnt, 8, 1, f) == 1;
  const uint8_t* src = packed ? packed->data() : payload;
  if (ok && n) ok = fwrite(src, elt, n, f) == n;
  ok = (fclose(f) == 0) && ok;
  return ok ? DVP_OK : DVP_EIO;
}

struct DumpView {
  uint32_t n_coeffs = 0, n_rows = 0, n_wires = 0;
  uint64_t nnz[3] = {0, 0, 0};
  const uint8_t* coeffs = nullptr;
  const uint8_t* rows = nullptr;  // first row header
};

// one validating pass over the dump: sizes, and max wire id + 1 (accumulate_m_values, src/srs.rs:56-62)
int dump_scan(const uint8_t* buf, size_t len, DumpView* v) {
  if (!buf || len < 8) return DVP_EIO;
  size_t off = 0;
  v->n_coeffs = rd32le(buf);
  off = 4;
  if ((len - off) / 32 < v->n_coeffs) return DVP_EIO;
  v->coeffs = buf + off;
  off += (size_t)32 * v->n_coeffs;
  if (len - off < 4) return DVP_EIO;
  v->n_rows = rd32le(buf + off);
  off += 4;
  v->rows = buf + off;
  uint32_t maxw = 0;
  bool any = false;
  for (uint32_t r = 0; r < v->n_rows; ++r) {
    if (len - off < 12) return DVP_EIO;
    uint32_t cnt[3] = {rd32le(buf + off), rd32le(buf + off + 4), rd32le(buf + off + 8)};
    off += 12;
    for (int k = 0; k < 3; ++k) {
      if ((len - off) / 8 < cnt[k]) return DVP_EIO;
      for (uint32_t t = 0; t < cnt[k]; ++t) {
        uint32_t w = rd32le(buf + off + 8 * (size_t)t), c = rd32le(buf + off + 8 * (size_t)t + 4);
        if (c >= v->n_coeffs) return DVP_EINVAL;  // the reference would index out of bounds and panic
        if (w > maxw) maxw = w;
        any = true;
      }
      v->nnz[k] += cnt[k];
      off += (size_t)8 * cnt[k];
    }
  }
  v->n_wires = any ? maxw + 1 : 1;
  return DVP_OK;
}

void dump_fill(const DumpView& v, uint64_t* coeffs, uint32_t* const row_ptr[3], uint32_t* const wire[3], uint32_t* const coeff[3]) {
  for (uint32_t i = 0; i < v.n_coeffs; ++i) be32_to_fr(v.coeffs + 32 * (size_t)i, coeffs + 4 * (size_t)i);
  const uint8_t* q = v.rows;
  uint32_t pos[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k) row_ptr[k][0] = 0;
  for (uint32_t r = 0; r < v.n_rows; ++r) {
    uint32_t cnt[3] = {rd32le(q), rd32le(q + 4), rd32le(q + 8)};
    q += 12;
    for (int k = 0; k < 3; ++k) {
      for (uint32_t t = 0; t < cnt[k]; ++t) {
        wire[k][pos[k]] = rd32le(q);
        coeff[k][pos[k]] = rd32le(q + 4);
        ++pos[k];
        q += 8;
      }
      row_ptr[k][r + 1] = pos[k];
    }
  }
}

std::string join(const char* dir, const char* name) {
  std::string s(dir);
  if (!s.empty() && s.back() != '/') s.push_back('/');
  return s + name;
}

// Provers opened by dvp_prove_cache_dir, keyed by (cache_dir, n_public, HIP device).  An entry is shared: a caller holds
// a reference for the whole of its prove, which runs under the entry's own mutex (a dvp_prover is one set of device
// buffers: two proofs on it must not overlap), and dvp_cache_dir_release only drops the table's reference, so the
// prover is destroyed when the last prove in flight returns.
struct OpenEntry {
  dvp_prover* p = nullptr;
  std::mutex mu;                    // guards the opening of `p`
  std::atomic<bool> opened{false};  // the files have been read (under mu); rc then holds the result
  int rc = DVP_OK;
  // A second prover over the same files, opened the first time a proof arrives while the first prover is busy: two host
  // threads calling dvp_prove_cache_dir on one cache_dir then have two proofs in flight on the GPU (+11 % constraints/s at
  // 2^20) instead of taking turns.  Costs one more decode of the SRS files and one more set of tables,
  // so it is opened only when (i) the first prover has finished a proof (its tables and MSM workspaces exist: what is in use
  // on the device is then a fair measure of one prover) and (ii) free HBM exceeds 1.25 x what is in use -- a replica must never
  // make the first prover's own allocations fail.  Callers take whichever of the two provers frees first (slot_cv).
  dvp_prover* p2 = nullptr;
  bool opened2 = false, opening2 = false;
  int rc2 = DVP_OK;
  std::mutex slot_mu;
  std::condition_variable slot_cv;
  bool busy[2] = {false, false};
  uint64_t proofs_done = 0;
  uint64_t room_retry_at = 1;  // a second prover is considered once proofs_done reaches this (first: after one completed proof)
  // dvp_cache_dir_set_binding (under slot_mu): a proof applies it to the prover it took when that prover's generation is behind, so a
  // prover opened later inherits it
  bool bind_has[2] = {false, false};
  uint8_t bind_hash[2][32];
  uint64_t bind_gen = 0, applied_gen[2] = {0, 0};
  // dvp_cache_dir_add_srs_dir (under the first prover's turn): the SRS directories loaded into further slots of `p`, by path.  The second
  // prover holds slot 0 only, so every multi-slot call takes the first.
  std::map<std::string, uint32_t> srs_dirs;
  ~OpenEntry() {
    if (p) dvp_prover_destroy(p);
    if (p2) dvp_prover_destroy(p2);
  }
};
typedef std::tuple<std::string, uint32_t, int> OpenKey;
std::mutex g_open_mu;
std::map<OpenKey, std::shared_ptr<OpenEntry>> g_open;

int current_device() {
  int d = -1;
  (void)hipGetDevice(&d);
  return d;
}
// The table lock only covers the lookup / insertion of a placeholder; reading the files, decoding the points and building
// the tables (seconds at full size) happen under the ENTRY's mutex, so opening one cache_dir neither blocks proofs on
// another one (or on another device) nor dvp_cache_dir_release.  A failed open leaves no entry behind.
int open_entry(const char* cache_dir, uint32_t n_public, std::shared_ptr<OpenEntry>* out) {
  OpenKey key(std::string(cache_dir), n_public, current_device());
  std::shared_ptr<OpenEntry> e;
  {
    std::lock_guard<std::mutex> g(g_open_mu);
    auto it = g_open.find(key);
    if (it == g_open.end()) it = g_open.emplace(key, std::make_shared<OpenEntry>()).first;
    e = it->second;
  }
  if (!e->opened.load(std::memory_order_acquire)) {  // (an opened entry is not locked here: its mutex is held for whole proofs)
    std::lock_guard<std::mutex> ge(e->mu);
    if (!e->opened.load(std::memory_order_relaxed)) {
      e->rc = dvp_prover_open_cache_dir(cache_dir, n_public, &e->p);
      e->opened.store(true, std::memory_order_release);
    }
  }
  if (e->rc != DVP_OK) {
    std::lock_guard<std::mutex> g(g_open_mu);
    auto it = g_open.find(key);
    if (it != g_open.end() && it->second == e) g_open.erase(it);
    return e->rc;
  }
  *out = e;
  return DVP_OK;
}

}  // namespace

extern "C" int dvp_file_fr_vec_write(const char* path, const uint64_t* limbs, size_t n) {
  if (!path || (!limbs && n)) return DVP_EINVAL;
  std::vector<uint8_t> packed(n * 29);
  for (size_t i = 0; i < n; ++i) {
    if (dvp::fr_first_noncanonical(limbs + 4 * i, 1) != 1) return DVP_EINVAL;
    memcpy(packed.data() + 29 * i, limbs + 4 * i, 29);  // little-endian host: the low 29 bytes of the 32
  }
  return write_counted(path, nullptr, n, 29, &packed);
}

extern "C" int dvp_file_fr_vec_read(const char* path, uint64_t* out, size_t cap, size_t* n) {
  if (!path || !n) return DVP_EINVAL;
  MappedFile f;
  int rc = f.open_ro(path);
  if (rc) return rc;
  const uint8_t* pl;
  rc = counted_payload(f, 29, &pl, n);
  if (rc) return rc;
  if (!out) return DVP_OK;
  if (cap < *n) return DVP_EINVAL;
  for (size_t i = 0; i < *n; ++i) {
    uint64_t v[4] = {0, 0, 0, 0};
    memcpy(v, pl + 29 * i, 29);
    // deserialize_uncompressed_unchecked (src/io_utils.rs:160) does not range-check; this boundary carries
    // canonical values only, so a value >= p is rejected instead of being passed on
    if (dvp::fr_first_noncanonical(v, 1) != 1) return DVP_EINVAL;
    memcpy(out + 4 * i, v, 32);
  }
  return DVP_OK;
}

extern "C" int dvp_file_point_vec_write(const char* path, const uint8_t* enc, size_t n) {
  if (!path || (!enc && n)) return DVP_EINVAL;
  return write_counted(path, enc, n, 30, nullptr);
}

extern "C" int dvp_file_point_vec_read(const char* path, uint8_t* out, size_t cap, size_t* n) {
  if (!path || !n) return DVP_EINVAL;
  MappedFile f;
  int rc = f.open_ro(path);
  if (rc) return rc;
  const uint8_t* pl;
  rc = counted_payload(f, 30, &pl, n);
  if (rc) return rc;
  if (!out) return DVP_OK;
  if (cap < *n) return DVP_EINVAL;
  memcpy(out, pl, 30 * *n);
  return DVP_OK;
}

extern "C" int dvp_file_witness_read(const char* path, uint64_t* out, size_t cap, size_t* n) {
  if (!path || !n) return DVP_EINVAL;
  MappedFile f;
  int rc = f.open_ro(path);
  if (rc) return rc;
  if (f.len < 4) return DVP_EIO;
  uint32_t cnt = ((uint32_t)f.p[0] << 24) | ((uint32_t)f.p[1] << 16) | ((uint32_t)f.p[2] << 8) | f.p[3];
  if ((f.len - 4) / 32 < cnt) return DVP_EIO;
  *n = cnt;
  if (!out) return DVP_OK;
  if (cap < cnt) return DVP_EINVAL;
  for (uint32_t i = 0; i < cnt; ++i) be32_to_fr(f.p + 4 + 32 * (size_t)i, out + 4 * (size_t)i);  // gnark_element_to_fr
  return DVP_OK;
}

extern "C" int dvp_file_witness_write(const char* path, const uint64_t* limbs, size_t n) {
  if (!path || (!limbs && n) || n > 0xffffffffull) return DVP_EINVAL;
  FILE* f = fopen(path, "wb");
  if (!f) return DVP_EIO;
  uint8_t hdr[4] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n};
  bool ok = fwrite(hdr, 4, 1, f) == 1;
  for (size_t i = 0; ok && i < n; ++i) {
    uint8_t be[32];
    for (int j = 0; j < 32; ++j) be[j] = (uint8_t)(limbs[4 * i + (31 - j) / 8] >> (8 * ((31 - j) % 8)));
    ok = fwrite(be, 32, 1, f) == 1;
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? DVP_OK : DVP_EIO;
}

extern "C" int dvp_r1cs_dump_sizes(const uint8_t* buf, size_t len, uint32_t* n_coeffs, uint32_t* n_rows, uint64_t nnz[3],
                                   uint32_t* n_wires) {
  if (!buf || !n_coeffs || !n_rows || !nnz || !n_wires) return DVP_EINVAL;
  DumpView v;
  int rc = dump_scan(buf, len, &v);
  if (rc) return rc;
  *n_coeffs = v.n_coeffs;
  *n_rows = v.n_rows;
  *n_wires = v.n_wires;
  for (int k = 0; k < 3; ++k) nnz[k] = v.nnz[k];
  return DVP_OK;
}

extern "C" int dvp_r1cs_dump_fill(const uint8_t* buf, size_t len, uint64_t* coeffs, uint32_t* const row_ptr[3], uint32_t* const wire[3],
                                  uint32_t* const coeff_id[3]) {
  if (!buf || !coeffs || !row_ptr || !wire || !coeff_id) return DVP_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!row_ptr[k] || !wire[k] || !coeff_id[k]) return DVP_EINVAL;
  DumpView v;
  int rc = dump_scan(buf, len, &v);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
    if (v.nnz[k] > 0xffffffffull) return DVP_EINVAL;
  dump_fill(v, coeffs, row_ptr, wire, coeff_id);
  return DVP_OK;
}

extern "C" int dvp_prover_open_cache_dir(const char* cache_dir, uint32_t n_public, dvp_prover** out) {
  if (!cache_dir || !out) return DVP_EINVAL;
  *out = nullptr;
  MappedFile dump;
  int rc = dump.open_ro(join(cache_dir, "r1cs_to_dvsnark").c_str());  // R1CS_CONSTRAINTS_FILE, src/artifacts.rs:76
  if (rc) return rc;
  DumpView v;
  rc = dump_scan(dump.p, dump.len, &v);
  if (rc) return rc;
  if (v.n_rows == 0) return DVP_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (v.nnz[k] > 0xffffffffull) return DVP_EINVAL;
  // the witness length is fixed by the commitment key: multi_scalar_mul asserts |assignment| == |g_m| (src/curve.rs:142)
  static const char* const names[5] = {"g_m", "g_q", "g_k_0", "g_k_1", "g_k_2"};  // src/artifacts.rs:18-27
  MappedFile srs[5];
  const uint8_t* payload[5];
  size_t cnt[5];
  for (int i = 0; i < 5; ++i) {
    rc = srs[i].open_ro(join(cache_dir, names[i]).c_str());
    if (rc) return rc;
    rc = counted_payload(srs[i], 30, &payload[i], &cnt[i]);
    if (rc) return rc;
  }
  uint32_t log_m = 0;
  while ((1ull << log_m) < v.n_rows) ++log_m;  // next_power_of_two, src/gnark_r1cs.rs:291
  if (log_m < 1) log_m = 1;
  const size_t m = (size_t)1 << log_m;
  if (cnt[0] < v.n_wires || cnt[0] < 1 + (size_t)n_public || cnt[0] > 0xffffffffull) return DVP_EINVAL;
  if (cnt[1] != m || cnt[2] != m || cnt[3] != m || cnt[4] != 2 * m) return DVP_EINVAL;
  std::vector<uint64_t> coeffs((size_t)4 * v.n_coeffs);
  std::vector<uint32_t> rp[3], wi[3], ci[3];
  uint32_t *rpp[3], *wip[3], *cip[3];
  for (int k = 0; k < 3; ++k) {
    rp[k].resize((size_t)v.n_rows + 1);
    wi[k].resize(v.nnz[k] ? v.nnz[k] : 1);
    ci[k].resize(v.nnz[k] ? v.nnz[k] : 1);
    rpp[k] = rp[k].data();
    wip[k] = wi[k].data();
    cip[k] = ci[k].data();
  }
  dump_fill(v, coeffs.data(), rpp, wip, cip);
  dvp_prover* p = nullptr;
  rc = dvp_prover_create(log_m, n_public, (uint32_t)cnt[0], &p);
  if (rc) return rc;
  rc = dvp_prover_set_coeffs(p, coeffs.data(), v.n_coeffs);
  for (int k = 0; k < 3 && !rc; ++k) rc = dvp_prover_set_matrix(p, k, v.n_rows, rpp[k], wip[k], cip[k]);
  for (int i = 0; i < 5 && !rc; ++i) rc = dvp_prover_set_srs_encoded(p, i, payload[i], cnt[i]);
  if (rc) {
    dvp_prover_destroy(p);
    return rc;
  }
  *out = p;
  return DVP_OK;
}

// one proof on the entry of (cache_dir, n_public): takes a prover of the entry (waiting its turn), brings its binding up to date, runs
// prove(prover), gives the prover back.  Shared by the limb flavour and the witness-file flavour of Proof::prove(cache_dir, ..).
// first_only: the proof needs the first prover (the one that holds the further SRS slots) and waits for that one.
template <class F>
static int prove_on_entry(const char* cache_dir, uint32_t n_public, F prove, bool first_only = false) {
  std::shared_ptr<OpenEntry> e;
  int rc = open_entry(cache_dir, n_public, &e);
  if (rc) return rc;
  long long replicas = 1;
  if (!first_only) (void)dvp_tune_get("DVP_CACHE_REPLICAS", &replicas);
  int slot = -1;
  {
    std::unique_lock<std::mutex> g(e->slot_mu);
    for (;;) {
      if (!e->busy[0]) { slot = 0; break; }
      if (replicas >= 2 && e->opened2 && e->rc2 == DVP_OK && !e->busy[1]) { slot = 1; break; }
      if (replicas >= 2 && !e->opened2 && !e->opening2 && e->proofs_done >= e->room_retry_at) {
        // the room check (device-wide, other tenants included) and the open itself run OUTSIDE slot_mu, which every release needs;
        // a failed check is not latched: it is asked again after another 16 completed proofs (memory may have come back)
        e->opening2 = true;
        g.unlock();
        size_t free_b = 0, total_b = 0;
        const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b > 1.25 * (double)(total_b - free_b);
        dvp_prover* q = nullptr;
        const int r2 = room ? dvp_prover_open_cache_dir(cache_dir, n_public, &q) : DVP_ENOMEM;
        g.lock();
        e->opening2 = false;
        if (room) {
          e->p2 = q;
          e->rc2 = r2;
          e->opened2 = true;
        } else {
          e->room_retry_at = e->proofs_done + 16;
        }
        e->slot_cv.notify_all();
        continue;
      }
      e->slot_cv.wait(g);
    }
    e->busy[slot] = true;
  }
  dvp_prover* pv = slot == 0 ? e->p : e->p2;
  rc = DVP_OK;
  {
    std::unique_lock<std::mutex> g(e->slot_mu);
    if (e->applied_gen[slot] != e->bind_gen) {
      const uint64_t gen = e->bind_gen;
      uint8_t h[2][32];
      const bool has[2] = {e->bind_has[0], e->bind_has[1]};
      memcpy(h, e->bind_hash, sizeof(h));
      g.unlock();
      rc = dvp_prover_set_transcript_binding(pv, has[0] ? h[0] : nullptr, has[1] ? h[1] : nullptr);
      g.lock();
      if (rc == DVP_OK) e->applied_gen[slot] = gen;
    }
  }
  if (rc == DVP_OK) rc = prove(pv);
  {
    std::lock_guard<std::mutex> g(e->slot_mu);
    e->busy[slot] = false;
    if (rc == DVP_OK) ++e->proofs_done;
  }
  e->slot_cv.notify_one();
  return rc;
}

extern "C" int dvp_prove_cache_dir(const char* cache_dir, const uint64_t* public_inputs, uint32_t n_public,
                                   const uint64_t* private_inputs, uint32_t n_private, uint8_t proof[118]) {
  if (!cache_dir || !proof) return DVP_EINVAL;
  return prove_on_entry(cache_dir, n_public,
                        [&](dvp_prover* pv) { return dvp_prove(pv, public_inputs, n_public, private_inputs, n_private, proof); });
}

// Proof::prove(cache_dir, Vec<Fr>, &[Fr]) with both vectors as the caller's memory holds them (dvp_prove_ark on the entry's prover)
extern "C" int dvp_prove_cache_dir_ark(const char* cache_dir, const uint64_t* public_ark, uint32_t n_public, const uint64_t* private_ark,
                                       uint32_t n_private, uint8_t proof[118]) {
  if (!cache_dir || !proof || (n_public && !public_ark) || (n_private && !private_ark)) return DVP_EINVAL;
  return prove_on_entry(cache_dir, n_public,
                        [&](dvp_prover* pv) { return dvp_prove_ark(pv, public_ark, n_public, private_ark, n_private, proof); });
}

// load_witness_from_file + Proof::prove in one call (src/gnark_r1cs.rs:188-211, src/dvsnark_test.rs:189-229): the file is mapped and its
// payload handed to dvp_prove_be32 as it is -- the elements are reduced mod p on the device.  Everything that can be said about the file
// without a device (header, count against the length, element 0 == 1) is said BEFORE the cache_dir entry is opened.
extern "C" int dvp_prove_cache_dir_witness_file(const char* cache_dir, uint32_t n_public, const char* witness_path, uint8_t proof[118],
                                                uint64_t* public_inputs_out) {
  if (!cache_dir || !proof) return DVP_EINVAL;
  const std::string path = witness_path ? std::string(witness_path) : join(cache_dir, "witness_to_dvsnark");  // src/artifacts.rs
  MappedFile f;
  int rc = f.open_ro(path.c_str());
  if (rc) return rc;
  if (f.len < 4) return DVP_EIO;
  const uint32_t cnt = ((uint32_t)f.p[0] << 24) | ((uint32_t)f.p[1] << 16) | ((uint32_t)f.p[2] << 8) | f.p[3];
  if ((f.len - 4) / 32 < cnt) return DVP_EIO;
  if (cnt < 1 + (uint64_t)n_public) return DVP_EINVAL;  // [1, public.., private..]
  const uint8_t* payload = f.p + 4;
  auto reduce = [&](size_t i, uint64_t out[4]) { be32_to_fr(payload + 32 * i, out); };
  if (!dvp::fr_be32_is_one(payload)) {  // the constant wire (src/proving.rs:449-452)
    dvp::g_last_error_index = 0;
    return DVP_EINVAL;
  }
  rc = prove_on_entry(cache_dir, n_public, [&](dvp_prover* pv) { return dvp_prove_be32(pv, payload, cnt, proof); });
  if (rc == DVP_OK && public_inputs_out)
    for (uint32_t i = 0; i < n_public; ++i) reduce(1 + (size_t)i, public_inputs_out + 4 * (size_t)i);
  return rc;
}

extern "C" int dvp_cache_dir_set_binding(const char* cache_dir, uint32_t n_public, const uint8_t* srs_hash, const uint8_t* circuit_hash,
                                         int bind_srs) {
  if (!cache_dir) return DVP_EINVAL;
  std::shared_ptr<OpenEntry> e;
  int rc = open_entry(cache_dir, n_public, &e);
  if (rc) return rc;
  uint8_t computed[32];
  if (bind_srs && !srs_hash) {  // the first prover's own SRS hash: take its turn like a proof
    {
      std::unique_lock<std::mutex> g(e->slot_mu);
      e->slot_cv.wait(g, [&] { return !e->busy[0]; });
      e->busy[0] = true;
    }
    rc = dvp_prover_srs_hash(e->p, computed);
    {
      std::lock_guard<std::mutex> g(e->slot_mu);
      e->busy[0] = false;
    }
    e->slot_cv.notify_all();
    if (rc) return rc;
    srs_hash = computed;
  }
  std::lock_guard<std::mutex> g(e->slot_mu);
  const uint8_t* h[2] = {srs_hash, circuit_hash};
  for (int k = 0; k < 2; ++k) {
    e->bind_has[k] = h[k] != nullptr;
    if (h[k]) memcpy(e->bind_hash[k], h[k], 32);
  }
  ++e->bind_gen;
  return DVP_OK;
}

// run(prover) for an entry that needs the circuit and no SRS (the circuit hash, the witness check).  The prover dvp_prove_cache_dir keeps
// for (cache_dir, n_public) on this device is used when it is open (taking its turn like a proof); otherwise a prover without SRS is
// built from the R1CS dump of cache_dir alone and destroyed: no SRS file is read.
template <class F>
static int on_circuit_prover(const char* cache_dir, uint32_t n_public, F run) {
  std::shared_ptr<OpenEntry> e;
  {
    std::lock_guard<std::mutex> g(g_open_mu);
    auto it = g_open.find(OpenKey(std::string(cache_dir), n_public, current_device()));
    if (it != g_open.end() && it->second->opened.load(std::memory_order_acquire) && it->second->rc == DVP_OK) e = it->second;
  }
  if (e) {
    {
      std::unique_lock<std::mutex> g(e->slot_mu);
      e->slot_cv.wait(g, [&] { return !e->busy[0]; });
      e->busy[0] = true;
    }
    const int rc = run(e->p);
    {
      std::lock_guard<std::mutex> g(e->slot_mu);
      e->busy[0] = false;
    }
    e->slot_cv.notify_all();
    return rc;
  }
  MappedFile dump;
  int rc = dump.open_ro(join(cache_dir, "r1cs_to_dvsnark").c_str());  // R1CS_CONSTRAINTS_FILE, src/artifacts.rs:76
  if (rc) return rc;
  DumpView v;
  rc = dump_scan(dump.p, dump.len, &v);  // what dvp_r1cs_dump_sizes reports: n_wires = highest wire id used + 1
  if (rc) return rc == DVP_EINVAL ? DVP_EIO : rc;  // a coefficient id outside the table: malformed
  if (v.n_rows == 0 || v.n_coeffs == 0) return DVP_EIO;
  for (int k = 0; k < 3; ++k)
    if (v.nnz[k] > 0xffffffffull) return DVP_EINVAL;
  uint32_t log_m = 0;
  while ((1ull << log_m) < v.n_rows) ++log_m;  // next_power_of_two, src/gnark_r1cs.rs:291
  if (log_m < 1) log_m = 1;
  std::vector<uint64_t> coeffs((size_t)4 * v.n_coeffs);
  std::vector<uint32_t> rp[3], wi[3], ci[3];
  uint32_t *rpp[3], *wip[3], *cip[3];
  for (int k = 0; k < 3; ++k) {
    rp[k].resize((size_t)v.n_rows + 1);
    wi[k].resize(v.nnz[k] ? v.nnz[k] : 1);
    ci[k].resize(v.nnz[k] ? v.nnz[k] : 1);
    rpp[k] = rp[k].data();
    wip[k] = wi[k].data();
    cip[k] = ci[k].data();
  }
  dump_fill(v, coeffs.data(), rpp, wip, cip);
  // the hash reads no wire: the prover only has to admit the ids the dump uses and [1, public..]
  const uint64_t n_wires = std::max<uint64_t>(v.n_wires, 1 + (uint64_t)n_public);
  if (n_wires > 0xffffffffull) return DVP_EINVAL;
  dvp_prover* p = nullptr;
  rc = dvp_prover_create(log_m, n_public, (uint32_t)n_wires, &p);
  if (rc) return rc;
  rc = dvp_prover_set_coeffs(p, coeffs.data(), v.n_coeffs);
  for (int k = 0; k < 3 && !rc; ++k) rc = dvp_prover_set_matrix(p, k, v.n_rows, rpp[k], wip[k], cip[k]);
  if (!rc) rc = run(p);
  dvp_prover_destroy(p);
  return rc;
}
// dvp_prover_circuit_hash from the R1CS dump of cache_dir alone (Transcript::circuit_info_hash, src/proving.rs:111-134, on the instance
// update_to_include_vandermode_matrix_d leaves, src/gnark_r1cs.rs:333-386) -- the verifier's way to the value: it ran the setup from
// the same dump.
extern "C" int dvp_circuit_hash_cache_dir(const char* cache_dir, uint32_t n_public, uint8_t out[32]) {
  if (!cache_dir || !out) return DVP_EINVAL;
  return on_circuit_prover(cache_dir, n_public, [&](dvp_prover* p) { return dvp_prover_circuit_hash(p, out); });
}

// dvp_prover_check_witness_be32 on a witness file, on the prover dvp_circuit_hash_cache_dir would use: no SRS file is read.  The header
// is checked as dvp_prove_cache_dir_witness_file checks it, before the prover is looked for; element 0 is left to the report.
extern "C" int dvp_check_witness_cache_dir_witness_file(const char* cache_dir, uint32_t n_public, const char* witness_path, dvp_unsat_row* rows,
                                                        size_t rows_cap, dvp_suspect_wire* wires, size_t wires_cap, dvp_witness_report* report) {
  if (!cache_dir || !report || (rows_cap && !rows) || (wires_cap && !wires)) return DVP_EINVAL;
  const std::string path = witness_path ? std::string(witness_path) : join(cache_dir, "witness_to_dvsnark");  // src/artifacts.rs
  MappedFile f;
  int rc = f.open_ro(path.c_str());
  if (rc) return rc;
  if (f.len < 4) return DVP_EIO;
  const uint32_t cnt = ((uint32_t)f.p[0] << 24) | ((uint32_t)f.p[1] << 16) | ((uint32_t)f.p[2] << 8) | f.p[3];
  if ((f.len - 4) / 32 < cnt) return DVP_EIO;
  if (cnt < 1 + (uint64_t)n_public) return DVP_EINVAL;  // [1, public.., private..]
  return on_circuit_prover(cache_dir, n_public, [&](dvp_prover* p) {
    return dvp_prover_check_witness_be32(p, f.p + 4, cnt, rows, rows_cap, wires, wires_cap, report);
  });
}

// ---- one prover, many verifiers (SRS per Trapdoor, src/srs.rs:31-50,177): further SRS directories in slots of the entry's first prover ----
// run(first prover) with the prover's turn taken, like a proof
template <class F>
static int on_first_prover(const std::shared_ptr<OpenEntry>& e, F run) {
  {
    std::unique_lock<std::mutex> g(e->slot_mu);
    e->slot_cv.wait(g, [&] { return !e->busy[0]; });
    e->busy[0] = true;
  }
  const int rc = run(e->p);
  {
    std::lock_guard<std::mutex> g(e->slot_mu);
    e->busy[0] = false;
  }
  e->slot_cv.notify_all();
  return rc;
}
extern "C" int dvp_cache_dir_add_srs_dir(const char* cache_dir, uint32_t n_public, const char* srs_dir, uint32_t* slot) {
  if (!cache_dir || !srs_dir || !slot) return DVP_EINVAL;
  std::shared_ptr<OpenEntry> e;
  int rc = open_entry(cache_dir, n_public, &e);
  if (rc) return rc;
  // srs_dir's own circuit, if it carries a dump: hashed before the turn is taken (srs_dir may be an open entry itself, cache_dir even)
  uint8_t h_other[32];
  bool has_dump = false;
  {
    MappedFile dump;
    has_dump = dump.open_ro(join(srs_dir, "r1cs_to_dvsnark").c_str()) == DVP_OK;
  }
  if (has_dump) {
    rc = dvp_circuit_hash_cache_dir(srs_dir, n_public, h_other);
    if (rc) return rc;
  }
  return on_first_prover(e, [&](dvp_prover* p) -> int {
    auto known = e->srs_dirs.find(srs_dir);
    if (known != e->srs_dirs.end()) {
      *slot = known->second;
      return DVP_OK;
    }
    if (has_dump) {
      uint8_t h_own[32];
      int r = dvp_prover_circuit_hash(p, h_own);
      if (r) return r;
      if (memcmp(h_own, h_other, 32)) return DVP_EINVAL;  // an SRS for another circuit
    }
    static const char* const names[5] = {"g_m", "g_q", "g_k_0", "g_k_1", "g_k_2"};  // src/artifacts.rs:18-27
    const size_t m = dvp_prover_msm_size(p, 1) / 4, n_wires = dvp_prover_msm_size(p, 0) - m;
    const size_t want[5] = {n_wires, m, m, m, 2 * m};
    MappedFile srs[5];
    const uint8_t* payload[5];
    size_t cnt[5];
    for (int i = 0; i < 5; ++i) {
      int r = srs[i].open_ro(join(srs_dir, names[i]).c_str());
      if (r) return r;
      r = counted_payload(srs[i], 30, &payload[i], &cnt[i]);
      if (r) return r;
    }
    for (int i = 0; i < 5; ++i)
      if (cnt[i] != want[i]) return DVP_EINVAL;
    uint32_t k = 0;
    int r = dvp_prover_srs_slot_add(p, &k);
    if (r) return r;
    const uint32_t back = dvp_prover_srs_slot_active(p);
    r = dvp_prover_srs_slot_select(p, k);
    for (int i = 0; i < 5 && !r; ++i) r = dvp_prover_set_srs_encoded(p, i, payload[i], cnt[i]);  // decoder and strict mode as for cache_dir's own
    (void)dvp_prover_srs_slot_select(p, back);
    if (r) {
      (void)dvp_prover_srs_slot_drop(p, k);
      return r;
    }
    e->srs_dirs[srs_dir] = k;
    *slot = k;
    return DVP_OK;
  });
}
// the binding of one slot of the entry's first prover.  Slot 0 is the entry's own SRS: dvp_cache_dir_set_binding, second prover included.
extern "C" int dvp_cache_dir_slot_set_binding(const char* cache_dir, uint32_t n_public, uint32_t slot, const uint8_t* srs_hash,
                                              const uint8_t* circuit_hash, int bind_srs) {
  if (!cache_dir) return DVP_EINVAL;
  if (slot == 0) return dvp_cache_dir_set_binding(cache_dir, n_public, srs_hash, circuit_hash, bind_srs);
  std::shared_ptr<OpenEntry> e;
  int rc = open_entry(cache_dir, n_public, &e);
  if (rc) return rc;
  return on_first_prover(e, [&](dvp_prover* p) -> int {
    const uint32_t back = dvp_prover_srs_slot_active(p);
    int r = dvp_prover_srs_slot_select(p, slot);
    if (r) return r;
    uint8_t computed[32];
    const uint8_t* sh = srs_hash;
    if (bind_srs && !sh) {
      r = dvp_prover_srs_hash(p, computed);
      sh = computed;
    }
    if (!r) r = dvp_prover_set_transcript_binding(p, sh, circuit_hash);
    (void)dvp_prover_srs_slot_select(p, back);
    return r;
  });
}
extern "C" int dvp_prove_cache_dir_multi(const char* cache_dir, uint32_t n_public, const uint32_t* slots, uint32_t n_slots,
                                         const uint64_t* public_inputs, const uint64_t* private_inputs, uint32_t n_private, uint8_t* proofs,
                                         int32_t* status) {
  if (!cache_dir || !slots || !n_slots || !proofs || !status) return DVP_EINVAL;
  return prove_on_entry(cache_dir, n_public, [&](dvp_prover* pv) {
    return dvp_prove_multi(pv, slots, n_slots, public_inputs, n_public, private_inputs, n_private, proofs, status);
  }, /*first_only=*/true);
}
extern "C" int dvp_prove_cache_dir_multi_ark(const char* cache_dir, uint32_t n_public, const uint32_t* slots, uint32_t n_slots,
                                             const uint64_t* public_ark, const uint64_t* private_ark, uint32_t n_private, uint8_t* proofs,
                                             int32_t* status) {
  if (!cache_dir || !slots || !n_slots || !proofs || !status) return DVP_EINVAL;
  return prove_on_entry(cache_dir, n_public, [&](dvp_prover* pv) {
    return dvp_prove_multi_ark(pv, slots, n_slots, public_ark, n_public, private_ark, n_private, proofs, status);
  }, /*first_only=*/true);
}
// the header checks of dvp_prove_cache_dir_witness_file, before cache_dir is opened
extern "C" int dvp_prove_cache_dir_multi_witness_file(const char* cache_dir, uint32_t n_public, const uint32_t* slots, uint32_t n_slots,
                                                      const char* witness_path, uint8_t* proofs, int32_t* status, uint64_t* public_inputs_out) {
  if (!cache_dir || !slots || !n_slots || !proofs || !status) return DVP_EINVAL;
  const std::string path = witness_path ? std::string(witness_path) : join(cache_dir, "witness_to_dvsnark");  // src/artifacts.rs
  MappedFile f;
  int rc = f.open_ro(path.c_str());
  if (rc) return rc;
  if (f.len < 4) return DVP_EIO;
  const uint32_t cnt = ((uint32_t)f.p[0] << 24) | ((uint32_t)f.p[1] << 16) | ((uint32_t)f.p[2] << 8) | f.p[3];
  if ((f.len - 4) / 32 < cnt) return DVP_EIO;
  if (cnt < 1 + (uint64_t)n_public) return DVP_EINVAL;  // [1, public.., private..]
  const uint8_t* payload = f.p + 4;
  if (!dvp::fr_be32_is_one(payload)) {  // the constant wire (src/proving.rs:449-452)
    dvp::g_last_error_index = 0;
    return DVP_EINVAL;
  }
  rc = prove_on_entry(cache_dir, n_public, [&](dvp_prover* pv) { return dvp_prove_multi_be32(pv, slots, n_slots, payload, cnt, proofs, status); },
                      /*first_only=*/true);
  if (rc == DVP_OK && public_inputs_out)
    for (uint32_t i = 0; i < n_public; ++i) be32_to_fr(payload + 32 * (1 + (size_t)i), public_inputs_out + 4 * (size_t)i);
  return rc;
}

// the prover dvp_prove_cache_dir uses for (cache_dir, n_public) on the current device, opened if need be: BORROWED --
// valid until dvp_cache_dir_release; for inspection (dvp_prover_debug_read, dvp_prover_msm_plan), not for concurrent proving
extern "C" int dvp_cache_dir_prover(const char* cache_dir, uint32_t n_public, dvp_prover** out) {
  if (!cache_dir || !out) return DVP_EINVAL;
  std::shared_ptr<OpenEntry> e;
  int rc = open_entry(cache_dir, n_public, &e);
  if (rc) return rc;
  *out = e->p;
  return DVP_OK;
}

extern "C" void dvp_cache_dir_release(const char* cache_dir) {
  std::lock_guard<std::mutex> g(g_open_mu);
  for (auto it = g_open.begin(); it != g_open.end();) {
    if (!cache_dir || std::get<0>(it->first) == cache_dir)
      it = g_open.erase(it);  // the prover goes when the last prove holding the entry returns
    else
      ++it;
  }
}
