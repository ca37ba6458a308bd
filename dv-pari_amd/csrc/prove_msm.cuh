// The prover's two MSMs: prover_msm_partial under the table budget, the in-library multi-GPU shards, prove_msm, and the plan / table /
// budget / coverage entries.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
#pragma once
#include "prove_state.cuh"

// which = 0: <[w | q2], [g_m | g_q]> (n_wires + m terms; commit_p = msm_q + msm_gm, src/proving.rs:463,512,515)
// which = 1: <[k_a | k_b | k_r], [g_k_0 | g_k_1 | g_k_2]> (4m terms, src/proving.rs:666-680)
// restricted to the index range [lo, hi): the per-GPU shard of the sum.
// d_out_enc (optional): the MSM's tail kernel also writes the 30-byte encoding of its result there
// d_err_defer (optional): deferred completion -- the call returns with the MSM enqueued (msm.hip: msm_core), its scalar-range word
// goes to that device word and nothing is copied to the host
static int prover_msm_partial(dvp_prover* p, int which, size_t lo, size_t hi, void* d_out_xy, void* d_out_inf, void* d_out_enc, void* stream,
                              unsigned long long* d_err_defer = nullptr) {
  if (!p || (which != 0 && which != 1) || !d_out_xy || !d_out_inf) return DVP_EINVAL;
  size_t total = which ? 4 * (size_t)p->m : (size_t)p->n_wires + p->m;
  if (lo > hi || hi > total) return DVP_EINVAL;
  const Fr* sc = which ? p->SK : p->SA;
  const Aff* bs = which ? p->bases_k : p->bases_a;
  const uint8_t* inf = which ? p->inf_k : p->inf_a;
  if (!bs) return DVP_EINVAL;  // an added SRS slot that no setter has touched yet holds no bases
  // after an extend-free begin (dvp_prove_begin_partial(need_extend = 0)) q2 and the r2 inside k_r were never computed:
  // a range that reads them would silently sum garbage
  if (!p->last_begin_extended && hi > lo && hi > (which ? 2 * (size_t)p->m : (size_t)p->n_wires)) return DVP_EINVAL;
  // fixed-base mode pays off once the shared 2^c-bucket set is well filled.  The pre-rotated table covers only the index
  // range this prover is asked for (a rank of a multi-process prove always asks for the same slice: W x slice x 64 B of
  // HBM instead of W x everything); a call outside the covered range rebuilds it for the new range.
  // A table the runtime refuses (DVP_ENOMEM) does not fail the call: the MSM goes through the one-shot path, and the allocation
  // is not tried again before the next dvp_prover_set_table_budget.
  const size_t fixed_min = (size_t)(tune().msm_fixed_min > 0 ? tune().msm_fixed_min : 1);
  hipStream_t st = (hipStream_t)stream;
  void* h_copy = d_out_enc && !d_err_defer ? p->fin_host : nullptr;
  const MsmOut out{d_out_xy, d_out_inf, d_out_enc, h_copy, p->blk, FIN_BYTES, d_err_defer};
  if (p->table_budget == UINT64_MAX) {
    if (hi - lo >= fixed_min && total < ((size_t)1 << 27) && !p->table_refused[which]) {
      if (p->fx[which] && (lo < p->fx_lo[which] || hi > p->fx_hi[which])) {
        msm_fixed_destroy(p->fx[which]);
        p->fx[which] = nullptr;
      }
      int rc = DVP_OK;
      if (!p->fx[which]) {
        rc = msm_fixed_create(bs + lo, (uint32_t)(hi - lo), hi - lo, &p->fx[which]);
        if (rc != DVP_OK && rc != DVP_ENOMEM) return rc;
        p->fx_lo[which] = lo;
        p->fx_hi[which] = hi;
      }
      if (rc == DVP_OK) {
        const size_t o = p->fx_lo[which];
        return msm_fixed_dev(p->fx[which], sc + lo, inf + lo, (uint32_t)(lo - o), (uint32_t)(hi - o), out, st);
      }
      p->table_refused[which] = true;
    }
    return msm_affine_dev(sc + lo, bs + lo, inf + lo, hi - lo, out, st);
  }
  // Under a budget the table is the planned prefix [0, cov) of the WHOLE vector, whatever range is asked for: [lo, min(hi, cov))
  // comes out of it, the rest of [lo, hi) out of the one-shot MSM, and k_join_points adds the two (a mixed MSM).
  size_t cov = 0;
  if (!p->table_refused[which]) {
    size_t pc[2];
    uint64_t pb[2];
    DVP_TRY(dvp_table_plan(dvp_prover_msm_size(p, 0), dvp_prover_msm_size(p, 1), p->table_budget, pc, pb));
    cov = pc[which];
  }
  if (p->fx[which] && (p->fx_lo[which] != 0 || p->fx_hi[which] != cov)) {
    msm_fixed_destroy(p->fx[which]);
    p->fx[which] = nullptr;
  }
  const size_t a = hi < cov ? hi : cov;  // end of the part the table serves
  if (cov > 0 && a > lo && a - lo >= fixed_min) {
    int rc = DVP_OK;
    if (!p->fx[which]) {
      rc = msm_fixed_create(bs, (uint32_t)cov, cov, &p->fx[which]);
      if (rc != DVP_OK && rc != DVP_ENOMEM) return rc;
      p->fx_lo[which] = 0;
      p->fx_hi[which] = cov;
    }
    if (rc == DVP_ENOMEM) {
      p->table_refused[which] = true;
    } else if (a == hi) {
      return msm_fixed_dev(p->fx[which], sc + lo, inf + lo, (uint32_t)lo, (uint32_t)hi, out, st);
    } else {
      // both halves with deferred completion on the caller's stream (the second one queues behind the first in the same workspace),
      // then the join: it writes what a single MSM's tail kernel would have -- point, encoding, range word -- so the call ends as
      // the single path does: deferred, or with the block copied to pinned memory ahead of ONE synchronisation
      char* mx = p->mix;
      unsigned long long* e2 = (unsigned long long*)(mx + MIX_OFF_ERR);
      unsigned long long* e_out = d_err_defer ? d_err_defer : (unsigned long long*)(mx + MIX_OFF_ERR_OUT);
      DVP_TRY(msm_fixed_dev(p->fx[which], sc + lo, inf + lo, (uint32_t)lo, (uint32_t)a, MsmOut{mx, mx + MIX_OFF_INF, nullptr, nullptr, nullptr, 0, e2}, st));
      rc = msm_affine_dev(sc + a, bs + a, inf + a, hi - a, MsmOut{mx + 64, mx + MIX_OFF_INF + 4, nullptr, nullptr, nullptr, 0, e2 + 1}, st);
      if (rc == DVP_OK)
        rc = msm_join_points_dev(mx, mx + MIX_OFF_INF, e2, mx + 64, mx + MIX_OFF_INF + 4, e2 + 1, (uint32_t)(a - lo), d_out_xy, d_out_inf, d_out_enc, e_out, st);
      if (rc != DVP_OK) {
        (void)hipStreamSynchronize(st);  // the first half is in flight in its workspace
        return rc;
      }
      if (d_err_defer) return DVP_OK;
      volatile unsigned long long* h_err = (volatile unsigned long long*)(p->fin_host + 1);  // behind the mirror
      if (h_copy) DVP_HIP(hipMemcpyAsync(h_copy, p->blk, FIN_BYTES, hipMemcpyDeviceToHost, st));
      DVP_HIP(hipMemcpyAsync((void*)h_err, e_out, 8, hipMemcpyDeviceToHost, st));
      DVP_HIP(hipStreamSynchronize(st));
      count_host_wait(0);
      const unsigned long long e = *h_err;
      if (e != ~0ull) {
        g_last_error_index = (int64_t)(e & 0xffffffffull);
        return DVP_EINVAL;
      }
      return DVP_OK;
    }
  }
  return msm_affine_dev(sc + lo, bs + lo, inf + lo, hi - lo, out, st);
}
extern "C" int dvp_prover_msm_partial(dvp_prover* p, int which, size_t lo, size_t hi, void* d_out_xy, void* d_out_inf, void* stream) {
  if (p && (which == 0 || which == 1) && d_out_xy == (void*)(p->pts + which)) {
    p->enc_fused[which] = false;  // the point changes, its encoding does not follow
    p->trace_ok = false;          // nor does a trace describe the proof whose point this was
  }
  return prover_msm_partial(p, which, lo, hi, d_out_xy, d_out_inf, nullptr, stream);
}

// ---- in-library multi-GPU (dvp_set_devices) ------------------------------------------------------------------------
// Only the MSMs shard: they are sums over disjoint index ranges and > 85 % of a proof.  Shard k lives on
// device shard_devices[k]: its slice [lo, hi) of both base vectors (copied once, device to device), the fixed-base
// tables of that slice, a scalar buffer and a stream.  A proof sends each shard its slice of the scalars
// (hipMemcpyPeerAsync), runs the partial MSMs concurrently -- one host thread per device -- and adds the partial points
// on the home device (k_sum_points).  RCCL is not involved: the exchange is N x 8..32 MB of scalars one way and N x 80
// bytes back, both point-to-point copies over xGMI.
static void shards_release(dvp_prover* p) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (auto& sh : p->shards) {
    (void)hipSetDevice(sh.device);
    for (int w = 0; w < 2; ++w) {
      if (sh.bases[w]) (void)hipFree(sh.bases[w]);
      if (sh.inf[w]) (void)hipFree(sh.inf[w]);
      if (sh.sc[w]) (void)hipFree(sh.sc[w]);
      msm_fixed_destroy(sh.fx[w]);
    }
    if (sh.out) (void)hipFree(sh.out);
    if (sh.st) (void)hipStreamDestroy(sh.st);
  }
  p->shards.clear();
  p->shard_devices.clear();
  (void)hipSetDevice(cur);
}
static void even_range(size_t total, size_t k, size_t n, size_t* lo, size_t* hi) {
  size_t base = total / n, rem = total % n;
  *lo = k * base + (k < rem ? k : rem);
  *hi = *lo + base + (k < rem ? 1 : 0);
}
static int shards_build(dvp_prover* p, const std::vector<int>& devs) {
  shards_release(p);
  const size_t n = devs.size();
  if (n > 64 || devs[0] != p->home_device) return DVP_EINVAL;  // ids[0] must be the device the prover's buffers live on
  // the single-device tables (up to 97 GB of rotations at 2^20 constraints) would sit beside the shard tables: shard 0's
  // msm_fixed_create would see less free HBM and fall back to the aligned windows
  for (int w = 0; w < 2; ++w) {
    msm_fixed_destroy(p->fx[w]);
    p->fx[w] = nullptr;
  }
  if (!p->mg_parts) DVP_HIP(hipMalloc((void**)&p->mg_parts, 64 * 68));
  p->shards.resize(n);
  int rc = DVP_OK;
  for (size_t k = 0; k < n && rc == DVP_OK; ++k) {
    dvp_prover::Shard& sh = p->shards[k];
    sh.device = devs[k];
    auto body = [&]() -> int {
      DVP_HIP(hipSetDevice(sh.device));
      if (sh.device != p->home_device) {
        // already-enabled / unsupported are fine (peer copies are staged then); clear the sticky error so that the next
        // hipGetLastError() check after a kernel launch does not report it
        if (hipDeviceEnablePeerAccess(p->home_device, 0) != hipSuccess) (void)hipGetLastError();
      }
      DVP_HIP(hipStreamCreateWithFlags(&sh.st, hipStreamNonBlocking));
      DVP_HIP(hipMalloc((void**)&sh.out, 2 * 80));
      for (int w = 0; w < 2; ++w) {
        const size_t total = w ? 4 * (size_t)p->m : (size_t)p->n_wires + p->m;
        even_range(total, k, n, &sh.lo[w], &sh.hi[w]);
        const size_t cnt = sh.hi[w] - sh.lo[w];
        const Aff* src_b = (w ? p->bases_k : p->bases_a) + sh.lo[w];
        const uint8_t* src_i = (w ? p->inf_k : p->inf_a) + sh.lo[w];
        DVP_HIP(hipMalloc((void**)&sh.bases[w], (cnt ? cnt : 1) * sizeof(Aff)));
        DVP_HIP(hipMalloc((void**)&sh.inf[w], cnt ? cnt : 1));
        DVP_HIP(hipMalloc((void**)&sh.sc[w], (cnt ? cnt : 1) * sizeof(Fr)));
        if (cnt) {
          DVP_HIP(hipMemcpyPeer(sh.bases[w], sh.device, src_b, p->home_device, cnt * sizeof(Aff)));
          DVP_HIP(hipMemcpyPeer(sh.inf[w], sh.device, src_i, p->home_device, cnt));
        }
      }
      // tables: the device's budget split evenly among the shards that name it, the K MSM first, all or nothing per MSM; a shard
      // whose table does not fit, or is refused by the runtime, runs one-shot (mgpu_msm: sh.fx[w] == nullptr)
      const size_t fixed_min = (size_t)(tune().msm_fixed_min > 0 ? tune().msm_fixed_min : 1);
      size_t sharing = 0;
      for (int d : devs) sharing += d == sh.device ? 1 : 0;
      uint64_t left = p->table_budget == UINT64_MAX ? UINT64_MAX : p->table_budget / sharing;
      for (int w = 1; w >= 0; --w) {
        const size_t cnt = sh.hi[w] - sh.lo[w];
        if (cnt < fixed_min || p->table_refused[w]) continue;
        const uint64_t need = (uint64_t)msm_fixed_rows_for(cnt) * cnt * sizeof(Aff);
        if (need > left) continue;
        const int rc_t = msm_fixed_create(sh.bases[w], (uint32_t)cnt, cnt, &sh.fx[w]);
        if (rc_t == DVP_ENOMEM) { p->table_refused[w] = true; continue; }
        DVP_TRY(rc_t);
        if (left != UINT64_MAX) left -= need;
      }
      return DVP_OK;
    };
    rc = body();
  }
  (void)hipSetDevice(p->home_device);
  if (rc != DVP_OK) {
    shards_release(p);
    return rc;
  }
  p->shard_devices = devs;
  return DVP_OK;
}

// MSM `which` over all shards -> home buffers d_out_xy / d_out_inf.  The home stream must have produced the scalars.
static int mgpu_msm(dvp_prover* p, int which, void* d_out_xy, void* d_out_inf, hipStream_t home_st) {
  const Fr* sc = which ? p->SK : p->SA;
  DVP_HIP(hipStreamSynchronize(home_st));
  const size_t n = p->shards.size();
  std::vector<int> rcs(n, DVP_OK);
  std::vector<int64_t> err_idx(n, -1);
  std::vector<std::thread> th;
  struct Rec { uint32_t xy[16]; uint32_t inf; };
  std::vector<Rec> recs(n);
  for (size_t k = 0; k < n; ++k) {
    th.emplace_back([&, k]() {
      dvp_prover::Shard& sh = p->shards[k];
      auto body = [&]() -> int {
        DVP_HIP(hipSetDevice(sh.device));
        const size_t cnt = sh.hi[which] - sh.lo[which];
        uint32_t* out = sh.out + 20 * which;
        if (cnt) DVP_HIP(hipMemcpyPeerAsync(sh.sc[which], sh.device, sc + sh.lo[which], p->home_device, cnt * sizeof(Fr), sh.st));
        if (sh.fx[which])
          DVP_TRY(msm_fixed_dev(sh.fx[which], sh.sc[which], sh.inf[which], 0, (uint32_t)cnt, MsmOut{out, out + 16}, sh.st));
        else
          DVP_TRY(msm_affine_dev(sh.sc[which], sh.bases[which], sh.inf[which], cnt, MsmOut{out, out + 16}, sh.st));
        DVP_HIP(hipMemcpyAsync(&recs[k], out, 68, hipMemcpyDeviceToHost, sh.st));
        DVP_HIP(hipStreamSynchronize(sh.st));
        return DVP_OK;
      };
      rcs[k] = body();
      err_idx[k] = g_last_error_index;  // thread-local in the worker: carry it back
    });
  }
  for (auto& t : th) t.join();
  DVP_HIP(hipSetDevice(p->home_device));
  for (size_t k = 0; k < n; ++k)
    if (rcs[k] != DVP_OK) {
      if (err_idx[k] >= 0) g_last_error_index = err_idx[k] + (int64_t)p->shards[k].lo[which];  // index in the whole vector
      return rcs[k];
    }
  // partial points -> home: packed as n points then n flags
  std::vector<uint32_t> pk(n * 17);
  for (size_t k = 0; k < n; ++k) {
    memcpy(&pk[16 * k], recs[k].xy, 64);
    pk[16 * n + k] = recs[k].inf;
  }
  DVP_HIP(hipMemcpyAsync(p->mg_parts, pk.data(), n * 68, hipMemcpyHostToDevice, home_st));
  DVP_TRY(msm_sum_points_dev(p->mg_parts, 64, p->mg_parts + 16 * n, (uint32_t)n, 1, d_out_xy, d_out_inf, home_st));
  DVP_HIP(hipStreamSynchronize(home_st));  // pk goes out of scope
  return DVP_OK;
}
// the MSM of a full proof: over the shards when a device list is set, else on the home device alone
static int prove_msm(dvp_prover* p, int which, void* d_out_xy, void* d_out_inf, void* stream) {
  const std::vector<int> devs = mgpu_devices();
  if (devs.size() > 1) {
    if (devs != p->shard_devices) DVP_TRY(shards_build(p, devs));
    p->enc_fused[which] = false;
    return mgpu_msm(p, which, d_out_xy, d_out_inf, (hipStream_t)stream);
  }
  if (!p->shards.empty()) shards_release(p);
  // the whole sum on this device, into the prover's own slot: let the tail kernel encode it too (dvp_prove_challenge / _finish then
  // skip their k_encode_point: one launch, one host round trip and one inversion chain less per commitment)
  const bool own = d_out_xy == (void*)(p->pts + which) && d_out_inf == (void*)(p->pts_inf32 + which);
  p->enc_fused[which] = false;
  DVP_TRY(prover_msm_partial(p, which, 0, dvp_prover_msm_size(p, which), d_out_xy, d_out_inf, own ? p->blk->enc + 30 * which : nullptr, stream));
  p->enc_fused[which] = own;
  return DVP_OK;
}
// window size / window count the fixed-base context of MSM `which` settled on (0,0 before its first use)
extern "C" int dvp_prover_msm_plan(const dvp_prover* p, int which, int* c_bits, int* windows) {
  if (!p || (which != 0 && which != 1) || !c_bits || !windows) return DVP_EINVAL;
  *c_bits = 0;
  *windows = 0;
  if (p->fx[which]) return msm_fixed_info(p->fx[which], c_bits, windows);
  if (!p->shards.empty() && p->shards[0].fx[which]) return msm_fixed_info(p->shards[0].fx[which], c_bits, windows);  // multi-GPU: shard 0's
  return DVP_OK;
}
// HBM held by the fixed-base table(s) of MSM `which` (all shards); *signed_windows = 1 for the default signed binary windows
extern "C" uint64_t dvp_prover_msm_table_bytes(const dvp_prover* p, int which, int* signed_windows) {
  if (signed_windows) *signed_windows = 0;
  if (!p || (which != 0 && which != 1)) return 0;
  uint64_t total = msm_fixed_table_bytes(p->fx[which], signed_windows);
  for (const auto& sh : p->shards) {
    int s = 0;
    total += msm_fixed_table_bytes(sh.fx[which], &s);
    if (s && signed_windows) *signed_windows = 1;
  }
  return total;
}
// dvp_prover_set_table_budget: tables that no longer fit are released now, the rest follows the new plan at the next proof
extern "C" int dvp_prover_set_table_budget(dvp_prover* p, uint64_t bytes) {
  if (!p) return DVP_EINVAL;
  p->table_budget = bytes;
  p->table_refused[0] = p->table_refused[1] = false;  // a new budget is the one occasion to ask the runtime again
  shards_release(p);                                  // rebuilt under the new budget by the next sharded proof
  size_t pc[2] = {0, 0};
  uint64_t pb[2] = {UINT64_MAX, UINT64_MAX};
  if (bytes != UINT64_MAX) DVP_TRY(dvp_table_plan(dvp_prover_msm_size(p, 0), dvp_prover_msm_size(p, 1), bytes, pc, pb));
  for (int w = 0; w < 2; ++w)
    if (p->fx[w] && msm_fixed_table_bytes(p->fx[w], nullptr) > pb[w]) {
      msm_fixed_destroy(p->fx[w]);
      p->fx[w] = nullptr;
    }
  return DVP_OK;
}
extern "C" int dvp_prover_msm_coverage(const dvp_prover* p, int which, size_t* covered, size_t* total, int* reason) {
  if (!p || (which != 0 && which != 1) || !covered || !total || !reason) return DVP_EINVAL;
  const size_t n = dvp_prover_msm_size(p, which);
  const size_t fixed_min = (size_t)(tune().msm_fixed_min > 0 ? tune().msm_fixed_min : 1);
  const size_t full = n >= fixed_min && n < ((size_t)1 << 27) ? n : 0;  // what no budget at all would put into tables
  size_t pc[2];
  uint64_t pb[2];
  DVP_TRY(dvp_table_plan(dvp_prover_msm_size(p, 0), dvp_prover_msm_size(p, 1), p->table_budget, pc, pb));
  size_t cov = pc[which];
  if (!p->shards.empty()) {  // in-library multi-GPU: the leading shards that hold a table
    cov = 0;
    for (const auto& sh : p->shards) {
      if (!sh.fx[which]) break;
      cov += sh.hi[which] - sh.lo[which];
    }
  }
  if (p->table_refused[which] && p->shards.empty()) cov = 0;
  *covered = cov;
  *total = n;
  *reason = p->table_refused[which] ? 2 : (cov >= full ? 0 : 1);
  return DVP_OK;
}
// the table the first pair round of MSM `which` gathers from on the home device (bench.py points dvp_ubench_gather at it)
extern "C" int dvp_prover_msm_table_ptr(const dvp_prover* p, int which, const void** d_table, uint64_t* bytes) {
  if (!p || (which != 0 && which != 1) || !d_table || !bytes) return DVP_EINVAL;
  *d_table = msm_fixed_table_ptr(p->fx[which]);
  *bytes = msm_fixed_table_bytes(p->fx[which], nullptr);
  return DVP_OK;
}
extern "C" size_t dvp_prover_msm_size(const dvp_prover* p, int which) {
  if (!p) return 0;
  return which ? 4 * (size_t)p->m : (size_t)p->n_wires + p->m;
}
