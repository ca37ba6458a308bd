// MSM test-only and microbenchmark C entries (include/dvpari_internal.h): dvp_debug_wave_trace, dvp_ubench_gf_mul, dvp_ubench_gather
// (with k_ubench_gather), dvp_debug_msm_rest_len, dvp_debug_msm_capture_arm / _fetch, dvp_debug_recode_signed.  No product entry lives
// here.  Unlike its msm_*.cuh siblings this is not a self-contained header but the tail of msm.hip kept apart: the entries read
// msm.hip's own host state (the wave-trace buffer, the workspaces, g_last_msm, g_capture, MsmFixedCtx), so msm.hip includes it once,
// at global scope behind its `using namespace dvp`, where the text stood; k_ubench_gather therefore stays outside namespace dvp.
#pragma once
#include "common.h"
#include "msm_recode.cuh"
#include "msm_reduce.cuh"
#include "msm_merge.cuh"

// GF(2^233) products per second of the hot kernels' multiplier alone (every CU busy, k_affine_round's occupancy): the
// ceiling bench.py's work model divides by, measured in the same process instead of quoted
// d_buf: device buffer of 64 + 64 * n_records bytes, zeroed by the caller (word 0 counts the records); NULL switches the trace off.
// While set, every pair round runs its TRACE instantiation and appends one record per wave (layout: WaveTrace above).
extern "C" int dvp_debug_wave_trace(void* d_buf, uint32_t n_records) {
  {
    std::lock_guard<std::mutex> g(g_wave_trace_mu);
    g_wave_trace_cap = d_buf ? n_records : 0;
    g_wave_trace_buf = (unsigned long long*)d_buf;
    g_wave_trace_tag.store(0);
  }
  // switching the trace off (or to another buffer): launches that took the old snapshot may still be writing into it -- the caller
  // is about to free it
  DVP_HIP(hipDeviceSynchronize());
  return DVP_OK;
}

extern "C" int dvp_ubench_gf_mul(int reps, double* products_per_s) {
  if (reps < 1 || !products_per_s) return DVP_EINVAL;
  int dev = 0, n_cu = 256;
  DVP_HIP(hipGetDevice(&dev));
  DVP_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  const int blocks = n_cu * 3 * 8;  // eight chip-fulls of 3 blocks per CU
  DevBuf out;
  DVP_TRY(out.alloc((size_t)blocks * EC_TPB * sizeof(Gf)));
  hipEvent_t e0, e1;
  DVP_HIP(hipEventCreate(&e0));
  DVP_HIP(hipEventCreate(&e1));
  float best = 1e30f;
  for (int it = 0; it < 3; ++it) {
    DVP_HIP(hipEventRecord(e0, 0));
    DVP_LAUNCH(k_ubench_mul, dim3(blocks), dim3(EC_TPB), EC_LDS, 0, out.as<Gf>(), reps);
    DVP_HIP(hipEventRecord(e1, 0));
    DVP_HIP(hipEventSynchronize(e1));
    float ms = 0;
    DVP_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best) best = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  DVP_HIP(hipGetLastError());
  *products_per_s = (double)blocks * EC_TPB * reps / (best * 1e-3);
  return DVP_OK;
}

// Random 64-byte gathers per second out of a device table (tools/ubench/gather.hip moved behind the ABI so that bench.py
// measures the ceiling of the first pair round's gathers in the same run, on the prover's own table): every lane reads
// whole 64-byte lines at hashed positions, four independent lines in flight per lane (the pair round keeps the two
// operands of the next slot in flight behind the current one's), at full occupancy -- the most the memory system gives.
__device__ __forceinline__ uint64_t ubench_mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__global__ void __launch_bounds__(256) k_ubench_gather(const uint4* __restrict__ t, uint64_t nlines, int per, uint32_t seed, uint32_t* __restrict__ out) {
  const uint64_t tid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll 4
  for (int k = 0; k < per; ++k) {
    const uint64_t idx = ubench_mix(tid * (uint64_t)per + k + ((uint64_t)seed << 40)) % nlines;
    const uint4* p = t + idx * 4;
    const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
    acc.x ^= a.x ^ b.x ^ c.x ^ d.x; acc.y ^= a.y ^ b.y ^ c.y ^ d.y; acc.z ^= a.z ^ b.z ^ c.z ^ d.z; acc.w ^= a.w ^ b.w ^ c.w ^ d.w;
  }
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) out[0] = 1;  // keeps the loads alive
}
extern "C" int dvp_ubench_gather(const void* d_table, size_t table_bytes, int reps, double* gathers_per_s) {
  if (reps < 1 || reps > 64 || !gathers_per_s || table_bytes < (1u << 20)) return DVP_EINVAL;
  int dev = 0, n_cu = 256;
  DVP_HIP(hipGetDevice(&dev));
  DVP_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  DevBuf own, out;
  if (!d_table) {  // contents do not matter for a read-rate figure, but untouched pages may not be backed: write them once
    DVP_TRY(own.alloc(table_bytes));
    DVP_HIP(hipMemset(own.p, 0x5a, table_bytes));
    d_table = own.p;
  }
  DVP_TRY(out.alloc(16));
  const int per = 32;
  const uint32_t blocks = (uint32_t)n_cu * 3 * 8;
  const uint64_t nlines = table_bytes / 64;
  hipEvent_t e0, e1;
  DVP_HIP(hipEventCreate(&e0));
  DVP_HIP(hipEventCreate(&e1));
  DVP_LAUNCH(k_ubench_gather, dim3(blocks), dim3(256), 0, 0, (const uint4*)d_table, nlines, per, 1u, out.as<uint32_t>());
  DVP_HIP(hipEventRecord(e0, 0));
  for (int r = 0; r < reps; ++r)
    DVP_LAUNCH(k_ubench_gather, dim3(blocks), dim3(256), 0, 0, (const uint4*)d_table, nlines, per, 2u + (uint32_t)r, out.as<uint32_t>());
  DVP_HIP(hipEventRecord(e1, 0));
  DVP_HIP(hipEventSynchronize(e1));
  float ms = 0;
  DVP_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  DVP_HIP(hipGetLastError());
  *gathers_per_s = (double)reps * blocks * 256.0 * per / (ms * 1e-3);
  return DVP_OK;
}


// the signed aligned windows (k_recode_signed): out_words[w * n + i] = 0 (digit 0) or 0x80000000 | 0x10000000 if the digit is
// negative | w << 20 | |digit| (|digit| = 2^(c-1) stored as key 0); *windows = ceil(234 / c)
// entries the device put on the rest list (k_bucket_pairs' buckets, k_accum_affine_fast's tasks) during the calling thread's last MSM:
// the tail kernel keeps the control word before it clears it for the next MSM
extern "C" int dvp_debug_msm_rest_len(uint32_t* n) {
  using namespace dvp;
  if (!n) return DVP_EINVAL;
  const LastMsm lm = g_last_msm;
  if (lm.dev < 0) return DVP_EINVAL;  // this thread has run no MSM
  MsmWorkspace& ws = g_ws_dev[lm.dev][lm.slot];
  std::lock_guard<std::mutex> g(ws.mu);
  if (!ws.p || ws.device != lm.dev) return DVP_EINVAL;
  int prev = 0;
  DVP_HIP(hipGetDevice(&prev));
  if (prev != lm.dev) DVP_HIP(hipSetDevice(lm.dev));
  hipError_t e = hipStreamSynchronize(lm.st);
  uint32_t w[2] = {0, 0};  // (d_max, rest_n)
  if (e == hipSuccess) e = hipMemcpy(w, (const char*)ws.p + 24, 8, hipMemcpyDeviceToHost);
  if (prev != lm.dev) (void)hipSetDevice(prev);
  DVP_HIP(e);
  *n = w[1];
  return DVP_OK;
}

// the stage capture (include/dvpari_internal.h; MsmCapture above)
extern "C" int dvp_debug_msm_capture_arm(size_t arena_bytes) {
  using namespace dvp;
  MsmCapture& c = g_capture;
  c.release();  // a capture nobody fetched, or an arming no MSM followed
  if (!arena_bytes) return DVP_OK;  // disarm
  DVP_HIP(hipMalloc((void**)&c.arena, arena_bytes));
  c.cap = arena_bytes;
  memset(c.hdr, 0, sizeof c.hdr);
  c.cnt = c.off = c.items = c.bkt = c.save0 = c.parts = c.res_xy = c.res_inf = c.res_enc = MsmCapture::Sec{0, 0};
  c.armed = true;
  return DVP_OK;
}
extern "C" int dvp_debug_msm_capture_fetch(void* out, size_t cap_bytes, size_t* need) {
  using namespace dvp;
  MsmCapture& c = g_capture;
  if (need) *need = 0;
  if (!c.taken) return DVP_EINVAL;  // this thread's last armed MSM did not run, or failed before its buckets were reduced
  int prev = 0;
  DVP_HIP(hipGetDevice(&prev));
  if (prev != c.dev) DVP_HIP(hipSetDevice(c.dev));
  hipError_t e = hipStreamSynchronize(c.st);
  std::vector<uint32_t> a;
  const bool fits = c.wanted <= c.cap;
  if (e == hipSuccess && c.copy_err != hipSuccess) e = c.copy_err;
  if (e == hipSuccess && fits) {
    a.resize((c.used + 3) / 4);
    if (c.used) e = hipMemcpy(a.data(), c.arena, c.used, hipMemcpyDeviceToHost);
  }
  if (prev != c.dev) (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    c.release();
    DVP_HIP(e);
  }
  if (!fits) {  // no partial blob: the arena the MSM wanted is reported instead
    g_last_error_index = (int64_t)c.wanted;
    c.release();
    return DVP_EINVAL;
  }
  // the lengths the device settled on, read from the captured offsets
  auto word = [&](const MsmCapture::Sec& s, size_t i) { return a[s.at / 4 + i]; };
  const uint32_t nk = c.hdr[CH_NKEYS], ra = c.hdr[CH_RA];
  const bool dense = c.hdr[CH_DENSE] != 0;
  const uint32_t levels = c.hdr[CH_LEVELS], nparts = c.hdr[CH_NPARTS];
  const bool has_save0 = c.hdr[CH_SIGN_MASK] != 0, has_enc = c.hdr[CH_ENC] != 0;
  bool ok = ra == c.nrounds && c.bkt.bytes == (size_t)nk * sizeof(Ld);
  // the merge tree and the tail: every region has the length the host knew when it enqueued the copy
  ok = ok && c.result && levels == c.nlevels && c.save0.bytes == (has_save0 ? sizeof(Ld) : 0) && c.parts.bytes == (size_t)nparts * sizeof(Ld) &&
       c.res_xy.bytes == 64 && c.res_inf.bytes == 4 && c.res_enc.bytes == (has_enc ? 30u : 0u);
  for (uint32_t j = 0; ok && j < levels; ++j) ok = c.levels[j].bytes == (size_t)nk * sizeof(Ld);
  const size_t items_len = word(c.off, nk);
  ok = ok && items_len * 4 <= c.items.bytes;
  size_t words = CAPTURE_HDR_WORDS + (size_t)nk + (nk + 1) + items_len + (size_t)nk * (sizeof(Ld) / 4);
  for (uint32_t r = 0; ok && r < ra; ++r) {
    const size_t total = word(c.rounds[r].ooff, nk), dw = r == 0 ? 0 : (dense ? 2 : 1) * total;
    ok = total * sizeof(Aff) <= c.rounds[r].pts.bytes && dw * 4 <= c.rounds[r].desc.bytes;
    c.hdr[CH_TOTAL + r] = (uint32_t)total;
    words += (size_t)nk + (nk + 1) + dw + total * (sizeof(Aff) / 4);
  }
  words += (size_t)levels * nk * (sizeof(Ld) / 4) + (has_save0 ? sizeof(Ld) / 4 : 0) + (size_t)nparts * (sizeof(Ld) / 4) + 16 + 1 + (has_enc ? 8 : 0);
  if (!ok) {  // cannot happen: every region was copied at its upper bound
    c.release();
    return DVP_EHIP;
  }
  c.hdr[CH_ITEMS_LEN] = (uint32_t)items_len;
  if (need) *need = words * 4;
  if (!out) return DVP_OK;  // the size alone; the capture stays
  if (cap_bytes < words * 4) return DVP_EINVAL;  // nothing written; the capture stays
  uint32_t* o = (uint32_t*)out;
  auto put = [&](const void* src, size_t n_words) { memcpy(o, src, n_words * 4); o += n_words; };
  auto sec = [&](const MsmCapture::Sec& s, size_t n_words) { put(a.data() + s.at / 4, n_words); };
  put(c.hdr, CAPTURE_HDR_WORDS);
  sec(c.cnt, nk);
  sec(c.off, (size_t)nk + 1);
  sec(c.items, items_len);
  for (uint32_t r = 0; r < ra; ++r) {
    const size_t total = c.hdr[CH_TOTAL + r];
    sec(c.rounds[r].ocnt, nk);
    sec(c.rounds[r].ooff, (size_t)nk + 1);
    sec(c.rounds[r].desc, r == 0 ? 0 : (dense ? 2 : 1) * total);
    sec(c.rounds[r].pts, total * (sizeof(Aff) / 4));
  }
  sec(c.bkt, (size_t)nk * (sizeof(Ld) / 4));
  for (uint32_t j = 0; j < levels; ++j) sec(c.levels[j], (size_t)nk * (sizeof(Ld) / 4));
  if (has_save0) sec(c.save0, sizeof(Ld) / 4);
  sec(c.parts, (size_t)nparts * (sizeof(Ld) / 4));
  sec(c.res_xy, 16);
  sec(c.res_inf, 1);
  if (has_enc) {  // 30 bytes in 8 words, the last two bytes zero
    uint32_t enc[8] = {0};
    memcpy(enc, (const char*)a.data() + c.res_enc.at, 30);
    put(enc, 8);
  }
  c.release();
  return DVP_OK;
}

extern "C" int dvp_debug_recode_signed(const uint64_t* scalars, size_t n, int c, uint32_t* out_words, int* windows) {
  if (!windows || c < 8 || c > FX_C_MAX + 1 || n > (1u << 24)) return DVP_EINVAL;
  MsmFixedCtx plan;
  plan.set_c_signed(c);
  if (plan.c != c) return DVP_EINVAL;  // a window size whose windows would all be one bit narrower: ask for c - 1
  *windows = plan.W;
  if (!out_words) return DVP_OK;
  if (!scalars || !n) return DVP_EINVAL;
  DevBuf ds, dw, de;
  DVP_TRY(ds.up(scalars, n * 32));
  DVP_TRY(dw.alloc((size_t)*windows * n * 4));
  DVP_TRY(de.alloc(8));
  DVP_HIP(hipMemset(de.p, 0xff, 8));
  DVP_LAUNCH(k_recode_signed, dim3(cdiv(n, 256)), dim3(256), 0, 0, ds.as<uint32_t>(), (const uint8_t*)nullptr, (uint32_t)n, c, *windows, plan.n_narrow,
                     dw.as<uint32_t>(), de.as<unsigned long long>());
  DVP_HIP(hipGetLastError());
  DVP_TRY(dw.down(out_words, (size_t)*windows * n * 4));
  unsigned long long e = 0;
  DVP_TRY(de.down(&e, 8));
  if (e != ~0ull) {
    g_last_error_index = (int64_t)(e & 0xffffffffull);
    return DVP_EINVAL;
  }
  return DVP_OK;
}
