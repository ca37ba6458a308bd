// BLAKE3 of an Fr vector as the reference serialises it (Vec<Fr>::serialize_uncompressed, the payload of write_fr_vec_to_file,
// src/io_utils.rs:42-70): n as u64 little-endian, then every entry as 29 bytes little-endian canonical.  The entries lie in HBM as 32
// bytes each (canonical or Montgomery), so the stream exists nowhere: it is packed on the device, window by window, and hashed by the
// chunk / tree hasher of blake3_tree.hip -- the scheme of the SRS hash and of the circuit hash.
//
// The stream in dwords: dwords 0 and 1 are n; behind them the 29-byte records do not lie on dwords, but four of them are 116 bytes = 29
// dwords, the unit one thread assembles in registers.  k_ch_coeffs of circuit_hash.hip packs its coefficient part the same way, in its
// own text: with the packing loop and the LDS hand-over in shared inline functions that kernel compiled to 155 VGPRs and three waves
// per SIMD instead of 110 and four, so the two stay apart (as k_verify and k_verify_trace do).  The
// stream's last dword is padded with zero bytes, which the hasher never reads: it is given the length in bytes.
// A window is a run of whole 1 KiB chunks; each is hashed by k_b3_leaves with its position in the stream as the chunk-counter base, the
// chaining values are reduced once at the end.  Scratch = the window + 32 bytes per chunk + the tree's first level: it does not grow
// with n beyond the chaining values.
#include <algorithm>

#include "common.h"
#include "fr.cuh"
#include "host_api.h"

namespace dvp {

static constexpr int FD_TPB = 256;
static constexpr uint32_t FD_GROUP_DWORDS = 29;                         // four 29-byte records
static constexpr uint32_t FD_BLOCK_DWORDS = FD_TPB * FD_GROUP_DWORDS;  // 7424 dwords = 1024 records per workgroup
static constexpr uint64_t FD_WINDOW_CHUNKS_DEFAULT = 61440;            // 60 MiB, the SRS hash's window
static constexpr uint64_t FD_WINDOW_CHUNKS_MAX = 1ull << 21;           // 2 GiB: a launch's grid stays far below 2^31 workgroups

// Dwords [lo, hi) of the stream of v[0, n) -> out[0, hi - lo).  Group g of four records fills dwords 2 + 29 g .. 2 + 29 g + 28; the
// workgroup owns groups group0 + 256 blockIdx .. + 255.  A thread assembles one group in registers (records at or beyond n are zero
// bytes: the pad of the stream's last dword), the workgroup's 7424 dwords meet in LDS (stride 29 dwords per thread: odd, no bank
// conflict) and leave in order, each only if inside [lo, hi).  v is read below n only, out is written inside [0, hi - lo) only.
// The packing loop and the LDS hand-over are k_ch_coeffs' (circuit_hash.hip), copied: a fix to one belongs in the other.
template <bool MONT>
__global__ void __launch_bounds__(FD_TPB)
k_frd_pack(const Fr* __restrict__ v, uint64_t n, uint64_t group0, uint64_t lo, uint64_t hi, uint32_t* __restrict__ out) {
  __shared__ uint32_t stage[FD_BLOCK_DWORDS];
  const uint64_t block_group = group0 + (uint64_t)blockIdx.x * FD_TPB;
  const uint64_t rec0 = 4 * (block_group + threadIdx.x);
  uint32_t w[FD_GROUP_DWORDS];
#pragma unroll
  for (int e = 0; e < (int)FD_GROUP_DWORDS; ++e) w[e] = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t R = rec0 + r;
    Fr val = fr_zero();
    if (R < n) val = MONT ? fr_from_mont(v[R]) : v[R];
    // 29 bytes at byte 29 r of the group = dword 7 r, shifted by r bytes
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      const uint32_t x = l == 7 ? (val.v[7] & 0xffu) : val.v[l];
      w[7 * r + l] |= x << (8 * r);
      if (r > 0 && 7 * r + l + 1 < (int)FD_GROUP_DWORDS) w[7 * r + l + 1] |= x >> (32 - 8 * r);
    }
  }
#pragma unroll
  for (int e = 0; e < (int)FD_GROUP_DWORDS; ++e) stage[FD_GROUP_DWORDS * threadIdx.x + e] = w[e];
  __syncthreads();
  const uint64_t q0 = 2 + FD_GROUP_DWORDS * block_group;  // the workgroup's first dword of the stream
  for (uint32_t idx = threadIdx.x; idx < FD_BLOCK_DWORDS; idx += FD_TPB) {
    const uint64_t q = q0 + idx;
    if (q >= lo && q < hi) out[q - lo] = stage[idx];
  }
  if (blockIdx.x == 0 && threadIdx.x < 2 && threadIdx.x >= lo && threadIdx.x < hi) out[threadIdx.x - lo] = (uint32_t)(n >> (32 * threadIdx.x));
}

// the plan of one digest: chunks of the stream, chunks of the window, and where the three regions of the scratch lie
struct FdPlan {
  uint64_t total_bytes, total_dwords, nchunks, win_chunks;
  size_t off_cvs, off_tmp, bytes;
};
static FdPlan fd_plan(size_t n) {
  FdPlan p;
  p.total_bytes = 8 + 29 * (uint64_t)n;
  p.total_dwords = (p.total_bytes + 3) / 4;
  p.nchunks = (p.total_bytes + 1023) / 1024;
  const long long knob = tune().fr_digest_window;
  const uint64_t want = knob > 0 ? std::min<uint64_t>((uint64_t)knob, FD_WINDOW_CHUNKS_MAX) : FD_WINDOW_CHUNKS_DEFAULT;
  p.win_chunks = std::min(want, p.nchunks);
  Carver c;
  c.take(p.win_chunks * 1024);
  p.off_cvs = c.take(p.nchunks > 1 ? p.nchunks * 32 : 0);
  p.off_tmp = c.take(p.nchunks > 1 ? b3_reduce_tmp_bytes(p.nchunks) : 0);
  p.bytes = c.o;
  return p;
}
size_t fr_digest_work_bytes(size_t n) { return fd_plan(n).bytes; }

int fr_vec_digest_dev(const Fr* d_fr, size_t n, bool montgomery, void* d_work, uint32_t* d_out32, hipStream_t st) {
  if ((n && !d_fr) || !d_work || !d_out32 || n > ((size_t)1 << 36)) return DVP_EINVAL;
  const FdPlan p = fd_plan(n);
  if (p.nchunks > (1ull << 32)) return DVP_EINVAL;  // 32-bit chunk counter
  uint32_t* w = (uint32_t*)d_work;
  uint32_t* cvs = (uint32_t*)((char*)d_work + p.off_cvs);
  uint32_t* tmp = (uint32_t*)((char*)d_work + p.off_tmp);
  for (uint64_t c0 = 0; c0 < p.nchunks; c0 += p.win_chunks) {
    const uint64_t lo = c0 * 256, hi = std::min((c0 + p.win_chunks) * 256, p.total_dwords);  // the window's dwords of the stream
    const uint64_t g0 = lo > 2 ? (lo - 2) / FD_GROUP_DWORDS : 0, g1 = hi > 2 ? (hi - 3) / FD_GROUP_DWORDS + 1 : 0;  // groups touched
    const dim3 grid(g1 > g0 ? cdiv(g1 - g0, FD_TPB) : 1);
    if (montgomery) DVP_LAUNCH(k_frd_pack<true>, grid, dim3(FD_TPB), 0, st, d_fr, (uint64_t)n, g0, lo, hi, w);
    else DVP_LAUNCH(k_frd_pack<false>, grid, dim3(FD_TPB), 0, st, d_fr, (uint64_t)n, g0, lo, hi, w);
    DVP_HIP(hipGetLastError());
    const uint64_t len = std::min((c0 + p.win_chunks) * 1024, p.total_bytes) - c0 * 1024;
    if (p.nchunks == 1) DVP_TRY(b3_single_chunk_dev((const uint8_t*)w, len, d_out32, st));
    else DVP_TRY(b3_leaves_dev((const uint8_t*)w, len, c0, cvs + 8 * c0, st));
  }
  if (p.nchunks > 1) DVP_TRY(b3_reduce_dev(cvs, p.nchunks, tmp, d_out32, st));
  return DVP_OK;
}

}  // namespace dvp

using namespace dvp;

extern "C" int dvp_fr_vec_digest_dev(const void* d_fr, size_t n, int montgomery, void* d_out32, void* stream) {
  if ((n && !d_fr) || !d_out32) return DVP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  void* work = nullptr;  // ordered on the stream, as dvp_blake3_dev's chaining values are
  DVP_HIP(hipMallocAsync(&work, fr_digest_work_bytes(n), st));
  const int rc = fr_vec_digest_dev((const Fr*)d_fr, n, montgomery != 0, work, (uint32_t*)d_out32, st);
  const hipError_t e = hipFreeAsync(work, st);
  if (rc == DVP_OK && e != hipSuccess) return hip_fail(e, "hipFreeAsync", __FILE__, __LINE__);
  return rc;
}

extern "C" int dvp_fr_vec_digest(const uint64_t* limbs, size_t n, uint8_t out[32]) {
  if ((n && !limbs) || !out) return DVP_EINVAL;
  DVP_TRY(scalars_in_range(limbs, n));
  DevBuf dv, dout;
  DVP_TRY(dv.up(limbs, n * 32));
  DVP_TRY(dout.alloc(32));
  DVP_TRY(dvp_fr_vec_digest_dev(dv.p, n, 0, dout.p, nullptr));
  return dout.down(out, 32);  // on the null stream, behind the digest
}
