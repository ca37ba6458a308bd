// BLAKE3 (hash mode) of a large DEVICE buffer: the 1 KiB chunks are independent, so one lane hashes one chunk (k_b3_leaves) and the
// chaining values are then combined pairwise, nine levels per launch (k_b3_tree).  Written from the BLAKE3 specification on top of
// b3d::compress (blake3_dev.cuh); checked against the host flavour (blake3.h) and the oracle's long vectors in tests/.
//
// Why one lane per chunk, loading straight from global memory: the sixteen blocks of a chunk are sequential, a
// compression is ~800 integer instructions per 64 bytes (~12 per byte -- the ALUs, not HBM, bound this kernel), and the half line a lane
// leaves behind is the half it reads next, one compression later, while the line is still in L2.  Staging whole chunks through LDS would
// make every load a full line but needs 64 KiB of LDS per wave (two waves per CU) for a kernel that lives on occupancy.
#include <algorithm>

#include "blake3_dev.cuh"
#include "common.h"
#include "host_api.h"

namespace dvp {

constexpr uint32_t B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8;
constexpr uint32_t B3_CHUNK = 1024;
constexpr uint32_t B3_TREE_RUN = 512;  // chaining values one workgroup of k_b3_tree reduces to one: nine levels per launch
constexpr uint32_t B3_TREE_THREADS = B3_TREE_RUN / 2;
__device__ constexpr uint32_t B3_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};

// the 64 bytes at q as 16 little-endian words.  q is `shift` (0..3, the same for every block of a launch) bytes past a 4-byte boundary:
// 16 (17 when shift != 0) aligned dwords from q - shift, funnel-shifted.  Reads [q - shift, q + 64 + (shift ? 4 - shift : 0)).
__device__ __forceinline__ void b3_load_block(const uint8_t* q, uint32_t shift, uint32_t w[17]) {
  const uint32_t* a = (const uint32_t*)(q - shift);
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = a[i];
  w[16] = shift ? a[16] : 0u;
}
__device__ __forceinline__ void b3_shift_block(const uint32_t w[17], uint32_t shift, uint32_t blk[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) blk[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], shift);
}
// the ragged end: n < 64 bytes (or a full block too close to the end of the buffer for the dword loads), byte by byte, zero-padded
__device__ __forceinline__ void b3_load_tail(const uint8_t* q, uint32_t n, uint32_t blk[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((uint32_t)(4 * i + k) < n) v |= (uint32_t)q[4 * i + k] << (8 * k);
    blk[i] = v;
  }
}

// chaining value of chunk c of data[0, len) -> out[8 c ..], chunk counter chunk_base + c.  root != 0 (a whole input of at most one
// chunk): the last block carries ROOT and out receives the digest.  Nothing at or beyond data + len is read; up to three bytes in front
// of data are (the aligned dword its first byte lies in).
__global__ void __launch_bounds__(64) k_b3_leaves(const uint8_t* __restrict__ data, size_t len, uint32_t chunk_base, size_t nchunks, uint32_t root,
                                                  uint32_t* __restrict__ out) {
  const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= nchunks) return;
  const uint8_t* p = data + c * B3_CHUNK;
  const size_t rem = len - c * B3_CHUNK;  // bytes from p to the end of the buffer
  const uint32_t clen = rem < B3_CHUNK ? (uint32_t)rem : B3_CHUNK;
  const uint32_t nblk = clen ? (clen + 63) / 64 : 1;
  const uint32_t shift = (uint32_t)((uintptr_t)data & 3);
  // block b may take the dword loads when it is full and the 17th dword ends inside the buffer
  auto fast = [&](uint32_t b) { return 64 * (b + 1) <= clen && (shift == 0 || rem - 64 * b + shift >= 68); };
  uint32_t cv[8], w[17], wn[17];
#pragma unroll
  for (int i = 0; i < 8; ++i) cv[i] = B3_IV[i];
#pragma unroll
  for (int i = 0; i < 17; ++i) w[i] = wn[i] = 0;
  if (fast(0)) b3_load_block(p, shift, w);
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; ++b) {
    const bool last = b + 1 == nblk;
    const uint32_t blen = last ? clen - 64 * b : 64u;
    uint32_t blk[16];
    if (fast(b)) b3_shift_block(w, shift, blk);
    else b3_load_tail(p + 64 * b, blen, blk);
    if (!last && fast(b + 1)) b3_load_block(p + 64 * (b + 1), shift, wn);  // in flight during this block's compression
    b3d::compress(cv, blk, blen, (b == 0 ? B3_CHUNK_START : 0u) | (last ? (B3_CHUNK_END | (root ? B3_ROOT : 0u)) : 0u), chunk_base + (uint32_t)c);
#pragma unroll
    for (int i = 0; i < 17; ++i) w[i] = wn[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) out[8 * c + i] = cv[i];
}

// One workgroup reduces the aligned run in[RUN g, RUN g + cnt) of chaining values to one, pairwise, level by level; an odd last value
// is carried up unchanged -- on aligned power-of-two runs that is BLAKE3's rule (the left subtree is the largest power of two).  final
// != 0 (a single workgroup, n <= RUN): the last compression carries ROOT and out receives the digest.
__global__ void __launch_bounds__(B3_TREE_THREADS) k_b3_tree(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out, uint32_t final) {
  __shared__ uint32_t cv[B3_TREE_RUN * 8];
  const size_t base = (size_t)blockIdx.x * B3_TREE_RUN;
  uint32_t cnt = n - base < B3_TREE_RUN ? (uint32_t)(n - base) : B3_TREE_RUN;
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < cnt * 8; i += B3_TREE_THREADS) cv[i] = in[base * 8 + i];
  __syncthreads();
  while (cnt > 1) {
    const uint32_t half = cnt >> 1, odd = cnt & 1;
    const bool act = t < half, carry = odd && t == half;
    uint32_t r[8];
    if (act) {
      uint32_t blk[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) blk[i] = cv[16 * t + i];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = B3_IV[i];
      b3d::compress(r, blk, 64, B3_PARENT | ((final && cnt == 2) ? B3_ROOT : 0u));
    } else if (carry) {
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = cv[8 * (cnt - 1) + i];
    }
    __syncthreads();
    if (act || carry) {
#pragma unroll
      for (int i = 0; i < 8; ++i) cv[8 * t + i] = r[i];
    }
    __syncthreads();
    cnt = half + odd;
  }
  if (t < 8) out[(size_t)blockIdx.x * 8 + t] = cv[t];
}

// ---- host side (prove.hip's SRS hash hashes its staging windows through these two) -------------------------------------------------
// chaining values of the chunks of d_data[0, len), len > 0, which is the piece of a longer stream that starts at chunk chunk_base
// (so at a multiple of 1024 bytes of it) -> d_cvs[8 k ..] for the piece's k-th chunk
int b3_leaves_dev(const uint8_t* d_data, size_t len, uint64_t chunk_base, uint32_t* d_cvs, hipStream_t st) {
  const size_t nchunks = (len + B3_CHUNK - 1) / B3_CHUNK;
  if (!len || chunk_base + nchunks > (1ull << 32)) return DVP_EINVAL;  // compress carries a 32-bit chunk counter
  DVP_LAUNCH(k_b3_leaves, dim3(cdiv(nchunks, 64)), dim3(64), 0, st, d_data, len, (uint32_t)chunk_base, nchunks, 0u, d_cvs);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}
// digest of a single chunk (len <= 1024; len = 0 is one empty chunk): ROOT on its own last block
int b3_single_chunk_dev(const uint8_t* d_data, size_t len, uint32_t* d_out32, hipStream_t st) {
  if (len > B3_CHUNK) return DVP_EINVAL;
  DVP_LAUNCH(k_b3_leaves, dim3(1), dim3(64), 0, st, d_data, len, 0u, (size_t)1, 1u, d_out32);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}
size_t b3_reduce_tmp_bytes(size_t n) { return ((n + B3_TREE_RUN - 1) / B3_TREE_RUN) * 32; }
// n >= 2 chaining values -> the digest.  d_cvs is overwritten; d_tmp holds b3_reduce_tmp_bytes(n).
int b3_reduce_dev(uint32_t* d_cvs, size_t n, uint32_t* d_tmp, uint32_t* d_out32, hipStream_t st) {
  if (n < 2) return DVP_EINVAL;
  uint32_t *src = d_cvs, *dst = d_tmp;
  for (;;) {
    const size_t nb = (n + B3_TREE_RUN - 1) / B3_TREE_RUN;
    const bool last = nb == 1;
    DVP_LAUNCH(k_b3_tree, dim3((unsigned)nb), dim3(B3_TREE_THREADS), 0, st, (const uint32_t*)src, n, last ? d_out32 : dst, last ? 1u : 0u);
    DVP_HIP(hipGetLastError());
    if (last) return DVP_OK;
    n = nb;
    std::swap(src, dst);
  }
}

}  // namespace dvp

using namespace dvp;

extern "C" int dvp_blake3_dev(const void* d_data, size_t len, void* d_out32, void* stream) {
  if (!d_out32 || (len && !d_data) || len > ((size_t)1 << 40)) return DVP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (len <= B3_CHUNK) return b3_single_chunk_dev((const uint8_t*)d_data, len, (uint32_t*)d_out32, st);
  const size_t nchunks = (len + B3_CHUNK - 1) / B3_CHUNK;
  void* scratch = nullptr;  // the chaining values (len / 32 bytes) and the first tree level's output behind them, ordered on the stream
  DVP_HIP(hipMallocAsync(&scratch, nchunks * 32 + b3_reduce_tmp_bytes(nchunks), st));
  uint32_t* cvs = (uint32_t*)scratch;
  int rc = b3_leaves_dev((const uint8_t*)d_data, len, 0, cvs, st);
  if (rc == DVP_OK) rc = b3_reduce_dev(cvs, nchunks, cvs + 8 * nchunks, (uint32_t*)d_out32, st);
  hipError_t e = hipFreeAsync(scratch, st);
  if (rc == DVP_OK && e != hipSuccess) return hip_fail(e, "hipFreeAsync", __FILE__, __LINE__);
  return rc;
}

// TEST ONLY (include/dvpari_internal.h): the two halves of dvp_blake3_dev apart, so that a stream can be hashed piecewise
extern "C" uint32_t dvp_debug_blake3_tree_run(void) { return B3_TREE_RUN; }
extern "C" int dvp_debug_blake3_leaves_dev(const void* d_data, size_t len, uint64_t chunk_base, void* d_cvs, void* stream) {
  if (!d_data || !d_cvs) return DVP_EINVAL;
  return b3_leaves_dev((const uint8_t*)d_data, len, chunk_base, (uint32_t*)d_cvs, (hipStream_t)stream);
}
extern "C" int dvp_debug_blake3_reduce_dev(void* d_cvs, size_t n, void* d_tmp, void* d_out32, void* stream) {
  if (!d_cvs || !d_tmp || !d_out32) return DVP_EINVAL;
  return b3_reduce_dev((uint32_t*)d_cvs, n, (uint32_t*)d_tmp, (uint32_t*)d_out32, (hipStream_t)stream);
}
