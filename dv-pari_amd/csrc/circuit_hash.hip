// The circuit half of the transcript binding: BLAKE3 of the stream the commented-out body of Transcript::circuit_info_hash would build
// (src/proving.rs:111-134) on the instance after update_to_include_vandermode_matrix_d (src/gnark_r1cs.rs:333-386), generated on the
// device from what a prover already holds -- the three CSR matrices, the coefficient table and the domain D -- and never materialised.
//
// The stream ("Circuit hash"): m = constraints, k = public inputs, c[0, n0) the coefficient table, d_i the i-th element of D.
//   i1 = first index with c[i1] == p - 1; none: i1 = n0 and p - 1 is appended (n1 = n0 + 1, otherwise n1 = n0), for k = 0 as well;
//   the updated table is c[0, n1) followed by -(d_i^j) at index n1 + i (k - 1) + (j - 1), i in [0, m), j in [1, k): N entries.
//   row part, u32 little-endian, for i = 0 .. m - 1: the coeff_ids of row i of A, of B, of C, then (k >= 1) i1, then the Vandermonde
//     ids n1 + i (k - 1) + (j - 1), j = 1 .. k - 1.  Wire ids are NOT part of it: the reference wrote only `coeff_id`s;
//   coefficient part, Vec<Fr>::serialize_uncompressed: N as u64 little-endian, then every entry as 29 bytes little-endian canonical.
// Row i starts at dword off(i) = rpA[min(i, nA)] + rpB[min(i, nB)] + rpC[min(i, nC)] + k i of the row part: the CSR row pointers are
// the prefix sums, so the row of any output dword is found by a binary search and nothing is scanned.  The row part is whole
// dwords, so the coefficient part starts on a dword as well; its 29-byte records do not: four of them are 116 bytes = 29 dwords, the
// unit one thread assembles.
//
// As dvp_prover_srs_hash does, the stream is produced into a window of whole 1 KiB chunks, each window is hashed by k_b3_leaves with its
// chunk position as the counter base, and the chaining values are reduced once.  Device scratch = the window + 32 bytes per chunk.
#include <algorithm>

#include "common.h"
#include "fr.cuh"
#include "host_api.h"

namespace dvp {

static constexpr int CH_TPB = 256;
static constexpr uint32_t CH_ROW_TABLE = 128;                       // row offsets a workgroup of k_ch_rows keeps in LDS
static constexpr uint32_t CH_GROUP_DWORDS = 29;                    // four 29-byte records
static constexpr uint32_t CH_BLOCK_DWORDS = CH_TPB * CH_GROUP_DWORDS;  // 7424 dwords = 1024 records per workgroup
static constexpr long long CH_WINDOW_CHUNKS_DEFAULT = 61440;       // 60 MiB, the SRS hash's window

// first dword of row i of the row part, i in [0, m]
__device__ __forceinline__ uint64_t ch_row_off(const ChCsr& s, uint32_t i, uint32_t k) {
  uint64_t o = (uint64_t)k * i;
#pragma unroll
  for (int q = 0; q < 3; ++q) o += s.rp[q][i < s.n_rows[q] ? i : s.n_rows[q]];
  return o;
}
// the largest row i in [a, b] with off(i) <= g; off(a) <= g is the caller's
__device__ __forceinline__ uint32_t ch_find_row(const ChCsr& s, uint32_t k, uint64_t g, uint32_t a, uint32_t b) {
  while (a < b) {
    const uint32_t mid = a + (b - a + 1) / 2;
    if (ch_row_off(s, mid, k) <= g) a = mid;
    else b = mid - 1;
  }
  return a;
}

// The row of every 256th dword of [lo, hi) -- the first dword of each workgroup of k_ch_rows -- by bisection over all m rows, one
// thread each, left in that dword's own slot of out: k_ch_rows reads it before it writes the slot, so the search of a workgroup costs
// one lone thread's 22 dependent loads among thousands of others' and no scratch beside the window.
__global__ void __launch_bounds__(CH_TPB)
k_ch_row_starts(ChCsr s, uint32_t m, uint32_t k, uint64_t lo, uint64_t hi, uint32_t* __restrict__ out) {
  const uint64_t g0 = lo + ((uint64_t)blockIdx.x * CH_TPB + threadIdx.x) * CH_TPB;
  if (g0 >= hi) return;
  out[g0 - lo] = ch_find_row(s, k, g0, 0, m - 1);
}

// dwords [lo, hi) of the row part -> out[0, hi - lo), one thread per dword; out[256 b] holds the row of the first dword of workgroup b
// (k_ch_row_starts).  The offsets of that row and the next CH_ROW_TABLE - 1 go to LDS and each thread bisects there; a dword behind
// them (possible only where rows hold fewer than two dwords on average: no term and at most one public input) bisects the row
// pointers themselves.  A row may be empty in any matrix and may span many workgroups.
__global__ void __launch_bounds__(CH_TPB)
k_ch_rows(ChCsr s, uint32_t m, uint32_t k, uint32_t i1, uint32_t n1, uint64_t lo, uint64_t hi, uint32_t* __restrict__ out) {
  __shared__ uint32_t first_row;
  __shared__ uint64_t soff[CH_ROW_TABLE + 1];
  const uint32_t t = threadIdx.x;
  const uint64_t g0 = lo + (uint64_t)blockIdx.x * CH_TPB;  // < hi by the grid's size
  if (t == 0) first_row = out[g0 - lo];
  __syncthreads();
  const uint32_t a = first_row;  // the largest row with off <= g0
  const uint32_t nt = m - a < CH_ROW_TABLE ? m - a : CH_ROW_TABLE;  // rows a .. a + nt - 1 in LDS, soff[nt] = the end of the last
  if (t <= nt) soff[t] = ch_row_off(s, a + t, k);
  __syncthreads();
  const uint64_t g = g0 + t;
  if (g >= hi) return;
  uint32_t i;
  uint64_t row_off;
  if (g < soff[nt]) {
    uint32_t ja = 0, jb = nt - 1;
    while (ja < jb) {
      const uint32_t mid = ja + (jb - ja + 1) / 2;
      if (soff[mid] <= g) ja = mid;
      else jb = mid - 1;
    }
    i = a + ja;
    row_off = soff[ja];
  } else {  // off(a + nt) <= g < off(m): a + nt <= m - 1
    i = ch_find_row(s, k, g, a + nt, m - 1);
    row_off = ch_row_off(s, i, k);
  }
  uint64_t r = g - row_off;  // position inside row i: < its length, since off(i + 1) > g
  uint32_t v = 0;
  bool done = false;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (!done && i < s.n_rows[q]) {
      const uint32_t c0 = s.rp[q][i], len = s.rp[q][i + 1] - c0;
      if (r < len) {
        v = s.cid[q][c0 + (uint32_t)r];
        done = true;
      } else {
        r -= len;
      }
    }
  }
  if (!done) v = r == 0 ? i1 : (uint32_t)((uint64_t)n1 + (uint64_t)i * (k - 1) + (r - 1));  // N <= 2^32: every id fits
  out[g - lo] = v;
}

// index of the first coefficient equal to p - 1 -> *first (preset to ~0)
__global__ void __launch_bounds__(CH_TPB) k_ch_find_minus_one(const Fr* __restrict__ coeffs_m, uint32_t n0, unsigned long long* __restrict__ first) {
  const uint32_t i = blockIdx.x * CH_TPB + threadIdx.x;
  if (i >= n0) return;
  if (fr_eq(coeffs_m[i], fr_neg(fr_one_mont()))) atomicMin(first, (unsigned long long)i);
}

// Dwords [lo, hi) of the coefficient part -> out[0, hi - lo).  Dwords 0 and 1 are N; behind them group t of four records fills dwords
// 2 + 29 t .. 2 + 29 t + 28.  A thread assembles one group in registers (records at or beyond N are zero bytes: the pad of the stream's
// last dword), the workgroup's 7424 dwords meet in LDS (stride 29: no bank conflict) and leave in order, each only if inside [lo, hi).
// A Vandermonde entry -(d_i^j): the thread's first one by square-and-multiply (at most 2 x 32 products, whatever k), the next three by
// one product each (or a load of d_(i+1) at a row's end), so a record's cost does not grow with j.
// k_frd_pack (fr_digest.hip) holds a second copy of the packing loop and of the LDS hand-over (why two: there): a fix to one belongs in
// the other.
__global__ void __launch_bounds__(CH_TPB)
k_ch_coeffs(const Fr* __restrict__ coeffs_m, uint32_t n0, uint64_t n1 /* 2^32 at most */, const Fr* __restrict__ dom_m, uint32_t m, uint32_t k, uint64_t N,
            uint64_t group0, uint64_t lo, uint64_t hi, uint32_t* __restrict__ out) {
  __shared__ uint32_t stage[CH_BLOCK_DWORDS];
  const uint64_t block_group = group0 + (uint64_t)blockIdx.x * CH_TPB;
  const uint64_t rec0 = 4 * (block_group + threadIdx.x);
  uint32_t w[CH_GROUP_DWORDS];
#pragma unroll
  for (int e = 0; e < (int)CH_GROUP_DWORDS; ++e) w[e] = 0;
  // running Vandermonde state: pw = d_i^j (Montgomery); vi == m: not started
  uint32_t vi = m, vj = 0;
  Fr d = fr_zero(), pw = fr_zero();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t R = rec0 + r;
    Fr val = fr_zero();
    if (R < n0) {
      val = fr_from_mont(coeffs_m[R]);
    } else if (R < n1) {  // the appended p - 1
      val = fr_neg(fr_one_canon());
    } else if (R < N) {
      if (vi == m) {
        const uint64_t v = R - n1;  // < m (k - 1) <= 2^32
        vi = (uint32_t)(v / (k - 1));
        vj = 1 + (uint32_t)(v % (k - 1));
        d = dom_m[vi];
        pw = fr_pow_u64(d, vj);
      } else if (vj + 1 < k) {
        ++vj;
        pw = fr_mul(pw, d);
      } else {  // R < N: vi + 1 < m
        ++vi;
        vj = 1;
        d = dom_m[vi];
        pw = d;
      }
      val = fr_from_mont(fr_neg(pw));
    }
    // 29 bytes at byte 29 r of the group = dword 7 r, shifted by r bytes
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      const uint32_t x = l == 7 ? (val.v[7] & 0xffu) : val.v[l];
      w[7 * r + l] |= x << (8 * r);
      if (r > 0 && 7 * r + l + 1 < (int)CH_GROUP_DWORDS) w[7 * r + l + 1] |= x >> (32 - 8 * r);
    }
  }
#pragma unroll
  for (int e = 0; e < (int)CH_GROUP_DWORDS; ++e) stage[CH_GROUP_DWORDS * threadIdx.x + e] = w[e];
  __syncthreads();
  const uint64_t q0 = 2 + CH_GROUP_DWORDS * block_group;  // the workgroup's first dword of the part
  for (uint32_t idx = threadIdx.x; idx < CH_BLOCK_DWORDS; idx += CH_TPB) {
    const uint64_t q = q0 + idx;
    if (q >= lo && q < hi) out[q - lo] = stage[idx];
  }
  if (blockIdx.x == 0 && threadIdx.x < 2 && threadIdx.x >= lo && threadIdx.x < hi) out[threadIdx.x - lo] = (uint32_t)(N >> (32 * threadIdx.x));
}

// The digest -> out[32] on the host.  mats: row pointers / coefficient ids on the device (n_rows <= m each), nnz = their term counts;
// coeffs_m / dom_m: the coefficient table and D, Montgomery; window_chunks <= 0: the default.  Runs on `st` and waits for it twice: for
// the index of p - 1 (the stream's length depends on it) and for the digest.
int circuit_hash_dev(const ChCsr& mats, const uint64_t nnz[3], const Fr* coeffs_m, uint32_t n0, const Fr* dom_m, uint32_t m, uint32_t k,
                     long long window_chunks, uint8_t out[32], hipStream_t st) {
  if (!coeffs_m || !n0 || !dom_m || !m || !out) return DVP_EINVAL;
  DevBuf first, dout;
  DVP_TRY(first.alloc(8));
  DVP_TRY(dout.alloc(32));
  DVP_HIP(hipMemsetAsync(first.p, 0xff, 8, st));
  DVP_LAUNCH(k_ch_find_minus_one, dim3(cdiv(n0, CH_TPB)), dim3(CH_TPB), 0, st, coeffs_m, n0, first.as<unsigned long long>());
  DVP_HIP(hipGetLastError());
  unsigned long long h_first = 0;
  DVP_HIP(hipMemcpyAsync(&h_first, first.p, 8, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  const bool found = h_first < n0;
  const uint32_t i1 = found ? (uint32_t)h_first : n0;
  const uint64_t n1 = (uint64_t)n0 + (found ? 0 : 1);
  const uint64_t N = n1 + (uint64_t)m * (k > 1 ? k - 1 : 0);
  if (N > (1ull << 32)) return DVP_EINVAL;  // the reference's `as u32` would wrap
  const uint64_t row_dwords = nnz[0] + nnz[1] + nnz[2] + (uint64_t)k * m;
  const uint64_t coeff_bytes = 8 + 29 * N, coeff_dwords = (coeff_bytes + 3) / 4;
  const uint64_t total_bytes = 4 * row_dwords + coeff_bytes, total_dwords = row_dwords + coeff_dwords;
  const uint64_t nchunks = (total_bytes + 1023) / 1024;
  if (nchunks > (1ull << 32)) return DVP_EINVAL;  // 32-bit chunk counter
  // at most 2 GiB of window: a launch's grid stays far below 2^31 workgroups
  const uint64_t want_chunks = window_chunks > 0 ? std::min<uint64_t>((uint64_t)window_chunks, 1ull << 21) : (uint64_t)CH_WINDOW_CHUNKS_DEFAULT;
  const uint64_t win_chunks = std::min(want_chunks, nchunks);
  DevBuf win, cvs, tmp;
  DVP_TRY(win.alloc(win_chunks * 1024));
  if (nchunks > 1) {
    DVP_TRY(cvs.alloc(nchunks * 32));
    DVP_TRY(tmp.alloc(b3_reduce_tmp_bytes(nchunks)));
  }
  uint32_t* w = win.as<uint32_t>();
  for (uint64_t c0 = 0; c0 < nchunks; c0 += win_chunks) {
    const uint64_t dlo = c0 * 256, dhi = std::min((c0 + win_chunks) * 256, total_dwords);  // the window's dwords of the stream
    if (dlo < row_dwords) {
      const uint64_t b = std::min(dhi, row_dwords);
      const unsigned blocks = cdiv(b - dlo, CH_TPB);
      DVP_LAUNCH(k_ch_row_starts, dim3(cdiv(blocks, CH_TPB)), dim3(CH_TPB), 0, st, mats, m, k, dlo, b, w);
      DVP_LAUNCH(k_ch_rows, dim3(blocks), dim3(CH_TPB), 0, st, mats, m, k, i1, (uint32_t)n1 /* read for k > 1 only: n1 < N <= 2^32 then */, dlo, b, w);
      DVP_HIP(hipGetLastError());
    }
    if (dhi > row_dwords) {
      const uint64_t a = std::max(dlo, row_dwords), lo = a - row_dwords, hi = dhi - row_dwords;  // dwords of the coefficient part
      const uint64_t g0 = lo > 2 ? (lo - 2) / CH_GROUP_DWORDS : 0, g1 = hi > 2 ? (hi - 3) / CH_GROUP_DWORDS + 1 : 0;  // groups touched
      DVP_LAUNCH(k_ch_coeffs, dim3(g1 > g0 ? cdiv(g1 - g0, CH_TPB) : 1), dim3(CH_TPB), 0, st, coeffs_m, n0, n1, dom_m, m, k, N, g0, lo, hi,
                 w + (a - dlo));
      DVP_HIP(hipGetLastError());
    }
    const uint64_t len = std::min((c0 + win_chunks) * 1024, total_bytes) - c0 * 1024;
    if (nchunks == 1) DVP_TRY(b3_single_chunk_dev(win.as<uint8_t>(), len, dout.as<uint32_t>(), st));
    else DVP_TRY(b3_leaves_dev(win.as<uint8_t>(), len, c0, cvs.as<uint32_t>() + 8 * c0, st));
  }
  if (nchunks > 1) DVP_TRY(b3_reduce_dev(cvs.as<uint32_t>(), nchunks, tmp.as<uint32_t>(), dout.as<uint32_t>(), st));
  DVP_HIP(hipMemcpyAsync(out, dout.p, 32, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  return DVP_OK;
}

}  // namespace dvp
