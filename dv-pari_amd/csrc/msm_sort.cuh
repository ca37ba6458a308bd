// MSM sort: the one-shot counting sort (k_hist_local / k_hist_scan / k_scatter_local), FxBits and the two-level sort of the
// fixed-base mode (k_part_* by the high key bits, then k_hist_local2 / k_hist_scan2 / k_scatter_local2 within a partition), the staged
// scatters, and level 1 of the signed flavour fused with the recoder (k_part_hist_signed, k_part_scatter_signed).  Part of msm.hip's
// translation unit: msm.hip includes it, and its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include "common.h"
#include "msm_recode.cuh"
#include "msm_scan.cuh"

namespace dvp {

// ---- counting sort by (window, pattern) without global atomics ---------------------------------------
// Scattered global atomics run at ~16 G/s on MI355X (they execute at the memory side), which made
// histogram + scatter cost as much as a third of the MSM.  Instead each block owns a chunk of
// SORT_CHUNK scalars of ONE window and keeps the 2^c counters in LDS (c <= 15: 2^15 x 4 B = 128 KB of
// the CU's 160 KB):
//   k_hist_local  : LDS histogram (two u16 counters per word) -> hist[w][chunk][2^c] (u16)
//   k_hist_scan   : per (w, pattern): exclusive prefix over chunks -> chunk_off (u32) and cnt[w][pattern]
//   (scan of cnt -> off, as before)
//   k_scatter_local: LDS cursors = off + chunk_off, ds_add_rtn per digit -> items[]
constexpr uint32_t SORT_CHUNK = 32768;  // counts fit in u16
constexpr int SORT_TPB = 1024;

__global__ void __launch_bounds__(SORT_TPB)
k_hist_local(const uint16_t* __restrict__ digits, uint32_t n, int c, uint16_t* __restrict__ hist) {
  extern __shared__ uint32_t lds_cnt[];  // 2^(c-1) words
  const uint32_t chunk = blockIdx.x, w = blockIdx.y, nb = 1u << c, nchunks = gridDim.x;
  for (uint32_t k = threadIdx.x; k < (nb >> 1); k += SORT_TPB) lds_cnt[k] = 0;
  __syncthreads();
  uint32_t lo = chunk * SORT_CHUNK, hi = min(n, lo + SORT_CHUNK);
  const uint16_t* dg = digits + (size_t)w * n;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += SORT_TPB) {
    uint32_t d = dg[i];
    if (d) atomicAdd(&lds_cnt[d >> 1], 1u << (16 * (d & 1)));
  }
  __syncthreads();
  uint32_t* out = (uint32_t*)(hist + ((size_t)w * nchunks + chunk) * nb);
  for (uint32_t k = threadIdx.x; k < (nb >> 1); k += SORT_TPB) out[k] = lds_cnt[k];
}

__global__ void __launch_bounds__(256)
k_hist_scan(const uint16_t* __restrict__ hist, uint32_t nchunks, int c, int W, uint32_t* __restrict__ chunk_off,
            uint32_t* __restrict__ cnt) {
  uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t nb = 1u << c;
  if (key >= ((uint32_t)W << c)) return;
  uint32_t w = key >> c, b = key & (nb - 1);
  uint32_t run = 0;
  for (uint32_t ch = 0; ch < nchunks; ++ch) {
    size_t idx = ((size_t)w * nchunks + ch) * nb + b;
    uint32_t v = hist[idx];
    chunk_off[idx] = run;
    run += v;
  }
  cnt[key] = run;
}

__global__ void __launch_bounds__(SORT_TPB)
k_scatter_local(const uint16_t* __restrict__ digits, uint32_t n, int c, const uint32_t* __restrict__ off,
                const uint32_t* __restrict__ chunk_off, uint32_t* __restrict__ items) {
  extern __shared__ uint32_t lds_cur[];  // 2^c words
  const uint32_t chunk = blockIdx.x, w = blockIdx.y, nb = 1u << c, nchunks = gridDim.x;
  const uint32_t* co = chunk_off + ((size_t)w * nchunks + chunk) * nb;
  const uint32_t* of = off + ((size_t)w << c);
  for (uint32_t k = threadIdx.x; k < nb; k += SORT_TPB) lds_cur[k] = of[k] + co[k];
  __syncthreads();
  uint32_t lo = chunk * SORT_CHUNK, hi = min(n, lo + SORT_CHUNK);
  const uint16_t* dg = digits + (size_t)w * n;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += SORT_TPB) {
    uint32_t d = dg[i];
    if (d) items[atomicAdd(&lds_cur[d], 1u)] = i;
  }
}

// ---- two-level counting sort for the fixed-base mode (keys of up to 20 bits) ----------------------------
// Level 1 partitions the entries by the top `hi` key bits (LDS cursors per block, up to 2^10 partitions); level 2 is the
// LDS counting sort above applied inside each partition on the low `lo` <= 15 bits.  Both levels scatter single entries,
// so the more bins a level has the fewer entries of a chunk share a 32-byte sector: with 2^15 level-2 bins each 4-byte
// entry costs a whole sector (1.3 GB of HBM writes for 160 MB of entries), with 2^9 level-1 bins the two level-1
// streams thrash the L2 instead.  The split is a per-context knob (MsmFixedCtx::hi_bits); staging each chunk in LDS
// and writing whole runs would remove the trade-off and is the known next step for this stage.
// An entry is the pair (table row, scalar i) (FXW_* entry words); its id e = row * n_total + i0 + i indexes the
// pre-rotated base table.
constexpr int FX_C_MAX = 20, FX_NP_MAX = 1 << (FX_C_MAX / 2);  // c = lo + hi bits, chosen per context
constexpr uint32_t FX_CHUNK = 8192;  // entries per block at both levels: the staged scatters keep a whole chunk in LDS (78 KB / 61 KB: two blocks per CU, so one block's copy-out overlaps the other's staging; 16384 = one block per CU: sort 1.27 -> 1.17 ms per proof; 4096: 1.54)
struct FxBits {
  int lo, hi;  // low bits sorted in LDS, high bits partitioned first
  __host__ __device__ uint32_t np() const { return 1u << hi; }
};

__global__ void __launch_bounds__(SORT_TPB)
k_part_hist(const uint32_t* __restrict__ digits, size_t total, FxBits fb, uint32_t* __restrict__ phist) {
  __shared__ uint32_t h[FX_NP_MAX];
  const uint32_t FX_NP = fb.np();
  const int FX_LO = fb.lo;
  for (uint32_t k = threadIdx.x; k < FX_NP; k += SORT_TPB) h[k] = 0;
  __syncthreads();
  size_t lo = (size_t)blockIdx.x * FX_CHUNK, hi = min(total, lo + FX_CHUNK);
  for (size_t e = lo + threadIdx.x; e < hi; e += SORT_TPB) {
    uint32_t d = digits[e];
    if (d) atomicAdd(&h[fxw_key(d) >> FX_LO], 1u);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < FX_NP; k += SORT_TPB) phist[(size_t)blockIdx.x * FX_NP + k] = h[k];
}
// exclusive prefix of every partition's counts over the level-1 blocks, in two coalesced launches (round 5; the first version gave a
// block a partition and walked phist down a column -- a 128-byte line per 4-byte count, twice: 52 us per MSM).
// pass A: a block takes FX_SCAN_CB consecutive level-1 blocks; a thread owns partition columns (consecutive threads, consecutive
// partitions: whole lines in, whole lines out) and leaves the prefix WITHIN the chunk in pbase and the chunk's totals in ctot[part][chunk];
// pass B: a wave per partition scans its chunk totals in place (exclusive) and leaves the partition's count.
// A level-1 block b then starts its run of partition p at pstart[p] + ctot[p][b / FX_SCAN_CB] + pbase[b][p].
constexpr uint32_t FX_SCAN_CB = 32;
__global__ void __launch_bounds__(256)
k_part_scan_chunks(const uint32_t* __restrict__ phist, uint32_t nblk, FxBits fb, uint32_t* __restrict__ pbase, uint32_t* __restrict__ ctot, uint32_t nch) {
  const uint32_t FX_NP = fb.np();
  const uint32_t ch = blockIdx.x, b0 = ch * FX_SCAN_CB, b1 = min(nblk, b0 + FX_SCAN_CB);
  for (uint32_t part = threadIdx.x; part < FX_NP; part += 256) {
    uint32_t run = 0;
#pragma unroll 8
    for (uint32_t b = b0; b < b1; ++b) {
      const uint32_t v = phist[(size_t)b * FX_NP + part];
      pbase[(size_t)b * FX_NP + part] = run;
      run += v;
    }
    ctot[(size_t)part * nch + ch] = run;
  }
}
__global__ void __launch_bounds__(256)
k_part_scan_totals(uint32_t* __restrict__ ctot, uint32_t nch, FxBits fb, uint32_t* __restrict__ pcount) {
  const uint32_t part = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (part >= fb.np()) return;  // whole waves
  uint32_t* row = ctot + (size_t)part * nch;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nch; base += 64) {
    const uint32_t idx = base + lane;
    const uint32_t v = idx < nch ? row[idx] : 0;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o);
      if ((int)lane >= o) x += y;
    }
    if (idx < nch) row[idx] = carry + x - v;
    carry += __shfl(x, 63);
  }
  if (lane == 0) pcount[part] = carry;
}
// partition starts and the global level-2 chunk index of each partition (one block of FX_NP_MAX threads)
__global__ void __launch_bounds__(FX_NP_MAX)
k_part_starts(const uint32_t* __restrict__ pcount, FxBits fb, uint32_t* __restrict__ pstart, uint32_t* __restrict__ cstart) {
  __shared__ uint32_t sp[FX_NP_MAX], sc[FX_NP_MAX];
  const uint32_t FX_NP = fb.np(), t = threadIdx.x;
  uint32_t pc = t < FX_NP ? pcount[t] : 0, cc = (pc + FX_CHUNK - 1) / FX_CHUNK;
  sp[t] = pc;
  sc[t] = cc;
  __syncthreads();
  for (uint32_t o = 1; o < FX_NP_MAX; o <<= 1) {
    uint32_t a = t >= o ? sp[t - o] : 0, b = t >= o ? sc[t - o] : 0;
    __syncthreads();
    sp[t] += a;
    sc[t] += b;
    __syncthreads();
  }
  if (t < FX_NP) {
    pstart[t] = sp[t] - pc;
    cstart[t] = sc[t] - cc;
  }
  if (t == FX_NP - 1) {
    pstart[FX_NP] = sp[t];
    cstart[FX_NP] = sc[t];
  }
}
__global__ void __launch_bounds__(SORT_TPB)
k_part_scatter(const uint32_t* __restrict__ digits, size_t total, uint32_t n, uint32_t n_total, uint32_t i0, FxBits fb,
               const uint32_t* __restrict__ pbase, const uint32_t* __restrict__ cbase, uint32_t nch, const uint32_t* __restrict__ pstart,
               uint16_t* __restrict__ plo, uint32_t* __restrict__ pid) {
  __shared__ uint32_t cur[FX_NP_MAX];
  const uint32_t FX_NP = fb.np();
  const int FX_LO = fb.lo;
  const uint32_t ch = blockIdx.x / FX_SCAN_CB;
  for (uint32_t k = threadIdx.x; k < FX_NP; k += SORT_TPB) cur[k] = pstart[k] + cbase[(size_t)k * nch + ch] + pbase[(size_t)blockIdx.x * FX_NP + k];
  __syncthreads();
  size_t lo = (size_t)blockIdx.x * FX_CHUNK, hi = min(total, lo + FX_CHUNK);
  for (size_t e = lo + threadIdx.x; e < hi; e += SORT_TPB) {
    uint32_t d = digits[e];
    if (!d) continue;
    const uint32_t i = (uint32_t)(e % n), key = fxw_key(d);
    uint32_t pos = atomicAdd(&cur[key >> FX_LO], 1u);
    plo[pos] = (uint16_t)(key & ((1u << FX_LO) - 1));
    pid[pos] = (fxw_row(d) * n_total + i0 + i) | ((d & FXW_NEG) ? ITEM_NEG : 0u);
  }
}
// the partition whose chunk range [cstart[k], cstart[k+1]) holds chunk g (empty partitions share their start with the
// next one, so take the LAST k with cstart[k] <= g)
__device__ __forceinline__ uint32_t fx_chunk_partition(const uint32_t* __restrict__ cstart, uint32_t FX_NP, uint32_t g) {
  uint32_t lo = 0, hi = FX_NP;  // invariant: cstart[lo] <= g, and cstart[hi] > g or hi == FX_NP
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (cstart[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}
// level 2, per global chunk g (partition hi, local chunk g - cstart[hi])
__global__ void __launch_bounds__(SORT_TPB)
k_hist_local2(const uint16_t* __restrict__ plo, const uint32_t* __restrict__ pstart, const uint32_t* __restrict__ cstart, FxBits fb,
              uint16_t* __restrict__ hist) {
  extern __shared__ uint32_t lds_cnt[];  // 2^(lo-1) words (two u16 counters per word)
  const uint32_t FX_NP = fb.np();
  const uint32_t g = blockIdx.x, nb = 1u << fb.lo;
  if (g >= cstart[FX_NP]) return;
  for (uint32_t k = threadIdx.x; k < (nb >> 1); k += SORT_TPB) lds_cnt[k] = 0;
  __syncthreads();
  uint32_t hi = fx_chunk_partition(cstart, FX_NP, g);
  uint32_t lo_e = pstart[hi] + (g - cstart[hi]) * FX_CHUNK, hi_e = min(pstart[hi + 1], lo_e + FX_CHUNK);
  // Round 5: eight entries per load (16 bytes) over the 16-byte-aligned body of the chunk, single entries for its ragged ends -- one
  // load per thread and chunk instead of eight 2-byte ones (100 MB at 1.3 TB/s: the kernel waited for its loads)
  auto count = [&](uint32_t d) { atomicAdd(&lds_cnt[d >> 1], 1u << (16 * (d & 1))); };
  const uint32_t body_lo = min(hi_e, (lo_e + 7u) & ~7u), body_hi = max(body_lo, hi_e & ~7u);
  for (uint32_t j = lo_e + threadIdx.x; j < body_lo; j += SORT_TPB) count(plo[j]);
  for (uint32_t j = body_lo + 8u * threadIdx.x; j < body_hi; j += 8u * SORT_TPB) {
    const uint4 v = *(const uint4*)(plo + j);
    count(v.x & 0xffffu); count(v.x >> 16); count(v.y & 0xffffu); count(v.y >> 16);
    count(v.z & 0xffffu); count(v.z >> 16); count(v.w & 0xffffu); count(v.w >> 16);
  }
  for (uint32_t j = body_hi + threadIdx.x; j < hi_e; j += SORT_TPB) count(plo[j]);
  __syncthreads();
  uint32_t* out = (uint32_t*)(hist + (size_t)g * nb);
  for (uint32_t k = threadIdx.x; k < (nb >> 1); k += SORT_TPB) out[k] = lds_cnt[k];
}
__global__ void __launch_bounds__(256)
k_hist_scan2(const uint16_t* __restrict__ hist, const uint32_t* __restrict__ cstart, FxBits fb, uint32_t* __restrict__ chunk_off,
             uint32_t* __restrict__ cnt) {
  uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;  // < 2^c
  if (key >= (1u << (fb.lo + fb.hi))) return;
  const uint32_t nb = 1u << fb.lo;
  uint32_t hi = key >> fb.lo, b = key & (nb - 1);
  uint32_t run = 0;
  for (uint32_t g = cstart[hi]; g < cstart[hi + 1]; ++g) {
    size_t idx = (size_t)g * nb + b;
    uint32_t v = hist[idx];
    chunk_off[idx] = run;
    run += v;
  }
  cnt[key] = run;
}
__global__ void __launch_bounds__(SORT_TPB)
k_scatter_local2(const uint16_t* __restrict__ plo, const uint32_t* __restrict__ pid, const uint32_t* __restrict__ pstart,
                 const uint32_t* __restrict__ cstart, FxBits fb, const uint32_t* __restrict__ off, const uint32_t* __restrict__ chunk_off,
                 uint32_t* __restrict__ items) {
  extern __shared__ uint32_t lds_cur[];  // 2^lo words
  const uint32_t FX_NP = fb.np();
  const int FX_LO = fb.lo;
  const uint32_t g = blockIdx.x, nb = 1u << FX_LO;
  if (g >= cstart[FX_NP]) return;
  uint32_t hi = fx_chunk_partition(cstart, FX_NP, g);
  const uint32_t* co = chunk_off + (size_t)g * nb;
  const uint32_t* of = off + ((size_t)hi << FX_LO);
  for (uint32_t k = threadIdx.x; k < nb; k += SORT_TPB) lds_cur[k] = of[k] + co[k];
  __syncthreads();
  uint32_t lo_e = pstart[hi] + (g - cstart[hi]) * FX_CHUNK, hi_e = min(pstart[hi + 1], lo_e + FX_CHUNK);
  for (uint32_t j = lo_e + threadIdx.x; j < hi_e; j += SORT_TPB) items[atomicAdd(&lds_cur[plo[j]], 1u)] = pid[j];
}

// ---- staged scatters (used when a level has <= SORT_TPB bins) ---------------------------------------------------------
// A block first places its chunk into LDS grouped by bin (LDS cursors start at the exclusive scan of the chunk's own
// histogram), then copies the staged chunk out in order: consecutive lanes hold consecutive entries of one bin, whose
// destinations are consecutive, so every bin leaves as one coalesced run instead of as single-entry sector writes.
__device__ __forceinline__ uint32_t block_scan_tpb(uint32_t v, uint32_t* sh, uint32_t* total) {
  return block_scan_waves<SORT_TPB / 64>(v, total, sh);
}
constexpr unsigned FX_STAGE1_LDS = (2 * FX_NP_MAX + SORT_TPB + 2 * FX_CHUNK) * 4;
constexpr unsigned FX_STAGE2_LDS = (2 * FX_NP_MAX + SORT_TPB + FX_CHUNK) * 4 + FX_CHUNK * 2;

__global__ void __launch_bounds__(SORT_TPB)
k_part_scatter_staged(const uint32_t* __restrict__ digits, size_t total, uint32_t n, uint32_t n_total, uint32_t i0, FxBits fb,
                      const uint32_t* __restrict__ phist, const uint32_t* __restrict__ pbase, const uint32_t* __restrict__ cbase, uint32_t nch,
                      const uint32_t* __restrict__ pstart, uint16_t* __restrict__ plo, uint32_t* __restrict__ pid) {
  extern __shared__ uint32_t lds_st[];
  uint32_t* cur = lds_st;             // [FX_NP_MAX]
  uint32_t* gdst = cur + FX_NP_MAX;   // [FX_NP_MAX] destination of staged position 0 of the bin
  uint32_t* sh = gdst + FX_NP_MAX;    // [SORT_TPB]
  uint32_t* st_d = sh + SORT_TPB;     // [FX_CHUNK]
  uint32_t* st_id = st_d + FX_CHUNK;  // [FX_CHUNK]
  const uint32_t FX_NP = fb.np(), t = threadIdx.x;
  const int FX_LO = fb.lo;
  const size_t hb = (size_t)blockIdx.x * FX_NP;
  uint32_t h = t < FX_NP ? phist[hb + t] : 0, tot;
  uint32_t ex = block_scan_tpb(h, sh, &tot);
  if (t < FX_NP) {
    cur[t] = ex;
    gdst[t] = pstart[t] + cbase[(size_t)t * nch + blockIdx.x / FX_SCAN_CB] + pbase[hb + t] - ex;
  }
  __syncthreads();
  const size_t lo = (size_t)blockIdx.x * FX_CHUNK, hi = min(total, lo + FX_CHUNK);
  const uint32_t w0 = (uint32_t)(lo / n);
  for (size_t e = lo + t; e < hi; e += SORT_TPB) {
    uint32_t d = digits[e];
    if (!d) continue;
    size_t i = e - (size_t)w0 * n;  // e mod n: a chunk spans few slots
    while (i >= n) i -= n;
    const uint32_t key = fxw_key(d);
    uint32_t pos = atomicAdd(&cur[key >> FX_LO], 1u);
    st_d[pos] = key;
    st_id[pos] = (fxw_row(d) * n_total + i0 + (uint32_t)i) | ((d & FXW_NEG) ? ITEM_NEG : 0u);
  }
  __syncthreads();
  const uint32_t mask = (1u << FX_LO) - 1;
  for (uint32_t pos = t; pos < tot; pos += SORT_TPB) {
    uint32_t d = st_d[pos], dst = gdst[d >> FX_LO] + pos;
    plo[dst] = (uint16_t)(d & mask);
    pid[dst] = st_id[pos];
  }
}

// ---- level 1 of the signed flavour straight from the scalars (round 4) -------------------------------------------------------
// k_recode_signed wrote W entry words per scalar (4 B each) that k_part_hist and the level-1 scatter then read back: 12 B of HBM
// traffic per entry for a few shifts' worth of work.  Here a block owns S = FX_CHUNK / W consecutive SCALARS (all their windows:
// <= FX_CHUNK entries) and both level-1 kernels recompute the words from the 32-byte scalar.  Which entries share a chunk changes,
// the sorted order inside a bucket with it -- the bucket's SUM does not.
__global__ void __launch_bounds__(SORT_TPB)
k_part_hist_signed(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t n, int c, int W, int n_narrow, uint32_t S,
                   FxBits fb, uint32_t* __restrict__ phist, unsigned long long* __restrict__ err) {
  __shared__ uint32_t h[FX_NP_MAX];
  const uint32_t FX_NP = fb.np();
  const int FX_LO = fb.lo;
  for (uint32_t k = threadIdx.x; k < FX_NP; k += SORT_TPB) h[k] = 0;
  __syncthreads();
  const uint32_t lo = blockIdx.x * S, hi = min(n, lo + S);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += SORT_TPB) {
    uint32_t s[9];
    if (!fx_load_scalar(scalars, inf, i, s, err, true)) continue;
    const uint32_t carry = fx_recode_signed_each(s, c, W, n_narrow, [&](int, uint32_t word) {
      if (word) atomicAdd(&h[fxw_key(word) >> FX_LO], 1u);
    });
    if (carry) atomicMin(err, (unsigned long long)i | (1ull << 62));  // cannot happen
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < FX_NP; k += SORT_TPB) phist[(size_t)blockIdx.x * FX_NP + k] = h[k];
}
template <bool STAGED>
__global__ void __launch_bounds__(SORT_TPB)
k_part_scatter_signed(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t n, int c, int W, int n_narrow, uint32_t S,
                      uint32_t n_total, uint32_t i0, FxBits fb, const uint32_t* __restrict__ phist, const uint32_t* __restrict__ pbase,
                      const uint32_t* __restrict__ cbase, uint32_t nch, const uint32_t* __restrict__ pstart, uint16_t* __restrict__ plo,
                      uint32_t* __restrict__ pid) {
  extern __shared__ uint32_t lds_st[];
  uint32_t* cur = lds_st;             // [FX_NP_MAX]
  uint32_t* gdst = cur + FX_NP_MAX;   // [FX_NP_MAX] STAGED: destination of staged position 0 of the bin
  uint32_t* sh = gdst + FX_NP_MAX;    // [SORT_TPB]
  uint32_t* st_d = sh + SORT_TPB;     // [FX_CHUNK]
  uint32_t* st_id = st_d + FX_CHUNK;  // [FX_CHUNK]
  const uint32_t FX_NP = fb.np(), t = threadIdx.x;
  const int FX_LO = fb.lo;
  const size_t hb = (size_t)blockIdx.x * FX_NP;
  const uint32_t mask = (1u << FX_LO) - 1;
  uint32_t tot = 0;
  const uint32_t ch = blockIdx.x / FX_SCAN_CB;
  if (STAGED) {
    uint32_t h = t < FX_NP ? phist[hb + t] : 0;
    uint32_t ex = block_scan_tpb(h, sh, &tot);
    if (t < FX_NP) {
      cur[t] = ex;
      gdst[t] = pstart[t] + cbase[(size_t)t * nch + ch] + pbase[hb + t] - ex;
    }
  } else {
    for (uint32_t k = t; k < FX_NP; k += SORT_TPB) cur[k] = pstart[k] + cbase[(size_t)k * nch + ch] + pbase[hb + k];
  }
  __syncthreads();
  const uint32_t lo = blockIdx.x * S, hi = min(n, lo + S);
  for (uint32_t i = lo + t; i < hi; i += SORT_TPB) {
    uint32_t s[9];
    if (!fx_load_scalar(scalars, inf, i, s, nullptr, false)) continue;
    fx_recode_signed_each(s, c, W, n_narrow, [&](int w, uint32_t word) {
      if (!word) return;
      const uint32_t key = fxw_key(word);
      const uint32_t id = ((uint32_t)w * n_total + i0 + i) | ((word & FXW_NEG) ? ITEM_NEG : 0u);
      const uint32_t pos = atomicAdd(&cur[key >> FX_LO], 1u);
      if (STAGED) {
        st_d[pos] = key;
        st_id[pos] = id;
      } else {
        plo[pos] = (uint16_t)(key & mask);
        pid[pos] = id;
      }
    });
  }
  if (!STAGED) return;
  __syncthreads();
  for (uint32_t pos = t; pos < tot; pos += SORT_TPB) {
    uint32_t d = st_d[pos], dst = gdst[d >> FX_LO] + pos;
    plo[dst] = (uint16_t)(d & mask);
    pid[dst] = st_id[pos];
  }
}

__global__ void __launch_bounds__(SORT_TPB)
k_scatter_local2_staged(const uint16_t* __restrict__ plo, const uint32_t* __restrict__ pid, const uint32_t* __restrict__ pstart,
                        const uint32_t* __restrict__ cstart, FxBits fb, const uint32_t* __restrict__ off,
                        const uint32_t* __restrict__ chunk_off, const uint16_t* __restrict__ hist, uint32_t* __restrict__ items) {
  extern __shared__ uint32_t lds_st[];
  uint32_t* cur = lds_st;
  uint32_t* gdst = cur + FX_NP_MAX;
  uint32_t* sh = gdst + FX_NP_MAX;
  uint32_t* st_id = sh + SORT_TPB;                 // [FX_CHUNK]
  uint16_t* st_b = (uint16_t*)(st_id + FX_CHUNK);  // [FX_CHUNK]
  const uint32_t FX_NP = fb.np(), t = threadIdx.x;
  const int FX_LO = fb.lo;
  const uint32_t g = blockIdx.x, nb = 1u << FX_LO;  // nb <= SORT_TPB
  if (g >= cstart[FX_NP]) return;
  const uint32_t hi = fx_chunk_partition(cstart, FX_NP, g);
  uint32_t h = t < nb ? hist[(size_t)g * nb + t] : 0, tot;
  uint32_t ex = block_scan_tpb(h, sh, &tot);
  if (t < nb) {
    cur[t] = ex;
    gdst[t] = off[((size_t)hi << FX_LO) + t] + chunk_off[(size_t)g * nb + t] - ex;
  }
  __syncthreads();
  const uint32_t lo_e = pstart[hi] + (g - cstart[hi]) * FX_CHUNK, hi_e = min(pstart[hi + 1], lo_e + FX_CHUNK);
  auto place = [&](uint32_t b, uint32_t id) {
    const uint32_t pos = atomicAdd(&cur[b], 1u);
    st_id[pos] = id;
    st_b[pos] = (uint16_t)b;
  };
  // Round 5: eight entries per thread and trip over the aligned body of the chunk (one 16-byte load of keys, two of ids) instead of
  // eight trips of a 2-byte and a 4-byte load; which entry of a bin lands where inside the bin changes, the bin's content does not
  const uint32_t body_lo = min(hi_e, (lo_e + 7u) & ~7u), body_hi = max(body_lo, hi_e & ~7u);
  for (uint32_t j = lo_e + t; j < body_lo; j += SORT_TPB) place(plo[j], pid[j]);
  for (uint32_t j = body_lo + 8u * t; j < body_hi; j += 8u * SORT_TPB) {
    const uint4 k = *(const uint4*)(plo + j), a = *(const uint4*)(pid + j), c = *(const uint4*)(pid + j + 4);
    place(k.x & 0xffffu, a.x); place(k.x >> 16, a.y); place(k.y & 0xffffu, a.z); place(k.y >> 16, a.w);
    place(k.z & 0xffffu, c.x); place(k.z >> 16, c.y); place(k.w & 0xffffu, c.z); place(k.w >> 16, c.w);
  }
  for (uint32_t j = body_hi + t; j < hi_e; j += SORT_TPB) place(plo[j], pid[j]);
  __syncthreads();
  for (uint32_t pos = t; pos < tot; pos += SORT_TPB) items[gdst[st_b[pos]] + pos] = st_id[pos];
}

}  // namespace dvp
