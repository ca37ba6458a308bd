// MSM batched-affine pair rounds: k_post_sort, the all-rounds bookkeeping (k_mscan_*, DescPlan, k_round_desc*), the slot
// planning (AFF_BMAX, aff_slots_per_thread), the shared-inversion exchange (AFF_SHARE_INV, aff_x_put / aff_x_get), WaveTrace, AffSlot,
// k_affine_round and the gather kernels that turn its output into the dense bucket array.  Part of msm.hip's translation unit:
// msm.hip includes it, and its kernels are launched and counted as msm.hip's (see the map at the top of msm.hip).
#pragma once
#include "common.h"
#include "k233.cuh"
#include "msm_scan.cuh"
#include "msm_reduce.cuh"

namespace dvp {

// ---- batched-affine pair rounds --------------------------------------------------------------------
// One round halves every bucket: output slot (key, j) = in[2j] + in[2j+1] (or in[2j] alone when the
// count is odd), all in AFFINE coordinates.  An affine addition needs one field inversion; a thread owns
// B output slots and shares ONE inversion among them (Montgomery's trick): per addition 3 products for
// the trick + 2 products + 1 squaring for the chord/tangent formulas, against 8M + 5S for a mixed
// projective addition.  Prefix products are parked in HBM ([slot-in-thread][thread] layout, so the
// traffic is coalesced).  (0,0) -- not a curve point -- marks infinity.
//
// A round after the first is two launches.  k_round_desc resolves every output slot to its two input points once --
// (a, b) = indices into `pts`, b = NONE for the odd leftover of a bucket -- with a group of lanes per bucket, so the
// hot kernel does not search the bucket offsets (18 dependent L2 round trips per slot in the first version); the first
// round reads the sorted item list itself as its descriptors (below).  k_affine_round then runs two software-pipelined passes over its slots: the descriptor of
// slot k+2 and the operands of slot k+1 are in flight while slot k multiplies, so the random 64-byte gathers of the
// bases (HBM misses in the first round: the pre-rotated table is 5 GB) are off the critical path.
constexpr uint32_t AFF_NONE = 0xffffffffu;
// slot descriptor of the rounds after the first: the slot adds points i and i + 1 of the previous round's output (DESC_PAIR set) or
// passes point i on (a bucket's odd leftover); i < 2^31.  The first round reads the sorted item list as (a, b) pairs instead; the
// dense order of the all-rounds bookkeeping (k_round_desc_all) adds a second word, the index the slot's result goes to.
constexpr uint32_t DESC_PAIR = 0x80000000u;

// Both sorts lay every bucket out from an EVEN position of the item list (scan of the counts rounded up to
// even); an odd bucket's spare slot gets AFF_NONE.  The list read as uint2 pairs is then exactly the descriptor array of
// the first pair round -- (a, b) table indices, b = NONE for the odd leftover -- so that round needs no descriptor
// kernel and no scan: its output offsets are the item offsets halved (k_post_sort, or the all-rounds scan).
// the three per-key passes between the sort and the first pair round of an MSM whose bookkeeping is not done by the all-rounds scan (small
// one-shot MSMs) as ONE launch (round 6): the NONE behind every odd bucket, the first round's counts and offsets, the largest bucket
__global__ void __launch_bounds__(256)
k_post_sort(uint32_t* __restrict__ items, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off /* nkeys + 1, even */, uint32_t nkeys,
            uint32_t* __restrict__ ocnt, uint32_t* __restrict__ ooff /* nkeys + 1 */, uint32_t* __restrict__ d_max) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t m = 0;
  if (k <= nkeys) {
    const uint32_t o = off[k];
    ooff[k] = o >> 1;
    if (k < nkeys) {
      const uint32_t c = cnt[k];
      if (c & 1) items[o + c] = AFF_NONE;
      ocnt[k] = (c + 1) >> 1;
      m = c;
    }
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(d_max, m);
}

// ---- the bookkeeping of ALL pair rounds at once (round 4) --------------------------------------------------------------------
// Round r's input counts are c_r = ceil(c_{r-1} / 2) of the sort's counts c_0, its offsets their exclusive scan: R scans that depend
// on nothing but c_0, so one three-launch scan carries all of them (a column of R running sums per key) where the rounds used to
// pay three launches each.  rp: (c_r, o_r) for r = 1 .. R, each nkeys + 1 words (o_r[nkeys] = total), at rp + 2 (r - 1) (nkeys + 1).
__global__ void __launch_bounds__(SCAN_TPB) k_mscan_local(const uint32_t* __restrict__ cnt0, uint32_t m, int R, uint32_t* __restrict__ rp,
                                                          uint32_t* __restrict__ bs /* [R][nb], then nb block maxima of cnt0 */) {
  __shared__ uint32_t sh[SCAN_TPB];
  const uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_EPT;
  uint32_t v[SCAN_EPT];
#pragma unroll
  for (int k = 0; k < SCAN_EPT; ++k) v[k] = (base + k < m) ? cnt0[base + k] : 0;
  {  // the largest count of this block (k_mscan_bsums reduces the blocks' maxima: no atomics -- 2 048 waves on one word cost 20 us)
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < SCAN_EPT; ++k) mx = max(mx, v[k]);
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < SCAN_TPB / 64; ++w) mx = max(mx, sh[w]);
      bs[(size_t)R * gridDim.x + blockIdx.x] = mx;
    }
    __syncthreads();
  }
  for (int r = 1; r <= R; ++r) {
    uint32_t* c = rp + (size_t)(2 * (r - 1)) * ((size_t)m + 1);
    uint32_t* o = c + ((size_t)m + 1);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_EPT; ++k) {
      v[k] = (v[k] + 1u) >> 1;
      s += v[k];
    }
    uint32_t tot;
    uint32_t ex = block_exclusive_scan(s, &tot, sh);
#pragma unroll
    for (int k = 0; k < SCAN_EPT; ++k) {
      if (base + k < m) {
        c[base + k] = v[k];
        o[base + k] = ex;
      }
      ex += v[k];
    }
    if (threadIdx.x == 0) bs[(size_t)(r - 1) * gridDim.x + blockIdx.x] = tot;
  }
}
__global__ void __launch_bounds__(SCAN_TPB) k_mscan_bsums(uint32_t* __restrict__ bs, uint32_t nb, uint32_t m, uint32_t* __restrict__ rp,
                                                          uint32_t* __restrict__ off0 /* item offsets (or nullptr): off0[m] = the padded total */,
                                                          uint32_t* __restrict__ dmax /* the largest count (or nullptr) */) {
  __shared__ uint32_t sh[SCAN_TPB];
  const int r = blockIdx.x + 1;
  uint32_t* row = bs + (size_t)(r - 1) * nb;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += SCAN_TPB) {
    uint32_t idx = base + threadIdx.x;
    uint32_t v = idx < nb ? row[idx] : 0;
    uint32_t tot;
    uint32_t ex = block_exclusive_scan(v, &tot, sh);
    if (idx < nb) row[idx] = ex + carry;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    rp[(size_t)(2 * (r - 1) + 1) * ((size_t)m + 1) + m] = carry;  // o_r[nkeys]
    if (r == 1 && off0) off0[m] = 2u * carry;
  }
  if (r == 1 && dmax) {  // the largest bucket, from the block maxima k_mscan_local left behind the R rows of block sums
    const uint32_t* bm = bs + (size_t)gridDim.x * nb;
    uint32_t mx = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += SCAN_TPB) mx = max(mx, bm[i]);
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < SCAN_TPB / 64; ++w) mx = max(mx, sh[w]);
      *dmax = mx;
    }
  }
}
// Round 5: the last launch of the scan also finishes what the SORT needs from the counts, which used to be six launches of their own
// (a second three-launch scan, k_pad_odd_buckets, a memset and k_max_u32): the item offsets off0 -- the scan of the counts rounded up
// to even is exactly twice o_1, the scan of ceil(c_0 / 2) --, the NONE in the spare slot of every odd bucket (a position the
// scatter never writes, so it may be filled before the scatter runs); the largest bucket comes out of k_mscan_local's block maxima
// (k_mscan_bsums).
__global__ void __launch_bounds__(SCAN_TPB) k_mscan_add(uint32_t* __restrict__ rp, const uint32_t* __restrict__ bs, uint32_t m, int R,
                                                        const uint32_t* __restrict__ cnt0, uint32_t* __restrict__ off0, uint32_t* __restrict__ items) {
  const uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_EPT;
  for (int r = 1; r <= R; ++r) {
    uint32_t* o = rp + (size_t)(2 * (r - 1) + 1) * ((size_t)m + 1);
    const uint32_t add = bs[(size_t)(r - 1) * gridDim.x + blockIdx.x];
    if (r == 1 && off0) {
#pragma unroll
      for (int k = 0; k < SCAN_EPT; ++k)
        if (base + k < m) {
          const uint32_t v = o[base + k] + add, c = cnt0[base + k];
          o[base + k] = v;
          off0[base + k] = 2u * v;
          if (c & 1u) items[2u * v + c] = AFF_NONE;
        }
      continue;
    }
#pragma unroll
    for (int k = 0; k < SCAN_EPT; ++k)
      if (base + k < m) o[base + k] += add;
  }
}
// slot descriptors of rounds 1 .. R - 1 in one launch: LPK lanes per bucket walk its outputs round by round
// (round r pairs the outputs of round r - 1: inputs at o_r[key] + 2 j, + 1; outputs at o_(r+1)[key] + j)
struct DescPlan {
  unsigned long long at[40];  // round r's descriptors start at desc + at[r]
};
// DENSE (Tune::msm_round_dense): a round's additions fill slots [0, A_r) and its odd leftovers [A_r, total_r), two words per slot
// {input index | DESC_PAIR, output index} -- the rows of k_affine_round that hold leftovers alone then copy and multiply nothing.
// The dense positions need no scan of their own: exclusive scans are linear, so the pairs of a key start at o_r - o_(r+1) (the scan
// of floor(c_r / 2)), its leftover sits at 2 o_(r+1) - o_r (the scan of c_r & 1) behind the A_r = o_r[nkeys] - o_(r+1)[nkeys] pairs.
template <int LPK, bool DENSE>
__global__ void __launch_bounds__(1024)
k_round_desc_all(const uint32_t* __restrict__ rp, uint32_t nkeys, int R, DescPlan plan, uint32_t* __restrict__ desc) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t key = gid / LPK, lane = gid % LPK;
  if (key >= nkeys) return;
  const size_t stride = (size_t)nkeys + 1;
  // the counts and offsets of up to eight rounds are asked for at once and the descriptors written afterwards: a round's three loads
  // used to sit in front of its stores, round after round
  for (int r0 = 1; r0 < R; r0 += 8) {
    uint32_t cr[8], o[8], oo[8], A[8];  // A: the round's additions (DENSE only)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = r0 + q;
      if (r < R) {
        const uint32_t* c = rp + (size_t)(2 * (r - 1)) * stride;
        cr[q] = c[key];
        o[q] = c[stride + key];
        oo[q] = c[3 * stride + key];
        A[q] = DENSE ? c[stride + nkeys] - c[3 * stride + nkeys] : 0u;
      } else {
        cr[q] = 0; o[q] = 0; oo[q] = 0; A[q] = 0;
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = r0 + q;
      if (r >= R) break;
      const uint32_t nout = (cr[q] + 1) >> 1;
      uint32_t* d = desc + plan.at[r];
      if (DENSE) {
        const uint32_t npair = cr[q] >> 1, a = o[q] - oo[q];
        uint2* d2 = (uint2*)d;
        for (uint32_t j = lane; j < npair; j += LPK) d2[a + j] = make_uint2((o[q] + 2 * j) | DESC_PAIR, oo[q] + j);
        if ((cr[q] & 1u) && lane == npair % LPK) d2[A[q] + (2 * oo[q] - o[q])] = make_uint2(o[q] + cr[q] - 1, oo[q] + npair);
        continue;
      }
      for (uint32_t j = lane; j < nout; j += LPK) d[oo[q] + j] = (o[q] + 2 * j) | ((2 * j + 1 < cr[q]) ? DESC_PAIR : 0u);
    }
  }
}

template <int LPK>
__global__ void __launch_bounds__(256)
k_round_desc(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, const uint32_t* __restrict__ ooff /* scan of ceil(cnt/2), nkeys+1 */,
             uint32_t nkeys, uint32_t* __restrict__ desc) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t key = gid / LPK, lane = gid % LPK;
  if (key >= nkeys) return;
  const uint32_t c = cnt[key], o = off[key], oo = ooff[key], nout = (c + 1) >> 1;
  for (uint32_t j = lane; j < nout; j += LPK) desc[oo + j] = (o + 2 * j) | ((2 * j + 1 < c) ? DESC_PAIR : 0u);
}

// Thread t of T = ceil(total / B) owns output slots s = k*T + t, k < B (lane-consecutive slots: coalesced
// descriptors, outputs, prefix products and -- after the first round -- inputs).
// B (slots per thread = additions per shared inversion) is chosen ON THE DEVICE from the round's size so that the
// grid is a whole number of chip-fulls: all threads of a round take the same time, so with a fixed B the last
// partial wave of blocks ran on a mostly idle chip (2.2 chip-fulls cost 3: the first version averaged 64 % of its
// 12 waves per CU).  With `cap` = resident threads of the chip, R = ceil(total / (cap * AFF_BMAX)) chip-fulls of
// B = ceil(total / (cap * R)) slots each: B is 33..136 in the big rounds (25..48 through round 4) and shrinks to 1..8 in the last ones, where a
// round is pure latency and short threads are what is wanted.
// Round 4 (tools/wave_trace.py, profiles/r04_wave_trace_*): the instruction arbiter of a SIMD serves its OLDEST wave first.  Of
// three resident waves with identical work the first finished after 1.32 ms, the second after 1.55, the third after 1.93; every
// later chip-full inherited the stagger and the end of each launch drained through SIMDs with two and then one wave left --
// that, not gaps between workgroups (a freed slot was refilled in 10-15 us) nor the launch ramp, was the whole of the missing
// resident-wave fraction (0.83-0.88).  Rotating the user priority with the slot index hands the issue slots round: the three
// waves of a SIMD now finish within 2 % of each other, a one-chip-full round ends 10 % sooner (1.58 -> 1.41 ms).
#ifndef AFF_PRIO
#define AFF_PRIO 1
#endif
// Pass 1 multiplies the slope's NUMERATOR into the prefix as well -- run * num and run * den are one gf_mul2 against one table of
// `run` --, and pass 2 gets lam = (run num) * inv and the stripped inverse den * inv from one gf_mul2 against `inv`: three table
// builds per addition.  (The compile-time switches back to the arithmetic of rounds 1-6 -- AFF_NUM1 = 0: four tables, AFF_XY = 0: y
// fetched a slot after x -- went when the rare cases left the slot loops: DESIGN.md and docs/HISTORY.md keep their measurements.)
//
// RARE slots.  A pair slot whose addition is not the chord formula -- an operand is infinity (x == 0), or x1 == x2: a doubling or
// P - P -- does not occur in real use (table points of distinct bases are distinct, and infinity only comes out of P - P), so the
// straight-line code of the slot loops only DETECTS it (tools/round_isa_budget.py: what a slot executes beside its products) and
// everything else sits behind wave-uniform branches no wave of a real input takes.  There pass 1 gives a doubling the tangent's
// den = x, num = y (lambda = x + y / x) and any other rare slot den = 1, num = 0, and says which it was in the free bits of word 7 of
// the prefix it parks (a field element's word 7 is below 2^9); pass 2 finds the flag in the entry it loads anyway: a doubling goes
// through the same products with its denominator put right before and lambda after, the others are finished on the spot without
// arithmetic -- p or q passed on, or infinity for P - P.  The arithmetic is the one these cases always had, so the bytes are too.
constexpr uint32_t AFF_W7_MASK = 0x1ffu, AFF_W7_DBL = 1u << 30, AFF_W7_SKIP = 1u << 31;
__device__ __forceinline__ uint32_t aff_or8(const Gf& a) {
  return ((a.w[0] | a.w[1] | a.w[2]) | (a.w[3] | a.w[4])) | ((a.w[5] | a.w[6]) | a.w[7]);
}
__device__ __forceinline__ void aff_set_prio(uint32_t v) {
  switch (v % 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    default: __builtin_amdgcn_s_setprio(2); break;
  }
}
// default (Tune::msm_aff_bmax).  48 through round 4 (swept flat 32 .. 128 then); re-swept at the end of round 5, with the product 15 %
// shorter: 48 / 64 / 68 / 72 / 136 / 255 -> 19.14 / 19.15 / 18.99 / 18.99 / 18.98 / 19.00 ms per 2^20 proof and 66.8 / - / - / 66.0 / 64.7-65.0 /
// 65.0 ms at 2^22 -- from 68 the first round of the commitment MSM and the second of the K MSM are ONE chip-full of 65 slots per thread
// instead of two of 33, from 130 the K MSM's first round is one of 129: fewer drains and a smaller inversion share
constexpr uint32_t AFF_BMAX = 136;
// bmax_bmin: bits 0..7 = most slots per thread, bits 8..15 = fewest (a small round then runs on fewer threads, each sharing its
// inversion among more additions: Tune::msm_aff_bmin)
__device__ __forceinline__ uint32_t aff_slots_per_thread(uint32_t total, uint32_t cap, uint32_t bmax_bmin) {
  const uint32_t bmax = bmax_bmin & 0xffu, bmin = (bmax_bmin >> 8) & 0xffu;  // (bit 16: AFF_SHARE_INV, below)
  const uint32_t units = (total + cap - 1) / cap;  // slots per resident thread if the round were one chip-full
  const uint32_t R = (units + bmax - 1) / bmax;
  const uint32_t B = R ? (units + R - 1) / R : 1;
  return B < bmin ? bmin : B;
}
// ---- one inversion per WORKGROUP instead of one per wave (bit 16 of the kernel's bmax argument; Tune::msm_aff_share_inv) ----------
// A SIMD pays an inversion per wave-instruction, not per lane: ~14 k of them per wave and launch, however few additions share them.
// With the bit set the waves of a workgroup of 128 or 256 threads post their running products to an exchange area behind the table
// regions, lane-wise products over the waves go up a tree (two waves form the pair products, one wave -- the INVERTING wave -- their
// product), that wave alone runs the chain on the workgroup's product and sends the two half inverses back down, and every wave
// recovers its own 1 / run with one more product: 3 + 2 + 4 wave-products and one chain per workgroup instead of four chains.  The
// field inverse is exact, so the result is the same bits.  Everything between the barriers is workgroup-uniform control flow.
// Exchange slots hold one Gf per lane of a wave as two rows of 64 x 16 B (conflict-free 128-bit accesses): slots 0 .. W-1 = the
// waves' products; W = 4: slots 4, 5 = the pair products run0 run1 and run2 run3, then 1 / (run0 run1) and 1 / (run2 run3) in their
// place; W = 2: slot 2 = the inverse of run0 run1.
constexpr uint32_t AFF_SHARE_INV = 1u << 16;
constexpr uint32_t AFF_X_SLOT_BYTES = 2048;
constexpr uint32_t aff_exchange_bytes(uint32_t waves) { return waves == 4 ? 6 * AFF_X_SLOT_BYTES : waves == 2 ? 3 * AFF_X_SLOT_BYTES : 0; }
// which wave inverts: co-resident workgroups should pick waves on DIFFERENT SIMDs, or their chains queue up on one.  The rule takes
// consecutive waves for consecutive dispatch sweeps over the chip (one workgroup per CU: AFF_INV_SPREAD of them on an MI355X).  Any
// value is correct; it only places the chains.  Measured (tools/wave_trace.py, "shared_inversion"): a wave's number does NOT name its
// SIMD -- every wave number turns up on all four -- so the rule spreads the chains no better than chance: of the inverting waves that
// overlap in time on one CU 27-33 % share a SIMD (docs/HISTORY.md; electing by the SIMD ids the waves could post is not built).
constexpr uint32_t AFF_INV_SPREAD = 256;
__device__ __forceinline__ void aff_x_put(uint32_t lane_addr, uint32_t slot, const Gf& v) {
  const uint32_t a = lane_addr + slot * AFF_X_SLOT_BYTES;
  gf_lds_st(a, (gf_u32x4){v.w[0], v.w[1], v.w[2], v.w[3]});
  gf_lds_st(a + 1024, (gf_u32x4){v.w[4], v.w[5], v.w[6], v.w[7]});
}
__device__ __forceinline__ Gf aff_x_get(uint32_t lane_addr, uint32_t slot) {
  const uint32_t a = lane_addr + slot * AFF_X_SLOT_BYTES;
  const gf_u32x4 lo = gf_lds_ld(a), hi = gf_lds_ld(a + 1024);
  Gf r;
  r.w[0] = lo.x; r.w[1] = lo.y; r.w[2] = lo.z; r.w[3] = lo.w;
  r.w[4] = hi.x; r.w[5] = hi.y; r.w[6] = hi.z; r.w[7] = hi.w;
  return r;
}
// FIRST only names the launch: k_affine_round<true> is the first pair round of an MSM (random gathers out of the
// pre-rotated table -- the dominant kernel bench.py's roofline block is about), <false> the later rounds (coalesced
// inputs); the code is the same, the two symbols keep them apart in rocprofv3's per-kernel statistics.
// Wave-level trace of a pair round (diagnostics only: dvp_debug_wave_trace, tools/wave_trace.py).  TRACE instantiations stamp
// s_memrealtime (100 MHz, constant) and s_memtime (shader clock) at the start of a wave, after its first pass, after the shared
// inversion and at its end, with the hardware slot the wave ran in (HW_ID: wave, SIMD, CU, SH, SE; XCC_ID): one 64-byte record
// per wave behind a 64-byte header whose first word is the record counter.  The production launches use TRACE = false.
struct WaveTrace {
  unsigned long long* buf;  // [0] = records written, records from word 8
  uint32_t cap, tag;
};
// a slot as the kernel sees it: the points it adds (b = NONE: a is passed on; a = NONE: no such slot) and, on the DENSE path, the
// index its result goes to (elsewhere that is the slot's own number)
struct AffSlot {
  uint32_t a, b, o;
};
// a whole point.  Signed-digit flavours (first round only: the operands are table entries named by sorted items): bit 31 of an item
// says "subtract"; -(x, y) = (x, x + y), applied as the point is loaded (one and-xor per word under the sign's mask, no branch)
template <bool FIRST>
__device__ __forceinline__ void aff_ld_point(const Aff* __restrict__ pts, uint32_t sm, uint32_t v, Gf& x, Gf& y) {
  const Aff* p = pts + (v & ~sm);
  x = p->x;
  y = p->y;
  if (FIRST) {
    const uint32_t neg = 0u - (uint32_t)((v & sm) != 0u);
#pragma unroll
    for (int i = 0; i < 8; ++i) y.w[i] = gf_andxor(neg, x.w[i], y.w[i]);
  }
}
// Slot k of a thread is slot sk = k nthr + tid of the round: the loops carry sk along (one addition per slot) for the descriptors, the
// prefix entries and the outputs.  lim = the round's slots for a thread below nthr, 0 beyond (there sk would name another thread's
// slot).  The load is unconditional from a clamped index and the VALUE is selected (round 6: returning `none` from an early exit made
// hipcc select between two ADDRESSES -- &desc[sk] and a private copy of `none`: 16 B of scratch per lane and, worse, a FLAT load per
// descriptor, which counts on lgkmcnt beside the multiplier's LDS reads).
template <bool FIRST, bool DENSE>
__device__ __forceinline__ AffSlot aff_ld_desc(const uint2* __restrict__ desc, int k, int B, uint32_t sk, uint32_t lim) {
  const bool ok = k >= 0 && k < B && sk < lim;
  const uint32_t at = ok ? sk : 0u;
  // first round: the item pair; later rounds: one word per slot, or two on the DENSE path
  const uint2 d = (FIRST || DENSE) ? desc[at] : make_uint2(((const uint32_t*)desc)[at], 0u);
  if (FIRST) return AffSlot{ok ? d.x : AFF_NONE, ok ? d.y : AFF_NONE, 0u};
  const uint32_t a = d.x & ~DESC_PAIR;
  return AffSlot{ok ? a : AFF_NONE, (ok && (d.x & DESC_PAIR)) ? a + 1 : AFF_NONE, d.y};
}
// DENSE (later rounds whose bookkeeping k_round_desc_all<.., true> did): two-word descriptors, additions first, leftovers last
template <bool FIRST, bool TRACE = false, bool DENSE = false>
__global__ void __launch_bounds__(EC_TPB) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_affine_round(const Aff* __restrict__ pts, const uint2* __restrict__ desc, const uint32_t* __restrict__ total_ptr /* ooff[nkeys] */,
               uint32_t cap, uint32_t bmax, GfSqrTables T, Gf* __restrict__ prefix, Aff* __restrict__ out, uint32_t sign_mask, WaveTrace wt) {
  extern __shared__ char lds_raw[];
  unsigned long long tr_t0 = 0, tr_c0 = 0, tr_t1 = 0, tr_t2 = 0;
  uint32_t tr_inverted = 0;  // bit 1: the launch shares its inversions, bit 0: this wave ran the chain
  if (TRACE) { tr_t0 = wall_clock64(); tr_c0 = clock64(); }
  GfLdsK L = gf_ldsk_init(lds_raw);
#if AFF_PRIO
  const uint32_t wslot = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | 4);  // HW_ID.wave_id: this wave's slot in its SIMD
#endif
  const uint32_t sm = FIRST ? sign_mask : 0u;
  auto ldx = [&](uint32_t v) -> Gf { return pts[v & ~sm].x; };
  auto ldp = [&](uint32_t v, Gf& x, Gf& y) { aff_ld_point<FIRST>(pts, sm, v, x, y); };
  const uint32_t total = *total_ptr;
  const int B = (int)aff_slots_per_thread(total, cap, bmax);
  const uint32_t nthr = (total + B - 1) / B;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  // shared inversion: barriers ahead, so only a workgroup WHOLLY beyond nthr leaves; in the last live one the threads at or beyond nthr
  // stay with run = 1 and no slot (ld_desc), and a wave of such threads alone skips both passes
  const bool share = (bmax & AFF_SHARE_INV) != 0 && blockDim.x > 64;
  if (share ? blockIdx.x * blockDim.x >= nthr : tid >= nthr) return;
  const bool wave_live = __builtin_amdgcn_readfirstlane(tid & ~63u) < nthr;
  const uint32_t lim = tid < nthr ? total : 0u;
  auto ld_desc = [&](int k, uint32_t sk) -> AffSlot { return aff_ld_desc<FIRST, DENSE>(desc, k, B, sk, lim); };
  const Gf one = gf_one();
  // pass 1: the running product of the denominators, and every slot's numerator times the product before it (x and y of a point
  // share a 64-byte half line: no request more than for x alone).  A slot's operands are consumed -- den = x1 + x2, num = y1 + y2, the
  // three zero tests -- before the next slot's are asked for INTO THE SAME REGISTERS: nothing is handed down the pipeline by copying.
  // A lane whose slot is no pair loads point 0 twice, so its den comes out 0 and becomes the one it multiplies with by an OR.
  // A wave whose lanes all hold leftovers -- the top rows of a DENSE round -- skips loads and product.
  Gf run = one;
  if (wave_live) {
    uint32_t sk = tid, sp = tid;  // the slot whose descriptor is asked for next, and slot k itself
    AffSlot d0 = ld_desc(0, sk);
    sk += nthr;
    AffSlot d1 = ld_desc(1, sk);
    sk += nthr;
    Gf xa, ya, xb, yb;
    {
      const bool p = d0.b != AFF_NONE;
      ldp(p ? d0.a : 0u, xa, ya);
      ldp(p ? d0.b : 0u, xb, yb);
    }
#pragma unroll 1
    for (int k = 0; k < B; ++k) {
#if AFF_PRIO
      aff_set_prio(wslot + (uint32_t)k);
#endif
      const bool pair = d0.b != AFF_NONE;
      Gf den = gf_add(xa, xb), num = gf_add(ya, yb);
      const bool ainf = aff_or8(xa) == 0u, binf = aff_or8(xb) == 0u;
      const bool rare = pair & (ainf | binf | (aff_or8(den) == 0u));
      bool dbl = false;
      den.w[0] |= pair ? 0u : 1u;
      if (__any(rare)) {
        if (rare) {
          dbl = !ainf & !binf & (aff_or8(num) == 0u);  // x1 == x2 and y1 == y2
          den = dbl ? xa : one;
          num = dbl ? ya : gf_zero();
        }
      }
      const AffSlot d2 = ld_desc(k + 2, sk);
      sk += nthr;
      {
        const bool p = d1.b != AFF_NONE;
        if (!DENSE || __any(p)) {
          ldp(p ? d1.a : 0u, xa, ya);
          ldp(p ? d1.b : 0u, xb, yb);
        }
      }
      if (!DENSE || __any(pair)) {
        Gf np, nrun;
        gf_mul2(num, den, run, L, np, nrun);
        if (__any(rare)) {
          if (rare) np.w[7] |= dbl ? AFF_W7_DBL : AFF_W7_SKIP;
        }
        if (pair) prefix[sp] = np;
        run = nrun;
      }
      sp += nthr;
      d0 = d1;
      d1 = d2;
    }
  }
  if (TRACE) tr_t1 = wall_clock64();
  // the inversion: of this wave's product, or (share) by one wave of the workgroup's.  ONE call site of the chain for both forms
  // (a second chain for the inverting wave with unfenced table passes, gf_sqr_tab_wide or two words of lookups in flight, cost every
  // instantiation 616-660 B of scratch per lane: the scheduler pulls the loads across the products around them)
  const uint32_t W = blockDim.x >> 6, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t xa = L.lane_base + (W - w) * GF_LDSK_BYTES_PER_WAVE;  // this lane's entry of exchange slot 0, behind the W table regions
  const uint32_t inverting = (blockIdx.x / AFF_INV_SPREAD) & (W - 1);
  Gf inv = run;
  if (share) {
    if (TRACE) tr_inverted = w == inverting ? 3u : 2u;
    aff_x_put(xa, w, run);
    __syncthreads();
    if (W == 4) {
      if ((w & 1u) == 0) aff_x_put(xa, 4 + (w >> 1), gf_mul(run, aff_x_get(xa, w + 1), L));
      __syncthreads();
    }
    if (w == inverting) {
      // (its neighbours wait at the barrier and issue nothing: ahead of the other workgroups' passes on this SIMD)
      __builtin_amdgcn_s_setprio(3);
      inv = gf_mul(aff_x_get(xa, W == 4 ? 4 : 0), aff_x_get(xa, W == 4 ? 5 : 1), L);
    }
  }
  if (!share || w == inverting) inv = gf_inv_fast(inv, T, L);
  if (share) {
    if (w == inverting) {
      if (W == 4) {
        // (the pair products are read back, not kept: nothing but the chain's own value is live across it)
        Gf ia, ib;
        gf_mul2(aff_x_get(xa, 5), aff_x_get(xa, 4), inv, L, ia, ib);  // 1 / (run0 run1) and 1 / (run2 run3)
        aff_x_put(xa, 4, ia);
        aff_x_put(xa, 5, ib);
      } else {
        aff_x_put(xa, 2, inv);
      }
      __builtin_amdgcn_s_setprio(0);  // (pass 2 resumes the rotation at its first slot)
    }
    __syncthreads();
    inv = gf_mul(aff_x_get(xa, W == 4 ? 4 + (w >> 1) : 2), aff_x_get(xa, w ^ 1u), L);
  }
  if (TRACE) tr_t2 = wall_clock64();
  // pass 2 (backwards): recover each inverse and finish the addition.  The next slot's WHOLE point p and its prefix entry are asked
  // for a slot ahead (x and y of a point share a 128-byte line, and a y fetched one slot after its x found the line evicted from the
  // L2 again: 6.3 line requests per addition, 4.3 so); of q only x is wanted -- the numerator is in the prefix already --, and it is
  // consumed into dd = x1 + x2 before the next one lands in its registers.  A pair runs straight-line code: one gf_mul2, the
  // squaring, one gf_mul, two stores; a leftover is copied.
  if (wave_live) {
    uint32_t sp = (uint32_t)(B - 1) * nthr + tid, sk = sp;
    auto ld_slot = [&](const AffSlot& e, uint32_t s, Gf& x1, Gf& y1, Gf& x2, Gf& pre) {
      const bool pair = e.b != AFF_NONE;
      ldp(e.a != AFF_NONE ? e.a : 0u, x1, y1);
      x2 = ldx(pair ? e.b : 0u);
      pre = prefix[pair ? s : 0u];
    };
    AffSlot e0 = ld_desc(B - 1, sk);
    sk -= nthr;
    AffSlot e1 = ld_desc(B - 2, sk);
    sk -= nthr;
    Gf px, py, qx, pre;
    ld_slot(e0, sp, px, py, qx, pre);
#pragma unroll 1
    for (int k = B - 1; k >= 0; --k) {
#if AFF_PRIO
      aff_set_prio(wslot + (uint32_t)k);
#endif
      const bool pair = e0.b != AFF_NONE, flagged = pair & (pre.w[7] > AFF_W7_MASK);
      const uint32_t sidx = DENSE ? e0.o : sp;
      Gf dd = gf_add(px, qx);
      bool add = pair, dbl = false;
      if (__any(flagged)) {
        if (flagged) {
          dbl = (pre.w[7] & AFF_W7_DBL) != 0u;
          if (dbl) {  // the tangent: the denominator pass 1 used is x (dd is 0 here)
            pre.w[7] &= AFF_W7_MASK;
            dd = px;
          } else {  // p == infinity: q; q == infinity: p; else p == -q: infinity
            add = false;
            const bool pinf = aff_or8(px) == 0u, qinf = aff_or8(qx) == 0u;
            Gf qy, unused;
            ldp(e0.b, unused, qy);
            out[sidx].x = pinf ? qx : qinf ? px : gf_zero();
            out[sidx].y = pinf ? qy : qinf ? py : gf_zero();
          }
        }
      }
      const AffSlot e2 = ld_desc(k - 2, sk);
      sk -= nthr;
      Gf npx, npy, npre;
      ld_slot(e1, sp - nthr, npx, npy, qx, npre);
      if (add) {
        Gf lam, inv_next;
        gf_mul2(pre, dd, inv, L, lam, inv_next);  // num/den (pre = num times the product before this slot), and the running inverse stripped of this slot's factor
        inv = inv_next;
        if (__any(dbl)) {
          if (dbl) {  // lambda = x + y / x; x3 = lambda^2 + lambda (curve a = 0)
            lam = gf_add(lam, px);
            dd = gf_zero();
          }
        }
        const Gf ox = gf_add(gf_add(gf_sqr(lam), lam), dd);
        // y3 = lam (x1 + x3) + x3 + y1   (the same expression covers the doubling)
        const Gf oy = gf_add(gf_add(gf_mul(gf_add(px, ox), lam, L), ox), py);
        out[sidx].x = ox;
        out[sidx].y = oy;
      } else if (e0.a != AFF_NONE && !pair) {  // a bucket's odd leftover: p is passed on
        out[sidx].x = px;
        out[sidx].y = py;
      }
      sp -= nthr;
      e0 = e1;
      e1 = e2;
      px = npx;
      py = npy;
      pre = npre;
    }
  }
#if AFF_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif
  if (TRACE) {
    const unsigned long long t3 = wall_clock64(), c3 = clock64();
    if ((threadIdx.x & 63u) == 0) {
      const unsigned long long i = atomicAdd(wt.buf, 1ull);
      if (i < wt.cap) {
        unsigned long long* r = wt.buf + 8 + 8 * i;
        r[0] = tr_t0; r[1] = tr_t1; r[2] = tr_t2; r[3] = t3;
        r[4] = tr_c0; r[5] = c3;
        r[6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);  // HW_ID | XCC_ID
        r[7] = (unsigned long long)blockIdx.x | ((unsigned long long)wt.tag << 32) | ((unsigned long long)(uint32_t)B << 48) | ((unsigned long long)(threadIdx.x >> 6) << 56) |
               ((unsigned long long)tr_inverted << 60);
      }
    }
  }
}

// dense bucket array from the last affine round: A[key] = (x, y, 1) or infinity
__global__ void __launch_bounds__(256)
k_bucket_gather_aff(const Aff* __restrict__ in, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                    uint32_t nkeys, Ld* __restrict__ A) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  Ld r = ld_infinity();
  if (cnt[k]) {
    Aff p = in[off[k]];
    if (!gf_is_zero(p.x)) r = ld_from_aff(p);  // x == 0 marks infinity (no point of E[r] has x = 0)
  }
  A[k] = r;
}
// same, straight from the sorted items (keys that never had more than one point)
__global__ void __launch_bounds__(256)
k_bucket_gather_items(const Aff* __restrict__ bases, const uint32_t* __restrict__ items, const uint32_t* __restrict__ cnt,
                      const uint32_t* __restrict__ off, uint32_t nkeys, Ld* __restrict__ A, uint32_t sign_mask) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  Ld r = ld_infinity();
  if (cnt[k]) {
    const uint32_t v = items[off[k]];
    Aff q = bases[v & ~sign_mask];
    if (v & sign_mask) q.y = gf_add(q.y, q.x);
    r = ld_from_aff(q);
  }
  A[k] = r;
}

// dense bucket array: A[key] = the single remaining item of key, or infinity
__global__ void __launch_bounds__(256)
k_bucket_gather(const Ld* __restrict__ in, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                uint32_t nkeys, Ld* __restrict__ A) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  A[k] = cnt[k] ? in[off[k]] : ld_infinity();
}

}  // namespace dvp
