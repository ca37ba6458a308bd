// Explain an unsatisfied witness: which rows fail a*b = C w (all of them counted, the first ones listed with a, b, c', i), which entries
// are not below p, and which wires occur in failing rows only.  Over the prover's resident matrices, without SRS, between proofs.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
//
//   k_wc_reduce      the assignment (any 256-bit values, little-endian limbs or the file's big-endian bytes) -> SA, reduced mod p
//                    (fr_reduce_le_words); counts and locates the entries that were not below p, looks at the constant wire
//   k_wc_rows        k_r1cs_eval's predicate per row, on SA: one bit per row (a wave's ballot), one count per workgroup
//   -- the host reads the 48-byte block here: a satisfying witness is done --
//   k_wc_scan        workgroup counts -> offsets (one workgroup, in place)
//   k_wc_list_rows   a failing row's rank = its workgroup's offset + the bits in front of it; ranks below the cap evaluate the row again
//                    and write {row, a, b, c', i}
//   k_wc_terms       per term of A, B, C: the wire's counter of terms in failing rows, or its mark of a term in a satisfied row
//   k_wc_flag_wires  suspect = counter > 0 and no mark: bits and workgroup counts again, then k_wc_scan and
//   k_wc_list_wires  the ranked write of {wire, n_terms}
// Both listings are compactions by rank: what a truncated list holds, and in which order, does not depend on scheduling.
#pragma once
#include "prove_state.cuh"

namespace dvp {

// the check's result block on the device
struct WcBlock {
  unsigned long long first[2];  // [0] unsatisfied row, [1] entry not below p; ~0 = none
  unsigned long long count[3];  // unsatisfied rows, entries not below p, suspect wires
  unsigned long long const_one; // the constant wire reduces to 1
};
struct WcRow {  // dvp_unsat_row
  unsigned long long row;
  Fr a, b, c, i;
};
static_assert(sizeof(WcRow) == sizeof(dvp_unsat_row) && sizeof(WcRow) == 136, "the record a host reads");

// First half of an ordered compaction over a grid of 256-thread workgroups: flag f of thread i becomes bit (i & 63) of bits[i >> 6],
// the workgroup's count goes to cnt[blockIdx.x], the total and the first flagged index to *total / *first.  Every thread of the
// workgroup calls it (threads behind the end with f = false).  Returns the workgroup's count.
__device__ __forceinline__ uint32_t wc_flag(bool f, size_t i, unsigned long long* __restrict__ bits, uint32_t* __restrict__ cnt,
                                            unsigned long long* __restrict__ total, unsigned long long* __restrict__ first) {
  __shared__ uint32_t per_wave[4];
  const unsigned long long mask = __ballot(f);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    bits[(size_t)blockIdx.x * 4 + wave] = mask;
    per_wave[wave] = (uint32_t)__popcll(mask);
    if (mask) atomicMin(first, (unsigned long long)(i + (size_t)__ffsll((long long)mask) - 1));
  }
  __syncthreads();
  const uint32_t n = per_wave[0] + per_wave[1] + per_wave[2] + per_wave[3];
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = n;
    if (n) atomicAdd(total, (unsigned long long)n);
  }
  return n;
}
// Second half: is i flagged, and how many flagged indices lie in front of it (off = the scanned workgroup counts)
__device__ __forceinline__ bool wc_rank(const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ off, size_t i, uint32_t* rank) {
  const size_t word = i >> 6;
  const unsigned long long mask = bits[word];
  const uint32_t lane = (uint32_t)(i & 63);
  if (!((mask >> lane) & 1)) return false;
  uint32_t r = off[i >> 8] + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
  for (size_t wd = word & ~(size_t)3; wd < word; ++wd) r += (uint32_t)__popcll(bits[wd]);
  *rank = r;
  return true;
}

template <bool BE>
__global__ void __launch_bounds__(256)
k_wc_reduce(const uint32_t* __restrict__ in, uint32_t n, Fr* __restrict__ out, WcBlock* __restrict__ blk) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool big = false;
  if (i < n) {
    Fr x, r;
#pragma unroll
    for (int k = 0; k < 8; ++k) x.v[k] = BE ? __builtin_bswap32(in[8 * (size_t)i + 7 - k]) : in[8 * (size_t)i + k];
    big = !fr_is_canonical(x);
    fr_reduce_le_words(x.v, r.v);
    out[i] = r;
    if (i == 0) blk->const_one = fr_eq(r, fr_one_canon()) ? 1ull : 0ull;
  }
  const unsigned long long mask = __ballot(big);
  if ((threadIdx.x & 63) == 0 && mask) {
    atomicAdd(&blk->count[1], (unsigned long long)__popcll(mask));
    atomicMin(&blk->first[1], (unsigned long long)i + (unsigned long long)__ffsll((long long)mask) - 1);
  }
}

// a, b, C w of row i as k_r1cs_eval forms them, and its predicate
__device__ __forceinline__ bool wc_row_fails(const Csr& A, const Csr& B, const Csr& C, const Fr* __restrict__ coeffs_m, const Fr* __restrict__ w,
                                             uint32_t i, Fr& a, Fr& b, Fr& cw) {
  a = csr_row(A, i, coeffs_m, w);
  b = csr_row(B, i, coeffs_m, w);
  cw = csr_row(C, i, coeffs_m, w);
  return !fr_eq(fr_mul(fr_to_mont(a), b), cw);  // a*b == c' + i  <=>  a*b == C w
}

__global__ void __launch_bounds__(256)
k_wc_rows(Csr A, Csr B, Csr C, const Fr* __restrict__ coeffs_m, const Fr* __restrict__ w, uint32_t m, unsigned long long* __restrict__ bits,
          uint32_t* __restrict__ cnt, WcBlock* __restrict__ blk) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  Fr a, b, cw;
  const bool bad = i < m && wc_row_fails(A, B, C, coeffs_m, w, i, a, b, cw);
  (void)wc_flag(bad, i, bits, cnt, &blk->count[0], &blk->first[0]);
}

// exclusive scan of n counts, in place, by ONE workgroup of 256 threads
__global__ void __launch_bounds__(256) k_wc_scan(uint32_t* __restrict__ cnt, uint32_t n) {
  __shared__ uint32_t sh[256];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n ? cnt[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      const uint32_t t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < n) cnt[i] = carry + sh[threadIdx.x] - v;
    carry += sh[255];
    __syncthreads();
  }
}

// the first `cap` failing rows, in row order: {row, a, b, c' = C w - i(d), i(d) = sum_j pub_j d^j}, canonical
__global__ void __launch_bounds__(256)
k_wc_list_rows(Csr A, Csr B, Csr C, const Fr* __restrict__ coeffs_m, const Fr* __restrict__ w, const Fr* __restrict__ dom_m, uint32_t npub,
               uint32_t m, const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ off, uint32_t cap, WcRow* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t rank;
  if (i >= m || !wc_rank(bits, off, i, &rank) || rank >= cap) return;
  Fr a, b, cw;
  (void)wc_row_fails(A, B, C, coeffs_m, w, i, a, b, cw);
  const Fr d = dom_m[i];
  Fr iv = fr_zero();
  for (int j = (int)npub - 1; j >= 0; --j) iv = fr_add(fr_mul(d, iv), w[1 + j]);  // Horner, canonical
  WcRow r;
  r.row = i;
  r.a = a;
  r.b = b;
  r.c = fr_sub(cw, iv);
  r.i = iv;
  out[rank] = r;
}

// per term of the dump's matrices (no Vandermonde fold): failing row -> the wire's counter, satisfied row -> the wire's mark
__device__ __forceinline__ void wc_row_terms(const Csr& M, uint32_t row, bool fails, uint32_t* __restrict__ in_bad, uint32_t* __restrict__ in_good) {
  if (row >= M.n_rows) return;
  for (uint32_t k = M.row_ptr[row]; k < M.row_ptr[row + 1]; ++k) {
    const uint32_t wi = M.wire[k];
    if (fails) atomicAdd(&in_bad[wi], 1u);
    else if (__atomic_load_n(&in_good[wi], __ATOMIC_RELAXED) == 0) atomicOr(&in_good[wi], 1u);  // the constant wire is in most rows: mark once
  }
}
__global__ void __launch_bounds__(256)
k_wc_terms(Csr A, Csr B, Csr C, uint32_t n_rows, const unsigned long long* __restrict__ bits, uint32_t* __restrict__ in_bad,
           uint32_t* __restrict__ in_good) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const bool fails = (bits[i >> 6] >> (i & 63)) & 1;
  wc_row_terms(A, i, fails, in_bad, in_good);
  wc_row_terms(B, i, fails, in_bad, in_good);
  wc_row_terms(C, i, fails, in_bad, in_good);
}

__global__ void __launch_bounds__(256)
k_wc_flag_wires(const uint32_t* __restrict__ in_bad, const uint32_t* __restrict__ in_good, uint32_t n_wires, unsigned long long* __restrict__ bits,
                uint32_t* __restrict__ cnt, WcBlock* __restrict__ blk, unsigned long long* __restrict__ first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool suspect = i < n_wires && in_bad[i] != 0 && in_good[i] == 0;
  (void)wc_flag(suspect, i, bits, cnt, &blk->count[2], first);
}
__global__ void __launch_bounds__(256)
k_wc_list_wires(const uint32_t* __restrict__ in_bad, uint32_t n_wires, const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ off,
                uint32_t cap, dvp_suspect_wire* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t rank;
  if (i >= n_wires || !wc_rank(bits, off, i, &rank) || rank >= cap) return;
  out[rank] = dvp_suspect_wire{i, in_bad[i]};
}

}  // namespace dvp

// scratch of one check: allocated on the stream, and freed on it when the scope ends, whichever way
struct WcScratch {
  void* p = nullptr;
  hipStream_t st = nullptr;
  WcScratch() = default;
  WcScratch(const WcScratch&) = delete;
  WcScratch& operator=(const WcScratch&) = delete;
  ~WcScratch() {
    if (p) (void)hipFreeAsync(p, st);
  }
  int alloc(size_t bytes, hipStream_t s) {
    st = s;
    DVP_HIP(hipMallocAsync(&p, bytes ? bytes : 16, s));
    return DVP_OK;
  }
};

// what every flavour asks before any device work
static int wc_args(const dvp_prover* p, const dvp_unsat_row* rows, size_t rows_cap, const dvp_suspect_wire* wires, size_t wires_cap,
                   const dvp_witness_report* rep) {
  if (!p || !rep || (rows_cap && !rows) || (wires_cap && !wires)) return DVP_EINVAL;
  if (!(p->coeffs_m && p->mat[0].row_ptr && p->mat[1].row_ptr && p->mat[2].row_ptr)) return DVP_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (p->mat[k].nnz && p->mat[k].max_coeff_id >= p->n_coeffs) return DVP_EINVAL;
  return DVP_OK;
}

// d_in: n_wires elements of 32 bytes on the device, little-endian limbs or (be) the witness file's big-endian bytes.  One wait for a
// satisfying witness; an unsatisfied one is listed behind that look at the count and waits a second time.
static int check_witness_impl(dvp_prover* p, const void* d_in, bool be, dvp_unsat_row* rows, size_t rows_cap, dvp_suspect_wire* wires,
                              size_t wires_cap, dvp_witness_report* rep, hipStream_t st) {
  DVP_TRY(wc_args(p, rows, rows_cap, wires, wires_cap, rep));
  if (!d_in) return DVP_EINVAL;
  memset(rep, 0, sizeof(*rep));
  rep->first_unsat = rep->first_noncanonical = -1;
  const uint32_t m = p->m, nw = p->n_wires;
  const uint32_t nb = cdiv(m, PT), nbw = cdiv(nw, PT);
  Csr A{p->mat[0].row_ptr, p->mat[0].wire, p->mat[0].coeff, p->mat[0].n_rows};
  Csr B{p->mat[1].row_ptr, p->mat[1].wire, p->mat[1].coeff, p->mat[1].n_rows};
  Csr C{p->mat[2].row_ptr, p->mat[2].wire, p->mat[2].coeff, p->mat[2].n_rows};
  WcScratch s1;
  Carver c1;
  const size_t o_blk = c1.take(sizeof(WcBlock)), o_bits = c1.take((size_t)nb * 4 * 8), o_cnt = c1.take((size_t)nb * 4);
  DVP_TRY(s1.alloc(c1.o, st));
  WcBlock* blk = (WcBlock*)((char*)s1.p + o_blk);
  unsigned long long* bits = (unsigned long long*)((char*)s1.p + o_bits);
  uint32_t* cnt = (uint32_t*)((char*)s1.p + o_cnt);
  DVP_HIP(hipMemsetAsync(blk->first, 0xff, sizeof(blk->first), st));
  DVP_HIP(hipMemsetAsync(blk->count, 0, sizeof(WcBlock) - sizeof(blk->first), st));
  Fr* w = p->SA;  // the reduced assignment, where a proof keeps its own: the next begin overwrites it
  p->trace_ok = false;  // SA no longer holds the last proof's assignment: that proof has no trace any more
  if (be) DVP_LAUNCH(k_wc_reduce<true>, dim3(nbw), dim3(PT), 0, st, (const uint32_t*)d_in, nw, w, blk);
  else DVP_LAUNCH(k_wc_reduce<false>, dim3(nbw), dim3(PT), 0, st, (const uint32_t*)d_in, nw, w, blk);
  DVP_LAUNCH(k_wc_rows, dim3(nb), dim3(PT), 0, st, A, B, C, p->coeffs_m, w, m, bits, cnt, blk);
  DVP_HIP(hipGetLastError());
  WcBlock h;
  DVP_HIP(hipMemcpyAsync(&h, blk, sizeof(h), hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  rep->n_unsat = h.count[0];
  rep->first_unsat = h.first[0] == ~0ull ? -1 : (int64_t)h.first[0];
  rep->n_noncanonical = h.count[1];
  rep->first_noncanonical = h.first[1] == ~0ull ? -1 : (int64_t)h.first[1];
  rep->constant_wire_is_one = (uint32_t)h.const_one;
  if (!h.count[0]) return DVP_OK;

  const uint32_t n_list = (uint32_t)std::min<unsigned long long>(rows_cap, h.count[0]);
  const uint32_t w_cap = (uint32_t)std::min<size_t>(wires_cap, nw);
  uint32_t n_rows = 0;
  for (int k = 0; k < 3; ++k) n_rows = std::max(n_rows, p->mat[k].n_rows);
  WcScratch s2;
  Carver c2;
  const size_t o_rows = c2.take((size_t)n_list * sizeof(WcRow)), o_bad = c2.take((size_t)nw * 4), o_good = c2.take((size_t)nw * 4),
               o_wbits = c2.take((size_t)nbw * 4 * 8), o_wcnt = c2.take((size_t)nbw * 4), o_wfirst = c2.take(8),
               o_wires = c2.take((size_t)w_cap * sizeof(dvp_suspect_wire));
  DVP_TRY(s2.alloc(c2.o, st));
  char* b2 = (char*)s2.p;
  uint32_t *in_bad = (uint32_t*)(b2 + o_bad), *in_good = (uint32_t*)(b2 + o_good), *wcnt = (uint32_t*)(b2 + o_wcnt);
  unsigned long long* wbits = (unsigned long long*)(b2 + o_wbits);
  if (n_list) {
    DVP_LAUNCH(k_wc_scan, dim3(1), dim3(PT), 0, st, cnt, nb);
    DVP_LAUNCH(k_wc_list_rows, dim3(nb), dim3(PT), 0, st, A, B, C, p->coeffs_m, w, p->dD, p->n_pub, m, bits, cnt, n_list, (WcRow*)(b2 + o_rows));
  }
  DVP_HIP(hipMemsetAsync(in_bad, 0, o_wbits - o_bad, st));  // both counter vectors
  DVP_HIP(hipMemsetAsync(b2 + o_wfirst, 0xff, 8, st));
  if (n_rows) DVP_LAUNCH(k_wc_terms, dim3(cdiv(n_rows, PT)), dim3(PT), 0, st, A, B, C, n_rows, bits, in_bad, in_good);
  DVP_LAUNCH(k_wc_flag_wires, dim3(nbw), dim3(PT), 0, st, in_bad, in_good, nw, wbits, wcnt, blk, (unsigned long long*)(b2 + o_wfirst));
  if (w_cap) {
    DVP_LAUNCH(k_wc_scan, dim3(1), dim3(PT), 0, st, wcnt, nbw);
    DVP_LAUNCH(k_wc_list_wires, dim3(nbw), dim3(PT), 0, st, in_bad, nw, wbits, wcnt, w_cap, (dvp_suspect_wire*)(b2 + o_wires));
  }
  DVP_HIP(hipGetLastError());
  std::vector<dvp_suspect_wire> hw(w_cap);  // the count of suspect wires arrives with them: the caller's array gets the listed ones only
  DVP_HIP(hipMemcpyAsync(&h, blk, sizeof(h), hipMemcpyDeviceToHost, st));
  if (n_list) DVP_HIP(hipMemcpyAsync(rows, b2 + o_rows, (size_t)n_list * sizeof(WcRow), hipMemcpyDeviceToHost, st));
  if (w_cap) DVP_HIP(hipMemcpyAsync(hw.data(), b2 + o_wires, (size_t)w_cap * sizeof(dvp_suspect_wire), hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  rep->n_rows_listed = n_list;
  rep->n_suspect_wires = h.count[2];
  rep->n_wires_listed = (uint32_t)std::min<unsigned long long>(w_cap, h.count[2]);
  if (rep->n_wires_listed) memcpy(wires, hw.data(), (size_t)rep->n_wires_listed * sizeof(dvp_suspect_wire));
  return DVP_OK;
}

extern "C" int dvp_prover_check_witness_dev(dvp_prover* p, const void* d_assignment, dvp_unsat_row* rows, size_t rows_cap,
                                            dvp_suspect_wire* wires, size_t wires_cap, dvp_witness_report* report, void* stream) {
  return check_witness_impl(p, d_assignment, false, rows, rows_cap, wires, wires_cap, report, (hipStream_t)stream);
}

// the host flavours stage into p->w on the prover's own stream, as the proving entries do (prove.hip), but ask for no SRS
static int wc_stream(dvp_prover* p) {
  if (!p->own_stream) DVP_HIP(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
  return DVP_OK;
}
extern "C" int dvp_prover_check_witness(dvp_prover* p, const uint64_t* pub, uint32_t n_public, const uint64_t* prv, uint32_t n_private,
                                        dvp_unsat_row* rows, size_t rows_cap, dvp_suspect_wire* wires, size_t wires_cap,
                                        dvp_witness_report* report) {
  DVP_TRY(wc_args(p, rows, rows_cap, wires, wires_cap, report));
  if (n_public != p->n_pub || 1 + (uint64_t)n_public + n_private != p->n_wires) return DVP_EINVAL;  // dvp_prove's count rules
  if ((n_public && !pub) || (n_private && !prv)) return DVP_EINVAL;
  DVP_TRY(wc_stream(p));
  const Fr one = fr_one_canon();  // the constant wire is the library's own, as in dvp_prove
  DVP_HIP(hipMemcpyAsync(p->w, &one, sizeof(Fr), hipMemcpyHostToDevice, p->own_stream));
  if (n_public) DVP_HIP(hipMemcpyAsync(p->w + 1, pub, (size_t)n_public * 32, hipMemcpyHostToDevice, p->own_stream));
  if (n_private) DVP_HIP(hipMemcpyAsync(p->w + 1 + n_public, prv, (size_t)n_private * 32, hipMemcpyHostToDevice, p->own_stream));
  DVP_HIP(hipStreamSynchronize(p->own_stream));
  return check_witness_impl(p, p->w, false, rows, rows_cap, wires, wires_cap, report, p->own_stream);
}
// n >= n_wires elements of 32 bytes big-endian, as the witness file holds them (dvp_prove_be32's count rule).  Element 0 is not
// looked at on the host: the report says whether it reduces to 1.
extern "C" int dvp_prover_check_witness_be32(dvp_prover* p, const uint8_t* witness_be32, size_t n, dvp_unsat_row* rows, size_t rows_cap,
                                             dvp_suspect_wire* wires, size_t wires_cap, dvp_witness_report* report) {
  DVP_TRY(wc_args(p, rows, rows_cap, wires, wires_cap, report));
  if (!witness_be32 || n < p->n_wires) return DVP_EINVAL;
  DVP_TRY(wc_stream(p));
  DVP_HIP(hipMemcpyAsync(p->w, witness_be32, (size_t)p->n_wires * 32, hipMemcpyHostToDevice, p->own_stream));
  DVP_HIP(hipStreamSynchronize(p->own_stream));
  return check_witness_impl(p, p->w, true, rows, rows_cap, wires, wires_cap, report, p->own_stream);
}

// one row's terms out of the resident CSR (which = 0/1/2: A/B/C as the dump holds them); a padding row has none
extern "C" int dvp_prover_row_terms(dvp_prover* p, int which, uint32_t row, uint32_t* wire_ids, uint32_t* coeff_ids, size_t cap, size_t* n) {
  if (!p || !n || which < 0 || which > 2 || row >= p->m || (cap && (!wire_ids || !coeff_ids)) || !p->mat[which].row_ptr) return DVP_EINVAL;
  const DevCsr& mt = p->mat[which];
  *n = 0;
  if (row >= mt.n_rows) return DVP_OK;
  uint32_t rp[2];
  DVP_HIP(hipMemcpy(rp, mt.row_ptr + row, 8, hipMemcpyDeviceToHost));
  *n = rp[1] - rp[0];
  const size_t take = std::min<size_t>(cap, *n);
  if (take) {
    DVP_HIP(hipMemcpy(wire_ids, mt.wire + rp[0], take * 4, hipMemcpyDeviceToHost));
    DVP_HIP(hipMemcpy(coeff_ids, mt.coeff + rp[0], take * 4, hipMemcpyDeviceToHost));
  }
  return DVP_OK;
}
