// Host functions and structs that one translation unit of libdvpari_hip.so defines and another uses, declared ONCE.  Every file that
// defines or calls one of them includes this header, so a changed signature is a compile error instead of a silently different
// symbol.  Only the host runtime's API header is needed: the types of the device headers are forward-declared.
// (The ECFFT context -- struct dvp_ecfft with every table built for it, its lock and its destructor -- and extend_inplace / extend_from
// are ecfft_internal.h; the code behind them is ecfft.hip's stage headers ecfft_*.cuh; the C ABI is include/dvpari*.h.)
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

struct dvp_ecfft;
struct dvp_dlog_report;  // include/dvpari.h
namespace dvp {
struct Aff;
struct Fr;
struct Gf;
struct GfSqrTables;
struct MsmFixedCtx;
}  // namespace dvp

// ---- ecfft.hip, prove.hip (the context is a global type of the C ABI) ----------------------------------------------------------
int ecfft_device_consts(dvp_ecfft* c);  // ecfft_enter_exit.cuh; takes the context's lock
int ecfft_domain_tables_dev(dvp_ecfft* t, int which, dvp::Fr* d_bar_weights, dvp::Fr* d_zinv_other, hipStream_t st);  // prove.hip

namespace dvp {

extern thread_local int64_t g_last_error_index;  // capi.cpp (dvp_last_error_index)

// ---- msm.hip -----------------------------------------------------------------------------------------------------------------
int gf_sqr_tables(GfSqrTables* out, hipStream_t st);
// where an MSM leaves its result, and how the call completes
struct MsmOut {
  void* d_out_xy;               // the sum, 64 bytes
  void* d_out_inf;              // its infinity flag, u32
  void* d_out_enc = nullptr;    // + the result's 30-byte encoding, written by the tail kernel itself
  void* h_copy = nullptr;       // a device block (d_copy, copy_bytes) the caller wants on the host (pinned) when the call returns: it
  const void* d_copy = nullptr;  // rides on the MSM's own final synchronisation
  size_t copy_bytes = 0;
  // DEFERRED completion: the call returns once everything is enqueued -- no final synchronisation, no h_copy; the scalar-range word
  // (~0 = fine, else the index of the first scalar >= p) is written to this device word by the tail kernel and the caller reads it
  // with whatever it synchronises on later
  unsigned long long* d_err_defer = nullptr;
};
// one-shot MSM over (d_scalars, d_bases)
int msm_affine_dev(const void* d_scalars, const void* d_bases, const void* d_inf, size_t n, const MsmOut& out, hipStream_t st);
// fixed-base contexts: partial sum over bases [lo, hi) of the context; d_scalars / d_inf point at element lo
int msm_fixed_dev(const MsmFixedCtx* c, const void* d_scalars, const void* d_inf, uint32_t lo, uint32_t hi, const MsmOut& out, hipStream_t st);
int msm_fixed_create(const Aff* d_bases, uint32_t n_total, size_t range_hint, MsmFixedCtx** out);
void msm_fixed_destroy(MsmFixedCtx* c);
int msm_fixed_info(const MsmFixedCtx* c, int* cbits, int* windows);
uint64_t msm_fixed_table_bytes(const MsmFixedCtx* c, int* signed_flavour);
const void* msm_fixed_table_ptr(const MsmFixedCtx* c);
int msm_fixed_rows_for(size_t count);
int msm_sum_points_dev(const void* d_pts, uint32_t pt_stride_bytes, const void* d_inf32, uint32_t n, uint32_t inf_stride, void* d_out_xy,
                       void* d_out_inf, hipStream_t st);
int msm_join_points_dev(const void* d_a_xy, const void* d_a_inf, const unsigned long long* d_a_err, const void* d_b_xy, const void* d_b_inf,
                        const unsigned long long* d_b_err, uint32_t covered, void* d_out_xy, void* d_out_inf, void* d_out_enc,
                        unsigned long long* d_err_out, hipStream_t st);

// ---- codec.hip ---------------------------------------------------------------------------------------------------------------
int codec_rule_now();
int gen_table(const Aff** out, hipStream_t st);
int mulgen_dev(const void* d_scalars, size_t n, Aff* d_out, uint8_t* d_inf, hipStream_t st);
int encode_dev(const Aff* d_pts, const uint8_t* d_inf, size_t n, uint8_t* d_out, hipStream_t st);
int encode_point_dev(const Aff* d_pt, const uint32_t* d_inf32, uint8_t* d_out, hipStream_t st);
int decode_dev(const uint8_t* d_enc, size_t n, Aff* d_out, uint8_t* d_inf, hipStream_t st);
int points_check_strict(const void* d_xy, const void* d_inf, size_t n, hipStream_t st);  // a no-op unless strict mode is on
// enqueue only: resets d_summary (16 bytes: first bad index or ~0, number of bad points), then classifies; d_inf / d_classes may be null
int points_check_dev(const void* d_xy, const void* d_inf, size_t n, void* d_classes, void* d_summary, hipStream_t st);

// ---- srs_check.hip -----------------------------------------------------------------------------------------------------------
// dvp_points_check_dlog_dev with the key already settled (the caller's seed, or what it derives when there is none); d_work holds
// dlog_check_work_bytes(n) bytes, 256-byte aligned.  Waits on `st`.
size_t dlog_check_work_bytes(size_t n);
int dlog_check_dev(const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, const uint8_t key[32], uint32_t flags, void* d_work,
                   dvp_dlog_report* report, hipStream_t st);

// ---- points_mul.hip ----------------------------------------------------------------------------------------------------------
int points_mul_dev(const void* d_scalars, size_t n_scalars, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy, void* d_out_inf,
                   void* d_summary, hipStream_t st);

// ---- fr_ops.hip --------------------------------------------------------------------------------------------------------------
int batch_inverse_dev(Fr* d, size_t n, hipStream_t st);
int barycentric_dev(const Fr* dom, const Fr* wts, const Fr* ev, size_t n, Fr alpha_m, Fr z_alpha_m, int tables_mont, Fr* d_partial, Fr* d_out,
                    hipStream_t st);
// The Fr vector kernels, enqueued on st: n elements, canonical in and out, a scalar s_m in Montgomery form; o may be an input; n == 0
// launches nothing.  (What the dvp_fr_vec_* entries, the setup and dvp_prover_prepares_precomputes are made of.)
int vec_mul_dev(const Fr* a, const Fr* b, Fr* o, size_t n, hipStream_t st);               // o = a b
int vec_scale_dev(const Fr* a, Fr s_m, Fr* o, size_t n, hipStream_t st);                  // o = s a
int vec_scalar_sub_dev(Fr s, const Fr* a, Fr* o, size_t n, hipStream_t st);               // o = s - a (s canonical)
int vec_axpy_dev(const Fr* a, Fr s_m, const Fr* b, Fr* o, size_t n, hipStream_t st);      // o = a + s b
int vec_to_mont_dev(const Fr* a, Fr* o, size_t n, hipStream_t st);                        // o = a R: the scale by R
constexpr uint32_t VEC_DOT_BLOCKS = 1024;  // block partials of a dot product at most
// *d_out = <a, b> (n >= 1): block partials into d_partial (VEC_DOT_BLOCKS Fr of scratch), then one block over them
int vec_dot_dev(const Fr* a, const Fr* b, size_t n, Fr* d_partial, Fr* d_out, hipStream_t st);

// ---- blake3_tree.hip ---------------------------------------------------------------------------------------------------------
int b3_leaves_dev(const uint8_t* d_data, size_t len, uint64_t chunk_base, uint32_t* d_cvs, hipStream_t st);
int b3_single_chunk_dev(const uint8_t* d_data, size_t len, uint32_t* d_out32, hipStream_t st);
size_t b3_reduce_tmp_bytes(size_t n);
int b3_reduce_dev(uint32_t* d_cvs, size_t n, uint32_t* d_tmp, uint32_t* d_out32, hipStream_t st);

// ---- fr_digest.hip -----------------------------------------------------------------------------------------------------------
// dvp_fr_vec_digest_dev with the scratch in the caller's hands (a prover's trace digests sixteen vectors through one): d_work holds
// fr_digest_work_bytes(n) bytes, 256-byte aligned, and is free again when the work enqueued on st has run
size_t fr_digest_work_bytes(size_t n);
int fr_vec_digest_dev(const Fr* d_fr, size_t n, bool montgomery, void* d_work, uint32_t* d_out32, hipStream_t st);

// ---- circuit_hash.hip --------------------------------------------------------------------------------------------------------
// what the generator reads of the three matrices: row pointers and coefficient ids (never the wire ids)
struct ChCsr {
  const uint32_t* rp[3];
  const uint32_t* cid[3];
  uint32_t n_rows[3];
};
int circuit_hash_dev(const ChCsr& mats, const uint64_t nnz[3], const Fr* coeffs_m, uint32_t n0, const Fr* dom_m, uint32_t m, uint32_t k,
                     long long window_chunks, uint8_t out[32], hipStream_t st);

}  // namespace dvp
