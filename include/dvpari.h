/*
 * dvpari.h -- C ABI of the MI355X-native DV-Pari proving backend (libdvpari_hip.so).
 *
 * Every entry point replaces one seam of the reference prover (alpenlabs/dv-pari); the seam is
 * cited next to it as <file>:<line> in the reference tree.  The reference has no plugin/operator
 * registry: its seams are Rust functions and its only FFI today is Rust -> C into xs233
 * (src/curve.rs:13).  A Rust maintainer binds these symbols with an `extern "C"` block
 * (INTEGRATION.md shows the stub) and the existing R1CS reader / setup / verifier keep working
 * unchanged.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller allocates every buffer, outputs included;
 *  - Fr values cross as 4 x uint64 little-endian limbs of the CANONICAL value (< p), never in
 *    Montgomery form (the reference converts with into_bigint() before its own FFI,
 *    src/curve.rs:162-170);
 *  - K-233 points cross either as 30-byte xsk233 encodings (CompressedCurvePoint,
 *    src/curve.rs:66-67) or as affine (x,y) of the prime-order representative on
 *    y^2+xy=x^3+1, each coordinate 4 x uint64 LE (polynomial basis, bit i = z^i), plus an
 *    infinity flag -- never as the opaque xsk233_point struct;
 *  - `_dev` variants take DEVICE pointers (hipMalloc / torch CUDA tensors) and a hipStream_t
 *    passed as void*; they enqueue work and return without synchronising;
 *  - return value: 0 = ok, < 0 = dvp_status.  Nothing aborts or throws across the boundary
 *    (the reference's prove() unwrap()/assert!()s abort the process, src/proving.rs:437,462,548).
 */
#ifndef DVPARI_H
#define DVPARI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dvp_status {
  DVP_OK = 0,
  DVP_EINVAL = -1,  /* bad size / null pointer / non-canonical scalar */
  DVP_EDECODE = -2, /* invalid 30-byte point (assert!(valid), src/io_utils.rs:223) */
  DVP_EUNSAT = -3,  /* R1CS row unsatisfied (assert_eq!, src/proving.rs:389-395) */
  DVP_EHIP = -4,    /* HIP runtime error other than out of memory */
  /* -5 is unused: no entry point of this library calls RCCL -- partial MSM results are combined by the host
   * (one process per GPU: torch.distributed all-gather + dvp_points_sum_dev) or by peer copies (dvp_set_devices) */
  DVP_EIO = -6,
  DVP_ENOMEM = -7,  /* the HIP runtime refused an allocation (hipErrorOutOfMemory, and only that): retry with a smaller plan --
                     * dvp_prover_set_table_budget, fewer provers per device.  A prover does not return it for its tables (it proves
                     * without them), only when the working set of a proof itself does not fit */
  DVP_ECHALLENGE = -8, /* Fiat-Shamir challenge fell inside D u D' (assert!, src/proving.rs:548-556) */
  DVP_EPOINT = -9      /* an affine point is unreduced, off the curve or outside E[r]; dvp_last_error_index() = the first such point */
} dvp_status;

const char* dvp_strerror(int status);
int dvp_version(void);
/* number of visible HIP devices; <0 on error.  The library never falls back to a CPU path. */
int dvp_device_count(void);
int dvp_set_device(int device_id);
/* In-library multi-GPU behind the unchanged prove signatures: after dvp_set_devices(ids, n), n > 1, every
 * dvp_prove / dvp_prove_dev / dvp_prove_cache_dir call shards the two MSMs of the proof (src/proving.rs:463,512,680) by
 * index range over the listed devices -- each device keeps its slice of the SRS bases and its fixed-base tables, one host
 * thread per device runs the partial MSM, scalars and partial points move by hipMemcpyPeer (xGMI), and the home device
 * (ids[0] = the device the prover was created on) adds the partial points.  The Fr stages (R1CS evaluation, ECFFT
 * extends, pointwise maps; < 15 % of a proof) stay on the home device.  An id may repeat (a one-GPU box can exercise
 * the path).  n <= 1 restores single-device proving.  Proof bytes are identical for every device list. */
int dvp_set_devices(const int* device_ids, int n);
/* last failing index for DVP_EDECODE / DVP_EUNSAT / DVP_EINVAL / DVP_EPOINT (thread-local), or -1 */
int64_t dvp_last_error_index(void);

/* ------------------------------------------------------------------------------------------ */
/* ECFFT over Fr -- replaces ecfft::FFTree as built by build_sect_ecfft_tree                    */
/* (src/ec_fft.rs:197-239) and used through extend/enter/exit.                                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct dvp_ecfft dvp_ecfft;

/* domain_len = 2^log2_leaves leaves x(C' + i*G'), G' of order domain_len; shifted!=0 adds the
 * base generator (order 2^base_log2) to the coset: build_ec_fftrees(.., shift_by_one,
 * base_log_n, ..), src/ec_fft.rs:93-170.  Twiddles are regenerated from the constants at
 * src/ec_fft.rs:205-229 (the FFTR cache of src/tree_io.rs is not read). */
int dvp_ecfft_create(uint32_t log2_leaves, int shifted, uint32_t base_log2, dvp_ecfft** out);
void dvp_ecfft_destroy(dvp_ecfft* ctx);
uint32_t dvp_ecfft_log2_leaves(const dvp_ecfft* ctx);
/* FFTree::f.leaves() (src/ec_fft.rs:180): out[leaves][4], canonical */
int dvp_ecfft_leaves(const dvp_ecfft* ctx, uint64_t* out);
/* FFTree::extend(evals, Moiety::S1), call site src/proving.rs:412-415.  evals: batch vectors of
 * leaves/2 values on the even leaves; out: same shape, values on the odd leaves. */
int dvp_ecfft_extend(dvp_ecfft* ctx, const uint64_t* evals, uint32_t batch, uint64_t* out);
int dvp_ecfft_extend_dev(dvp_ecfft* ctx, const void* d_evals, uint32_t batch, void* d_out, void* stream);
/* FFTree::enter / FFTree::exit, call sites src/ec_fft.rs:266,317,411: `leaves` coefficients <->
 * `leaves` evaluations on all leaves. */
int dvp_ecfft_enter(dvp_ecfft* ctx, const uint64_t* coeffs, uint64_t* evals_out);
int dvp_ecfft_exit(dvp_ecfft* ctx, const uint64_t* evals, uint64_t* coeffs_out);
int dvp_ecfft_enter_dev(dvp_ecfft* ctx, const void* d_coeffs, void* d_out, void* stream);
int dvp_ecfft_exit_dev(dvp_ecfft* ctx, const void* d_evals, void* d_out, void* stream);
/* Z_D(x), Z_D'(x) for the even (which=0) / odd (which=1) half of the leaves, evaluated through
 * the isogeny chain (replaces DensePolynomial::evaluate on z_poly, src/ec_fft.rs:475) */
int dvp_ecfft_vanish_at(const dvp_ecfft* ctx, int which, const uint64_t x[4], uint64_t out[4]);

/* ------------------------------------------------------------------------------------------ */
/* Fr vector kernels -- ark_ff::batch_inversion (src/proving.rs:604,614; src/ec_fft.rs:482)     */
/* and evaluate_poly_at_alpha_using_barycentric_weights (src/ec_fft.rs:455-491).                */
/* ------------------------------------------------------------------------------------------ */
int dvp_fr_batch_inverse(uint64_t* vals, size_t n); /* in place; zeros stay zero */
int dvp_fr_batch_inverse_dev(void* d_vals, size_t n, void* stream);
/* the rayon pointwise maps of src/proving.rs:492-654 and the setup loops of src/srs.rs:53-84,138-160
 * as reusable vector ops (canonical in, canonical out): out = a o b ; out = s*a ; out = s - a ;
 * <a,b> ; sparse rows out[r] = sum coeffs[cid]*x[col] (eval_row, src/gnark_r1cs.rs:273-280) */
int dvp_fr_vec_mul(const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
int dvp_fr_vec_scale(const uint64_t* a, const uint64_t s[4], size_t n, uint64_t* out);
/* out[i] = a[i] + s * b[i]: the (A + delta B + delta^2 C) combination of accumulate_m_values' three sums (src/srs.rs:73-80) */
int dvp_fr_vec_axpy(const uint64_t* a, const uint64_t s[4], const uint64_t* b, size_t n, uint64_t* out);
int dvp_fr_vec_scalar_sub(const uint64_t s[4], const uint64_t* a, size_t n, uint64_t* out);
int dvp_fr_vec_dot(const uint64_t* a, const uint64_t* b, size_t n, uint64_t out[4]); /* n = 0: out = 0, a and b are not read */
/* CSR rows: row_ptr holds n_rows + 1 non-decreasing offsets into col / coeff_ids, the last one their length.  DVP_EINVAL, before any
 * device work, for a row r with row_ptr[r] > row_ptr[r + 1] or row_ptr[r + 1] > row_ptr[n_rows] (dvp_last_error_index() = r) and
 * for an entry k with col[k] >= n_cols or coeff_ids[k] >= n_coeffs (index k); col / coeff_ids may be NULL only when there is no entry */
int dvp_fr_spmv(const uint32_t* row_ptr, const uint32_t* col, const uint32_t* coeff_ids, uint32_t n_rows,
                const uint64_t* coeffs, uint32_t n_coeffs, const uint64_t* x, uint32_t n_cols, uint64_t* out);
int dvp_barycentric_eval(const uint64_t* domain, const uint64_t* bar_weights, const uint64_t z_at_alpha[4],
                         const uint64_t* evals, size_t n, const uint64_t alpha[4], uint64_t out[4]);
/* gnark_element_to_fr over a vector (src/gnark_r1cs.rs:58-77,188-211): n x 32 bytes big-endian, any value below 2^256, -> n x 4
 * canonical limbs, exactly Fr::from_be_bytes_mod_order, one lane per element on the device.  n = 0 is DVP_OK and touches nothing.  The
 * host flavour takes be32 at any alignment (a witness file's payload starts at byte 4).  The _dev flavour only enqueues on `stream`;
 * d_out may equal d_be32 (in place: a lane reads and writes only its own 32 bytes); DVP_EINVAL before any device call for a NULL
 * pointer with n > 0, for a pointer that is not 16-byte aligned and for n > 2^32 - 256 (one launch; the file format counts in 32 bits). */
int dvp_fr_from_be32(const uint8_t* be32, size_t n, uint64_t* out /* n x 4 */);
int dvp_fr_from_be32_dev(const void* d_be32, size_t n, void* d_out /* may equal d_be32 */, void* stream);
/* Fr as arkworks holds it in memory <-> canonical limbs.  The crate's Fr is Fp256<MontBackend<FqConfig, 4>> (src/curve.rs:16-22): four
 * little-endian u64 holding a * 2^256 mod p, below p -- what `slice.as_ptr() as *const u64` points at.  from_ark is into_bigint() over a
 * vector (out = x * 2^-256 mod p), to_ark is Fr::from_bigint (out = a * 2^256 mod p); one lane per element on the device.  Both are
 * total: any value below 2^256 is reduced mod p first, the result is canonical.  n = 0 is DVP_OK and touches nothing.  The host
 * flavours take any alignment.  The _dev flavours only enqueue on `stream`; d_out NULL or == d_in converts in place (a lane reads and
 * writes only its own 32 bytes); DVP_EINVAL before any device call for d_in NULL with n > 0, for a pointer that is not 16-byte aligned
 * and for n > 2^32 - 256 (one launch). */
int dvp_fr_from_ark(const uint64_t* ark /* n x 4 */, size_t n, uint64_t* out /* n x 4 */);
int dvp_fr_to_ark(const uint64_t* limbs /* n x 4 */, size_t n, uint64_t* out_ark /* n x 4 */);
int dvp_fr_from_ark_dev(const void* d_in, size_t n, void* d_out /* NULL or == d_in: in place */, void* stream);
int dvp_fr_to_ark_dev(const void* d_in, size_t n, void* d_out /* NULL or == d_in: in place */, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* sect233k1 / xsk233 group                                                                     */
/* ------------------------------------------------------------------------------------------ */
/* multi_scalar_mul(&[Fr], &[CurvePoint]) -> CurvePoint, src/curve.rs:141-158 (call sites
 * src/proving.rs:463,512,680).  Affine flavour: bases_xy[n][8] = x||y of the E[r]
 * representative; bases_inf[n] (may be NULL) marks neutral elements. */
int dvp_msm_affine(const uint64_t* scalars, const uint64_t* bases_xy, const uint8_t* bases_inf, size_t n,
                   uint64_t out_xy[8], int* out_is_infinity);
/* sum of n partial points held as 80-byte records (x || y, u32 infinity flag, pad): what the ranks of a multi-process
 * prove all-gather, combined with n - 1 additions (RCCL has no reduction for curve points) */
int dvp_points_sum_dev(const void* d_records, uint32_t n, void* d_out_xy, void* d_out_inf, void* stream);
int dvp_msm_affine_dev(const void* d_scalars, const void* d_bases_xy, const void* d_bases_inf, size_t n,
                       void* d_out_xy /*8 x u64*/, void* d_out_inf /*u32*/, void* stream);
/* Fixed-base flavour of the same seam: the reference calls multi_scalar_mul with the SAME bases (the SRS
 * vectors g_m, g_q, g_k_*) in every proof, so a multiple 2^(o_w) P of every base is computed once for every window w
 * (W x the storage) and all windows then share one bucket set.  range_hint = bases a typical call covers
 * (the per-GPU shard; 0 = n).  run: sum over i in [lo, hi) of scalars[i - lo] * base[i]. */
typedef struct dvp_msm_ctx dvp_msm_ctx;
/* DVP_ENOMEM: the table does not fit the device.  There is no fallback inside a context -- the context IS the table -- so the caller
 * uses dvp_msm_affine (the one-shot MSM, no table) for these bases then. */
int dvp_msm_ctx_create(const uint64_t* bases_xy, const uint8_t* bases_inf, size_t n, size_t range_hint, dvp_msm_ctx** out);
void dvp_msm_ctx_destroy(dvp_msm_ctx* ctx);
/* window bits c and window count the context settled on (all W windows share one bucket set: 2^(c-1) buckets of |digit| for the
 * default signed windows) */
int dvp_msm_ctx_plan(const dvp_msm_ctx* ctx, int* c_bits, int* windows);
/* HBM held by the context's precomputed table.  Default flavour: aligned windows of signed binary digits over W ~ 12 multiples
 * 2^(o_w) P of every base (0.77 KB per base: 3.2 GB for the 4m bases of a 2^20-constraint prover); DVP_MSM_ALIGNED_SIGNED = 0
 * (environment, read once) selects aligned tau-adic windows over W + 1 Frobenius images instead.  *signed_windows (may be NULL)
 * reports which one this is (1 = the default).  Results do not depend on the flavour. */
uint64_t dvp_msm_ctx_table_bytes(const dvp_msm_ctx* ctx, int* signed_windows);
int dvp_msm_ctx_run(dvp_msm_ctx* ctx, const uint64_t* scalars, size_t lo, size_t hi, uint64_t out_xy[8], int* out_is_infinity);
int dvp_msm_ctx_run_dev(dvp_msm_ctx* ctx, const void* d_scalars, size_t lo, size_t hi, void* d_out_xy, void* d_out_inf, void* stream);
/* dvp_msm_ctx_run with the hi - lo scalars as arkworks holds them (the &[Fr] of multi_scalar_mul, src/curve.rs:141-158; see
 * dvp_fr_from_ark): they are copied into the call's own device buffer and converted there. */
int dvp_msm_ctx_run_ark(dvp_msm_ctx* ctx, const uint64_t* scalars_ark, size_t lo, size_t hi, uint64_t out_xy[8], int* out_is_infinity);
/* same seam with the reference's own wire formats: scalars n x 32 B canonical LE, bases n x 30 B
 * xsk233 encodings (read_point_vec_from_file payload, src/io_utils.rs:187-239). */
int dvp_msm_xsk233(const uint8_t* scalars, const uint8_t* bases_enc, size_t n, uint8_t out_enc[30]);
/* multi_scalar_mul(&[Fr], &[CurvePoint]) itself, src/curve.rs:141-158: the scalars are the slice's memory (n x 4 u64, arkworks form,
 * see dvp_fr_from_ark), converted on the device; everything else is dvp_msm_xsk233. */
int dvp_msm_xsk233_ark(const uint64_t* scalars_ark, const uint8_t* bases_enc, size_t n, uint8_t out_enc[30]);

/* point_scalar_mul_gen over a vector + to_bytes: the SRS commitment loop of
 * compute_srs_matrices, src/srs.rs:126-160 (one fixed-base multiplication per scalar). */
int dvp_mulgen_batch(const uint64_t* scalars, size_t n, uint8_t* out_enc /* n x 30 */);
int dvp_mulgen_batch_affine(const uint64_t* scalars, size_t n, uint64_t* out_xy /* n x 8 */, uint8_t* out_inf);

/* CurvePoint::to_bytes / from_bytes over vectors (src/curve.rs:93-109, src/io_utils.rs:217-226) */
int dvp_points_encode(const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_enc);
int dvp_points_decode(const uint8_t* enc, size_t n, uint64_t* out_xy, uint8_t* out_inf);
/* Which presentation of the encoded field element the 30 bytes of a point hold.  The reference reaches its codec through
 * xs233 (src/curve.rs:93-109), whose source is not available offline and for which the reference holds no known-answer
 * bytes, so the rule is selectable: rule = bit 0: the element is w + 1 | bit 1: big-endian bytes | bits 2..3: 0 w = sqrt(s/x),
 * 1 w^2 (= s/x = lambda), 2 sqrt(w) -- the classes every candidate of tools/pin_xsk233.py falls into; 0 (default) is the
 * candidate followed so far.  tools/pin_xsk233.py <k> <bytes of k G from xs233> names the number to set.  Process-wide; files
 * written under one rule must be read under it.  DVP_CODEC_RULE in the environment sets the initial value. */
int dvp_codec_set_rule(int rule);
int dvp_codec_get_rule(void);
/* CurvePoint::add over two vectors (src/curve.rs:84-90; complete: doubling, inverses, neutral).  Equality of two
 * CurvePoints (src/curve.rs:69-76) is equality of (x, y, infinity) on this representation. */
int dvp_points_add(const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, size_t n, uint64_t* out_xy,
                   uint8_t* out_inf);

/* point_scalar_mul over a vector (src/curve.rs:113-126, the operation multi_scalar_mul is made of): out[i] = k_i P_i for n independent
 * pairs, one launch.  scalars: canonical (< r), 4 u64 limbs each; n_scalars = n, or 1 = one scalar for every point; anything else is
 * DVP_EINVAL.  xy / inf as everywhere (inf may be NULL); out_inf[i] = 1 with zero coordinates for O (k_i = 0 or P_i = O).
 * dvp_points_mul / dvp_points_mul_xsk233: n = 0 is DVP_OK and touches nothing; a NULL scalars / xy / enc or a NULL output with n > 0 and
 * a wrong n_scalars are DVP_EINVAL before any device call; a non-canonical scalar is DVP_EINVAL with dvp_last_error_index() = the
 * first such scalar, and no output is written.  dvp_points_mul_xsk233 takes and gives the reference's wire formats (scalars 32 B LE,
 * points 30 B, under the codec rule in force); a bad encoding is DVP_EDECODE with its index.
 * dvp_points_mul_dev: enqueues on `stream` and returns, never waits on the host and never checks points; d_out_xy may equal d_xy,
 * d_inf may be NULL.  A non-canonical scalar makes its lane produce O and is reported in d_summary = { u64 first such index or ~0,
 * u64 their number }, which the call itself resets (the layout of dvp_points_check_dev). */
int dvp_points_mul(const uint64_t* scalars, size_t n_scalars, const uint64_t* xy, const uint8_t* inf /* may be NULL */, size_t n,
                   uint64_t* out_xy, uint8_t* out_inf);
int dvp_points_mul_dev(const void* d_scalars, size_t n_scalars, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy,
                       void* d_out_inf, void* d_summary /* 16 bytes, written by the call */, void* stream);
int dvp_points_mul_xsk233(const uint8_t* scalars /* n_scalars x 32 B LE */, size_t n_scalars, const uint8_t* enc /* n x 30 B */,
                          size_t n, uint8_t* out_enc /* n x 30 B */);

/* out[j] = sum over seg_ptr[j] <= i < seg_ptr[j+1] of k_i P_i, for j < n_seg: n_seg independent multi_scalar_mul
 * (src/curve.rs:141-158) over consecutive slices of one scalar vector and one point vector, in one call.  Stage 1 is dvp_points_mul_dev
 * over all n pairs; stage 2 sums the products of every segment with complete additions: pieces of at most P = DVP_MSM_SEG_PIECE
 * consecutive operands, one lane each, level after level until every segment has one sum (at most
 * P ceil(log_P(longest segment)) dependent additions and one inversion behind stage 1, whatever the cut).  Results are affine, so they
 * do not depend on P or on DVP_POINTS_MUL_W.
 * seg_ptr is CSR-style, as row_ptr of dvp_fr_spmv, and a HOST array in every flavour: seg_ptr[0] = 0, non-decreasing,
 * seg_ptr[n_seg] = n.  DVP_EINVAL before any device call, with dvp_last_error_index() = the first offending j: 0 for seg_ptr[0] != 0,
 * j for seg_ptr[j] > seg_ptr[j + 1] or seg_ptr[j + 1] > n, n_seg - 1 for seg_ptr[n_seg] < n.  Empty segments are allowed anywhere and
 * give O (out_inf = 1, zero coordinates; the xsk233 flavour: the neutral element's encoding).  n_seg = 0 is DVP_OK and touches nothing;
 * n = 0 with n_seg > 0 writes n_seg times O (the host flavours without a device).  NULL required pointers, n or n_seg >= 2^32 and a
 * work_bytes below dvp_msm_segments_work_bytes(n, n_seg) are DVP_EINVAL before any device call.
 * dvp_msm_segments / dvp_msm_segments_xsk233: as dvp_points_mul -- in strict mode the points are checked first (DVP_EPOINT with the
 * index), then a non-canonical scalar is DVP_EINVAL with its index; no output is written in either case; a bad encoding is
 * DVP_EDECODE with its index.
 * dvp_msm_segments_dev: enqueues on `stream` and returns; never checks points; allocates nothing on the device.  A lane with a
 * non-canonical scalar contributes O and is reported in d_summary (the layout of dvp_points_mul_dev; the call resets it); every
 * segment is still written.  d_work is the caller's: dvp_msm_segments_work_bytes (pure host arithmetic, non-decreasing in both
 * arguments, enough for every admissible DVP_MSM_SEG_PIECE) bytes that no other work in flight uses.  The outputs must not overlap the
 * inputs or d_work.  The offsets of every level are computed on the host from seg_ptr -- O(n_seg) per level, seg_ptr is not read after
 * the call returns -- and reach the device through a ring of four pinned staging buffers the library owns, one asynchronous copy on
 * `stream` per call.  The call does not wait for work already on `stream`.  What it can block on: (1) the geometry copy of the call
 * four calls before it, when that copy has not run yet because the work in front of it on ITS stream has not finished; (2) a pinned
 * allocation, when the call needs more staging bytes than the slot it is given has held before (the runtime may synchronise the device
 * there); (3) the first call on a device, which builds the inversion tables every entry of the group shares.
 * When to call dvp_msm_affine per segment instead: the one-shot pipeline is ~33 dependent launches per call whatever its size, this
 * entry pays ~58 additions per point whatever the cut; measured on one MI355X (tools/README.md, "Segmented MSM") a loop of
 * dvp_msm_affine_dev overtakes this entry between 4096 and 65536 points per segment (loop / this entry = 2.9-4.7 at
 * 4096 points, 0.3-0.5 at 65536; near 2^14-2^15 by interpolation): call dvp_msm_affine per segment for segments of 2^15 points and up.
 * Out of scope here: gathered bases (a column index per term), a per-segment bucket method in LDS, fusing the reduction into the
 * multiplication kernel, a device-resident seg_ptr, and use of this entry inside the prover. */
int dvp_msm_segments(const uint64_t* scalars /* n x 4 */, const uint64_t* xy /* n x 8 */, const uint8_t* inf /* may be NULL */, size_t n,
                     const uint64_t* seg_ptr /* n_seg + 1 */, size_t n_seg, uint64_t* out_xy /* n_seg x 8 */, uint8_t* out_inf /* n_seg */);
size_t dvp_msm_segments_work_bytes(size_t n, size_t n_seg);
int dvp_msm_segments_dev(const void* d_scalars, const void* d_xy, const void* d_inf /* may be NULL */, size_t n,
                         const uint64_t* seg_ptr /* HOST, n_seg + 1, read only during the call */, size_t n_seg,
                         void* d_out_xy, void* d_out_inf /* n_seg bytes */, void* d_work, size_t work_bytes,
                         void* d_summary /* 16 bytes, written by the call */, void* stream);
int dvp_msm_segments_xsk233(const uint8_t* scalars /* n x 32 B LE */, const uint8_t* enc /* n x 30 B */, size_t n,
                            const uint64_t* seg_ptr, size_t n_seg, uint8_t* out_enc /* n_seg x 30 B */);

/* Affine points checked on the device.  The kernels behind the affine entries assume points of E[r] (the prime-order subgroup) with
 * reduced coordinates; the 30-byte path can only produce such points (dvp_points_decode), the affine path takes what it is given.
 * Every point i with inf[i] == 0 (inf == NULL: every point) gets exactly one class; a point with inf[i] != 0 is class 0 whatever its
 * coordinates hold.
 *   0                    reduced, on y^2 + xy = x^3 + 1, in E[r]
 *   DVP_POINT_UNREDUCED  a bit in 233 .. 255 of x or y is set
 *   DVP_POINT_OFF_CURVE  reduced, but the curve equation fails ((0,0) and (0, y != 1) included)
 *   DVP_POINT_ORDER4     on the curve, x != 0, Tr(x) = 1: not even in 2E
 *   DVP_POINT_COSET_N    on the curve and P + N in E[r], N = (0,1) (N itself included): xsk233's OWN affine view of a group element
 *                        (xsk233 = { P + N : P in E[r] }); this library takes the E[r] representative P or the 30-byte encoding
 * dvp_points_check: DVP_OK when every point is class 0, else DVP_EPOINT with dvp_last_error_index() = the first bad point; classes
 * (optional, n bytes) and *n_bad (optional) are filled either way.  n = 0: DVP_OK, nothing is touched.
 * dvp_points_check_dev: enqueues on `stream` and returns DVP_OK; the verdict is d_summary = { u64 first bad index or ~0, u64 number
 * of bad points }, which the call itself resets (it need not be initialised); d_inf and d_classes may be NULL.
 *
 * Strict mode (process-wide like dvp_codec_set_rule; initial value DVP_POINTS_STRICT from the environment, default 0 = off): when on,
 * the entries that copy affine points from the caller -- dvp_msm_affine, dvp_msm_ctx_create, dvp_prover_set_srs_affine,
 * dvp_prover_set_srs_affine_dev, dvp_points_add, dvp_points_encode, dvp_points_mul, dvp_msm_segments -- run the check on their device copy before anything else uses
 * it and return DVP_EPOINT with the index of the first bad point.  dvp_points_add checks operand a, then operand b: the index is that
 * of the first bad point of a, and only when a is clean that of the first bad point of b (both count from 0).  dvp_points_mul and dvp_msm_segments check their
 * points before their scalars: a bad point together with a bad scalar is DVP_EPOINT.  After a failure
 * dvp_msm_ctx_create has freed what it allocated and not written *out, and the SRS setters leave vector `which` UNSET: a later proof
 * fails as it does for a vector that was never given, never on stale or rejected bases.
 * NEVER checked, strict or not: the `_dev` run entries dvp_msm_affine_dev, dvp_msm_ctx_run_dev, dvp_points_sum_dev, dvp_points_mul_dev, dvp_msm_segments_dev and the prover's own
 * buffers -- they must not wait on the host; a caller who wants a check there enqueues dvp_points_check_dev itself. */
#define DVP_POINT_UNREDUCED 0x01u
#define DVP_POINT_OFF_CURVE 0x02u
#define DVP_POINT_ORDER4 0x04u
#define DVP_POINT_COSET_N 0x08u
int dvp_points_check(const uint64_t* xy, const uint8_t* inf /* may be NULL */, size_t n, uint8_t* classes /* optional, n bytes */,
                     size_t* n_bad /* optional */);
int dvp_points_check_dev(const void* d_xy, const void* d_inf, size_t n, void* d_classes /* optional */,
                         void* d_summary /* 16 bytes, written by the call */, void* stream);
int dvp_points_set_strict(int on);
int dvp_points_get_strict(void);

/* "Are these points the given multiples of G?": P_i == s_i G for every i < n, checked on the device (csrc/srs_check.hip).  The claims
 * are linear in the group, so they fold into ONE multi-scalar multiplication of n + 1 points, the argument of dvp_verify_batch_rlc:
 *     sum_i r_i P_i + (p - sum_i r_i s_i) G == O      <=>      sum_i r_i (P_i - s_i G) == O.
 * scalars: n x 4 limbs, canonical; xy / inf as everywhere (inf may be NULL); inf[i] != 0 means O, which is right exactly when s_i = 0.
 * The return value is DVP_OK whenever the check ran: the answer is in *report.  A scalar that is not below p is DVP_EINVAL with
 * dvp_last_error_index() = its index (the host flavour finds it before any device work, the _dev flavour after the points were
 * checked); n = 0 gives verdict 0 and touches nothing but *report; n >= 2^27 is DVP_EINVAL (the one-shot MSM's limit).
 *   1. dvp_points_check_dev over the points.  A bad point gives DVP_DLOG_BAD_POINT with its index and class and nothing further runs:
 *      the MSM never sees a point outside E[r] (see DVP_POINT_COSET_N above: its kernels assume E[r]).
 *   2. h = BLAKE3 of the points as given -- the n x 64 xy bytes, then the n infinity bytes (NULL: n zero bytes) -- by the device hash
 *      of dvp_blake3_dev; key = seed (32 bytes), or BLAKE3("dv-pari dlog check v1") for seed == NULL; k = BLAKE3(key || h);
 *      r_i = (first 16 bytes of BLAKE3(k || LE64(i)), read little-endian) | 2^127.  Hashing the points into k fixes the coefficients
 *      only after the points are, so the check stays sound under a predictable seed -- which the seed is when none is passed.
 *   3. one lane per element computes r_i (MSM scalar i) and r_i s_i; block sums give MSM scalar n = p - sum r_i s_i, MSM base n = G.
 *   4. the one-shot MSM.  O: verdict 0, path DVP_DLOG_PATH_COMBINED.  Error bound: fix every coefficient but one; at most one value
 *      mod p of the last cancels a non-zero error and the coefficient takes 2^127 values, so a wrong vector passes with probability at
 *      most 2^-127 (BLAKE3 read as a random oracle).
 *   5. otherwise (path DVP_DLOG_PATH_LOCATED), or alone under DVP_DLOG_CHECK_EXACT (path DVP_DLOG_PATH_EXACT, no hash involved): s_i G
 *      by the batched fixed-base multiplication in batches of at most 2^20, compared entry for entry in index order up to the first
 *      batch that differs: verdict DVP_DLOG_WRONG with first_bad exact.
 * The scalars may be trapdoor material (the discrete logs of an SRS): every buffer of the library that held s_i, r_i s_i or their sums
 * is zeroed before it is freed or handed back, on every exit.
 * dvp_points_check_dlog_dev: device pointers; d_work is the caller's, 256-byte aligned, dvp_points_check_dlog_work_bytes(n) bytes
 * (pure host arithmetic, at most about 170 bytes per point) that nothing else in flight uses; fewer is DVP_EINVAL.  It allocates nothing on
 * the device.  It waits on the host for the verdict of step 1 (so that no MSM kernel is enqueued over bad points), for the MSM's
 * result, and per batch when it has to locate; *report is complete when it returns. */
#define DVP_DLOG_CHECK_EXACT 0x1u /* skip the combined check: compare every point */
#define DVP_DLOG_BAD_POINT 0x1u   /* a point outside E[r] / unreduced / off the curve */
#define DVP_DLOG_WRONG 0x2u       /* well-formed, but some P_i != s_i G */
#define DVP_DLOG_PATH_COMBINED 1u
#define DVP_DLOG_PATH_LOCATED 2u /* the combined check failed, then the entry was located */
#define DVP_DLOG_PATH_EXACT 3u
typedef struct dvp_dlog_report {
  uint32_t verdict;    /* 0 = every P_i equals s_i G; else DVP_DLOG_* bits */
  uint32_t path;       /* DVP_DLOG_PATH_* */
  int64_t first_bad;   /* index of the first wrong or ill-formed point, -1 when none */
  uint8_t point_class; /* dvp_points_check class of that point, 0 when it is a well-formed wrong point */
} dvp_dlog_report;
int dvp_points_check_dlog(const uint64_t* scalars /* n x 4, canonical */, const uint64_t* xy, const uint8_t* inf /* may be NULL */, size_t n,
                          const uint8_t* seed /* 32 bytes or NULL */, uint32_t flags, dvp_dlog_report* report);
int dvp_points_check_dlog_dev(const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, const uint8_t* seed, uint32_t flags,
                              void* d_work, size_t work_bytes, dvp_dlog_report* report, void* stream);
size_t dvp_points_check_dlog_work_bytes(size_t n);

/* ------------------------------------------------------------------------------------------ */
/* Prover -- Proof::prove(cache_dir, public_inputs, private_inputs), src/proving.rs:426-688,      */
/* with the cache_dir artefacts handed over once and kept resident in HBM.                      */
/* ------------------------------------------------------------------------------------------ */
typedef struct dvp_prover dvp_prover;
#define DVP_MAX_LOG2_CONSTRAINTS 24 /* largest validated / index-safe size; dvp_prover_create returns DVP_EINVAL above it */

/* m = 2^log2_m constraints (R1CSInstance::num_constraints, src/gnark_r1cs.rs:291); witness vector
 * = [1, public.., private..] of n_wires entries (src/proving.rs:355-359).  Builds TREE_2N and the
 * prover precomputes of prover_prepares_precomputes (src/proving.rs:225-325) on the device. */
int dvp_prover_create(uint32_t log2_m, uint32_t n_public, uint32_t n_wires, dvp_prover** out);
void dvp_prover_destroy(dvp_prover* p);
/* coefficient table of the R1CS dump (canonical; src/gnark_r1cs.rs:282-296) */
int dvp_prover_set_coeffs(dvp_prover* p, const uint64_t* coeffs, uint32_t n);
/* one of L/R/O (which = 0/1/2) as CSR over n_rows <= m rows of (wire_id, coeff_id) terms
 * (src/gnark_r1cs.rs:97-119).  The Vandermonde fold of update_to_include_vandermode_matrix_d
 * (:333-386) is applied inside the kernel, do not pre-apply it. */
int dvp_prover_set_matrix(dvp_prover* p, int which, uint32_t n_rows, const uint32_t* row_ptr, const uint32_t* wire_ids,
                          const uint32_t* coeff_ids);
/* SRS vectors, which = 0 g_m (n_wires), 1 g_q (m), 2 g_k_0 (m), 3 g_k_1 (m), 4 g_k_2 (2m)
 * (src/artifacts.rs:18-83, src/srs.rs:126-160): file payload (n x 30 B) or affine. */
int dvp_prover_set_srs_encoded(dvp_prover* p, int which, const uint8_t* enc, size_t n);
int dvp_prover_set_srs_affine(dvp_prover* p, int which, const uint64_t* xy, const uint8_t* inf, size_t n);
int dvp_prover_set_srs_affine_dev(dvp_prover* p, int which, const void* d_xy, const void* d_inf, size_t n);
/* proof = commit_p[30] | kzg_k[30] | a0[29] | b0[29]: the byte image of Proof::to_bits (:691-718) */
int dvp_prove(dvp_prover* p, const uint64_t* public_inputs, uint32_t n_public, const uint64_t* private_inputs,
              uint32_t n_private, uint8_t proof[118]);
/* the same with the assignment [1, public.., private..] (n_wires canonical Fr) already in HBM */
int dvp_prove_dev(dvp_prover* p, const void* d_assignment, uint8_t proof[118], void* stream);
/* load_witness_from_file's payload -> Proof::prove (src/gnark_r1cs.rs:188-211, src/dvsnark_test.rs:189-229): the first n_wires
 * elements of [1, public.., private..] as the witness file holds them, 32 bytes big-endian each and NOT reduced -- the bytes are
 * copied into the prover's witness buffer and reduced mod p there, on the device (dvp_fr_from_be32_dev, in place); everything else
 * is dvp_prove (device lists, transcript flavours, table budgets, bindings, error order).  n < n_wires is DVP_EINVAL; n > n_wires
 * reads the first n_wires elements only (the reference's zip truncates the same way).  Element 0 must reduce to 1 (1 + p is
 * accepted), else DVP_EINVAL with dvp_last_error_index() = 0, before any device work; no other element is looked at on the host. */
int dvp_prove_be32(dvp_prover* p, const uint8_t* witness_be32, size_t n, uint8_t proof[118]);
/* dvp_prove with both vectors as arkworks holds them (Proof::prove's public_inputs: Vec<Fr> and private_inputs: &[Fr],
 * src/proving.rs:426-452; the layout is dvp_fr_from_ark's): the bytes are copied into the prover's witness buffer and converted there,
 * on the device, in place (one dvp_fr_from_ark_dev over elements 1 .. n_wires - 1 on the prover's own stream); the constant wire is
 * written by the library.  No host-side conversion and no host wait beyond dvp_prove's.  Everything else is dvp_prove: counts and
 * NULL pointers are DVP_EINVAL, an unsatisfied witness is DVP_EUNSAT with the same row. */
int dvp_prove_ark(dvp_prover* p, const uint64_t* public_ark, uint32_t n_public, const uint64_t* private_ark, uint32_t n_private,
                  uint8_t proof[118]);

/* One witness, many verifiers.  DV-Pari is designated-verifier: every verifier runs the setup with a trapdoor of its own and so has
 * an SRS of its own (SRS per Trapdoor, src/srs.rs:31-50,177), while the circuit, the witness and everything a proof computes before
 * its first MSM do not depend on the SRS.  A prover therefore holds SRS SLOTS.  A slot is what depends on the SRS: the five base
 * vectors, their fixed-base tables and table budget, and the transcript binding (bind-srs makes it a function of the SRS).  A new
 * prover has slot 0 and it is active; every other entry of this header -- the SRS setters, every prove form, the staged begin ..
 * finish entries, dvp_prover_srs_hash, dvp_prover_set_transcript_binding, dvp_prover_msm_plan / _coverage / _table_bytes /
 * _partial, dvp_prover_set_table_budget, dvp_prover_trace_last -- acts on the ACTIVE slot and does what it did before slots existed.
 *
 * dvp_prover_srs_slot_add     (src/srs.rs:31-50,177) a new empty slot, or a dropped index reused: no bases (its first setter allocates
 *                             them), no table limit, the reference's binding (hashes of empty buffers).  Not selected.
 * dvp_prover_srs_slot_select  (src/srs.rs:31-50,177) makes `slot` active: a swap of host-side fields, no device work and no wait.
 *                             Unless the slot is active already, dvp_prover_trace_last answers afterwards as after an SRS setter.
 * dvp_prover_srs_slot_active / _count  (src/srs.rs:31-50,177) the active index / the number of indices ever handed out.
 * dvp_prover_srs_slot_drop    (src/srs.rs:31-50,177) waits for the device (every stream), frees the slot's bases and tables and
 *                             leaves the index empty and reusable.  The active slot or an unknown index: DVP_EINVAL.
 * dvp_prover_srs_slot_bytes   (src/srs.rs:31-50,177) what the slot holds on the device now: the base vectors with their flag bytes
 *                             (65 bytes per point, 0 before the first setter) and the tables (built by the slot's first proof, so 0
 *                             before it; 0 for ever under a budget of 0).  A dropped index answers (0, 0).
 *
 * The table budget is per slot: the device total is the SUM over the slots (dvp_prover_msm_coverage on each selected slot says what
 * that slot got).  Limit: slots and a device list do not combine.  With a list of more than one device in force (dvp_set_devices)
 * dvp_prover_srs_slot_add is DVP_EINVAL, and while any prover holds more than one slot such a list is DVP_EINVAL: the shards hold
 * per-device slices of one SRS. */
int dvp_prover_srs_slot_add(dvp_prover* p, uint32_t* slot);
int dvp_prover_srs_slot_select(dvp_prover* p, uint32_t slot);
uint32_t dvp_prover_srs_slot_active(const dvp_prover* p);
uint32_t dvp_prover_srs_slot_count(const dvp_prover* p);
int dvp_prover_srs_slot_drop(dvp_prover* p, uint32_t slot);
int dvp_prover_srs_slot_bytes(const dvp_prover* p, uint32_t slot, uint64_t* bases, uint64_t* tables);
/* Proof::prove (src/proving.rs:426-688) of ONE witness for the SRS of every listed slot (src/srs.rs:31-50,177): phase 1 -- the R1CS
 * rows, the unsatisfied-row check, the extends, the quotient -- runs once; then, per slot in the order given, exactly what
 * dvp_prove_dev runs after it: the commitment MSM over the slot's bases, the transcript under the slot's binding, the challenge
 * phase, the K MSM, and the 118 bytes into proofs + 118 j.  The flavour (device or host transcript) is chosen as dvp_prove_dev
 * chooses it.  A slot may repeat (same bytes twice).
 *   Arguments: NULL pointers and n_slots == 0 are DVP_EINVAL; a slot index never handed out or dropped is DVP_EINVAL with
 *     dvp_last_error_index() = its position in `slots`; both before any device work.
 *   The witness: DVP_EUNSAT with its row, or DVP_EINVAL with the index of a scalar >= p, shows at the first slot's wait as in a
 *     single proof; the call returns it, proves no further slot and leaves `proofs` untouched.
 *   A slot: status[j] = DVP_OK, DVP_EINVAL for a slot that lacks one of its five vectors, DVP_ECHALLENGE, or an MSM's status; the
 *     other slots are proven all the same and the call returns DVP_OK.  proofs + 118 j is written only where status[j] == DVP_OK.
 *   On return the slot that was active at the call is active again; dvp_prover_trace_last is valid only if the last listed slot is
 *     that slot and its proof succeeded, and otherwise answers as after an SRS setter.
 *   Host waits: what dvp_prove_dev waits, once per slot, and none for phase 1: in the device-transcript flavour one stream wait per
 *     slot (plus one per MSM that is too small for a first pair round, as in a single proof).
 * The host forms stage the witness once, as dvp_prove / dvp_prove_be32 / dvp_prove_ark do, and run on the prover's own stream. */
int dvp_prove_multi_dev(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const void* d_assignment, uint8_t* proofs /* n_slots x 118 */,
                        int32_t* status /* n_slots */, void* stream);
int dvp_prove_multi(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint64_t* public_inputs, uint32_t n_public,
                    const uint64_t* private_inputs, uint32_t n_private, uint8_t* proofs, int32_t* status);
int dvp_prove_multi_be32(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint8_t* witness_be32, size_t n, uint8_t* proofs,
                         int32_t* status);
int dvp_prove_multi_ark(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint64_t* public_ark, uint32_t n_public,
                        const uint64_t* private_ark, uint32_t n_private, uint8_t* proofs, int32_t* status);

/* Explain an unsatisfied witness.  dvp_prove answers a witness that does not fit the circuit with DVP_EUNSAT and the smallest failing
 * row (the reference's assert, src/proving.rs:389-395); the check says how many rows fail, lists the first ones with their values,
 * counts the entries that are not below p, and names the wires that occur in failing rows only.  It runs on the device over the
 * prover's resident matrices and needs the coefficients and all three matrices and no SRS (as dvp_prover_circuit_hash).
 *
 * The assignment is [1, public.., private..], n_wires elements of any 256-bit value.  An entry >= p is not refused: it is counted
 * (n_noncanonical, first_noncanonical) and every row is evaluated on the entries reduced mod p, so the report is defined for any input;
 * constant_wire_is_one says whether entry 0 reduces to 1.
 *   rows: n_unsat = the number of rows r < m with a*b != C w, the predicate and the arithmetic of dvp_prove, so first_unsat is the
 *     index DVP_EUNSAT carries (-1 when none); padding rows evaluate to zero and are satisfied.  The first rows_cap failing rows come
 *     back in increasing row order as {row, a, b, c, i}, canonical, with c = C w - i(d_row) and i = sum_j pub_j d_row^j (the
 *     reference's c_vals / i_vals), so a*b != c + i holds for each.
 *   wires: a suspect wire has at least one term of A, B or C (as the dump holds them, without the Vandermonde terms) in a failing row
 *     and none in a satisfied row.  n_suspect_wires is exact; the first wires_cap of them come back in increasing wire index as
 *     {wire, n_terms}.  One corrupted wire shows up here; the honest wires that share its rows mostly do not.
 * Both lists are compactions by rank: a truncated list holds the same records in the same order on every run.
 *
 * Returns DVP_OK whenever the check ran -- the answer is in the report, an unsatisfied witness is not an error status here.
 * DVP_EINVAL, before any device work: a NULL prover / report / assignment, a NULL array with a non-zero cap (cap 0 with NULL gives
 * the counts alone), a prover without coefficients or matrices, and the count rules of dvp_prove (dvp_prover_check_witness) and of
 * dvp_prove_be32 (_be32: n < n_wires; a longer buffer is truncated).  rows and wires are HOST arrays in every flavour.
 *   _dev: the assignment (little-endian limbs) is on the device; enqueues on `stream` and waits for the result -- once for a
 *     satisfying witness; for an unsatisfied one the listing and the per-term pass run behind the host's look at the count, and the
 *     call waits a second time.  The per-term pass never runs for a satisfying witness.
 *   dvp_prover_check_witness / _be32: dvp_prove's / dvp_prove_be32's arguments, staged on the prover's own stream; the limb flavour
 *     writes the constant wire itself, the be32 flavour reports element 0 as it finds it.
 * The check borrows the prover's per-proof buffers (which hold nothing between proofs) and allocates its scratch in stream order:
 * m/8 + 4 m/256 bytes for the rows, 8 bytes per wire when rows fail, plus the listed records.  Call it between proofs, not beside a
 * proof on the same handle; proofs made afterwards are byte for byte what they were. */
typedef struct dvp_unsat_row {
  uint64_t row;
  uint64_t a[4], b[4], c[4], i[4];
} dvp_unsat_row;
typedef struct dvp_suspect_wire {
  uint32_t wire, n_terms;
} dvp_suspect_wire;
typedef struct dvp_witness_report {
  uint64_t n_unsat;
  int64_t first_unsat; /* -1 when none */
  uint64_t n_noncanonical;
  int64_t first_noncanonical; /* -1 when none */
  uint64_t n_suspect_wires;
  uint32_t n_rows_listed, n_wires_listed, constant_wire_is_one;
} dvp_witness_report;
int dvp_prover_check_witness_dev(dvp_prover* p, const void* d_assignment, dvp_unsat_row* rows, size_t rows_cap, dvp_suspect_wire* wires,
                                 size_t wires_cap, dvp_witness_report* report, void* stream);
int dvp_prover_check_witness(dvp_prover* p, const uint64_t* public_inputs, uint32_t n_public, const uint64_t* private_inputs,
                             uint32_t n_private, dvp_unsat_row* rows, size_t rows_cap, dvp_suspect_wire* wires, size_t wires_cap,
                             dvp_witness_report* report);
int dvp_prover_check_witness_be32(dvp_prover* p, const uint8_t* witness_be32, size_t n, dvp_unsat_row* rows, size_t rows_cap,
                                  dvp_suspect_wire* wires, size_t wires_cap, dvp_witness_report* report);
/* One row's (wire_id, coeff_id) terms of A / B / C (which = 0 / 1 / 2) out of the resident CSR, so that a host can print a failing row
 * without the dump.  *n = the row's term count, of which the first min(cap, *n) are written; a padding row (n_rows <= row < m) gives
 * *n = 0.  row >= m, a bad `which`, a NULL n, NULL arrays with a non-zero cap or a matrix that was never set: DVP_EINVAL, without a
 * device call. */
int dvp_prover_row_terms(dvp_prover* p, int which, uint32_t row, uint32_t* wire_ids, uint32_t* coeff_ids, size_t cap, size_t* n);

/* prove in phases, so that the two MSMs -- the only stages that shard across GPUs -- can be split by
 * index range and their partial sums combined by the caller (all-gather + local add):
 *   begin -> msm_partial(0, lo, hi) -> challenge(commit point) -> msm_partial(1, lo, hi) -> finish */
int dvp_prove_begin(dvp_prover* p, const void* d_assignment, void* stream);
/* begin for a rank whose MSM shards need neither q2 nor r2 (they lie inside [w] and [k_a | k_b]): need_extend = 0
 * skips the extends and the quotient; need_extend != 0 is dvp_prove_begin */
int dvp_prove_begin_partial(dvp_prover* p, const void* d_assignment, int need_extend, void* stream);
/* The extends by VECTOR: the extends of a, b, c' (and i, unless it is evaluated by Horner: dvp_prover_extend_count
 * says 3 or 4) are independent (src/proving.rs:410-422).  After dvp_prove_begin_partial(need_extend = 0) a rank extends only
 * the vectors of `mask` (bit v = vector v of [a, b, c', i]), the ranks that need q2 / r2 exchange the extended vectors --
 * dvp_prover_extended_ptr(v) is the device address of vector v (m canonical Fr) to send from / receive into -- and
 * dvp_prove_quotient then forms r2 and q2 (src/proving.rs:492-508).  begin_partial(need_extend = 1) is exactly
 * begin_partial(0) + dvp_prove_extend_vectors(all) + dvp_prove_quotient. */
uint32_t dvp_prover_extend_count(const dvp_prover* p);
int dvp_prove_extend_vectors(dvp_prover* p, uint32_t mask, void* stream);
int dvp_prover_extended_ptr(dvp_prover* p, uint32_t v, void** d_ptr);
/* vector v of the current proof has been written into dvp_prover_extended_ptr(v) by the caller (received from the rank that
 * extended it).  dvp_prove_quotient returns DVP_EINVAL unless every vector was either extended here or marked since the
 * last begin: a missed exchange cannot turn into a silently wrong q2. */
int dvp_prove_mark_extended(dvp_prover* p, uint32_t v);
int dvp_prove_quotient(dvp_prover* p, void* stream);
size_t dvp_prover_msm_size(const dvp_prover* p, int which);
/* window bits / window count chosen for MSM `which` (0,0 until its fixed-base tables exist) */
int dvp_prover_msm_plan(const dvp_prover* p, int which, int* c_bits, int* windows);
/* HBM held by the fixed-base tables of MSM `which` on all devices (see dvp_msm_ctx_table_bytes): what is actually allocated now --
 * 0 before the first proof, and never more per device than dvp_prover_set_table_budget allows */
uint64_t dvp_prover_msm_table_bytes(const dvp_prover* p, int which, int* signed_windows);
/* The most HBM per device the fixed-base tables of this prover (both MSMs together) may hold.  UINT64_MAX = no limit (the default);
 * 0 = no tables.  New provers, those of dvp_prove_cache_dir included, start from DVP_TABLE_BUDGET_BYTES in the environment (read
 * once).  May be called at any time between proofs: tables that no longer fit are released at once, and the next proof follows the
 * new plan.  The plan is deterministic: MSM 1 ([k_a | k_b | k_r], 4m terms) is served first, then MSM 0; at most one of the two is
 * partly covered, by a table over a PREFIX [0, covered) of its bases -- the rest of that sum runs through the one-shot MSM and one
 * point addition joins the two; a prefix shorter than DVP_MSM_FIXED_MIN gets no table.  Proof bytes do not depend on the budget.
 * With dvp_set_devices the budget of a device is split evenly among the shards that name it, and a shard's table is all or
 * nothing per MSM.  A table the runtime refuses although the budget allows it is not an error either: that MSM runs one-shot
 * (dvp_prover_msm_coverage: reason 2) and the allocation is tried again only after the next call of this function. */
int dvp_prover_set_table_budget(dvp_prover* p, uint64_t bytes);
/* *covered = leading bases of MSM `which` served from tables on the home device (with dvp_set_devices: by the leading shards that
 * hold one), *total = dvp_prover_msm_size, *reason = 0 not limited (everything DVP_MSM_FIXED_MIN lets into a table is in one),
 * 1 limited by the budget, 2 an allocation was refused by the runtime.  Before the first proof this is the plan, not zeros. */
int dvp_prover_msm_coverage(const dvp_prover* p, int which, size_t* covered, size_t* total, int* reason);
int dvp_prover_msm_partial(dvp_prover* p, int which, size_t lo, size_t hi, void* d_out_xy, void* d_out_inf, void* stream);
int dvp_prove_challenge(dvp_prover* p, const void* d_commit_xy, const void* d_commit_inf, void* stream);
/* The same phase for provers that share one proof by INDEX (one process per GPU): the pointwise stages, the batch
 * inversions and the barycentric sums (src/proving.rs:561-654) are computed only where this rank needs them.
 * part 1: alpha from the commitment, 1/(d - alpha) on this rank's slice [d_lo, d_hi) of D (its share of the three
 *   barycentric sums) and on the part of D / D' that its K-scalar range [k_lo, k_hi) of [k_a | k_b | k_r] reads;
 *   d_record_out receives a 128-byte record (three partial sums + the rank's alpha-in-domain flag).
 * part 2: d_records = the n records of all ranks (all-gathered, any order; the slices must partition [0, m)):
 *   a0 b0 i0 r0, then the K scalars of [k_lo, k_hi) only -- the only range dvp_prover_msm_partial(1, ..) may then cover. */
int dvp_prove_challenge_partial(dvp_prover* p, const void* d_commit_xy, const void* d_commit_inf, size_t d_lo, size_t d_hi,
                                size_t k_lo, size_t k_hi, void* d_record_out, void* stream);
int dvp_prove_challenge_finish(dvp_prover* p, const void* d_records, uint32_t n_records, size_t k_lo, size_t k_hi, void* stream);
int dvp_prove_finish(dvp_prover* p, const void* d_kzg_xy, const void* d_kzg_inf, uint8_t proof[118], void* stream);
/* (D, D') = get_both_domains(tree2n), src/ec_fft.rs:179-189 */
int dvp_prover_domains(dvp_prover* p, uint64_t* d, uint64_t* d2);
/* which = 0: (1/Z_D'(D_i), 1/Z_D(D'_i)) = (bar_wts, z_vals2inv); which = 1: the D' mirrors
 * (bar_wtsd, z_vals2d_inv) -- compute_barycentric_weights / prepare_z_inv, src/srs.rs:267-311 */
int dvp_prover_domain_tables(dvp_prover* p, int which, uint64_t* bar_weights, uint64_t* zinv_other);

/* the same tables from a stand-alone 2m-leaf tree (TREE_2N): bar_weights[m], zinv_other[m], canonical */
int dvp_ecfft_domain_tables(dvp_ecfft* tree2n, int which, uint64_t* bar_weights, uint64_t* zinv_other);

/* Transcript::output, src/proving.rs:164-197, and the BLAKE3 hash it is built on */
int dvp_transcript_challenge(const uint8_t commit_p[30], const uint64_t* public_inputs, uint32_t n_public, uint64_t out[4]);
int dvp_blake3(const uint8_t* data, size_t len, uint8_t out[32]);
/* BLAKE3 of a DEVICE buffer, chunk-parallel: one lane per 1 KiB chunk, then the chaining values pairwise, nine levels per launch
 * (csrc/blake3_tree.hip).  d_data may start at any byte address (nothing at or beyond d_data + len is read; up to three bytes in front
 * of it are, the aligned dword its first byte lies in) and may be NULL only for len = 0; d_out32: 32 bytes on the device.  Enqueues on
 * `stream` and does not wait; its scratch (len / 32 bytes of chaining values) is allocated and freed in stream order.  DVP_ENOMEM only
 * when the runtime refuses that scratch; len > 2^40 is DVP_EINVAL (32-bit chunk counter). */
int dvp_blake3_dev(const void* d_data, size_t len, void* d_out32, void* stream);

/* Binding the transcript to the SRS and the circuit.  Transcript::srs_hash and ::circuit_info_hash (src/proving.rs:82-134) hash EMPTY
 * buffers in the reference ("takes awfully long to hash this much data"), so a proof's challenge binds neither; that stays the default
 * here, byte for byte.  On this device the SRS hash is milliseconds, so a host may opt in: the compile-time half of the transcript
 * becomes H(srs_hash || circuit_hash), a NULL hash meaning BLAKE3("") (NULL, NULL = the reference's constant).  Prover and verifier
 * must be given the same pair: a proof made under one binding fails under any other with DVP_VERIFY_EQUATION.
 *
 * dvp_prover_srs_hash: BLAKE3 of the stream the commented-out loop at src/proving.rs:91-101 would build -- to_bytes() of every point of
 * g_k[0], g_k[1], g_k[2], then g_q, then g_m, i.e. the payloads of the files g_k_0, g_k_1, g_k_2, g_q, g_m in that order without their
 * 8-byte counts -- encoded and hashed on the device through a bounded staging window.  It DEPENDS ON THE CODEC RULE IN FORCE
 * (dvp_codec_set_rule): the same bases hash differently under another rule.  DVP_EINVAL until all five SRS vectors are set.  Under
 * dvp_set_devices the home device's copies are hashed (they stay complete), so the device list does not change the result.  Waits
 * for the result; call it between proofs.
 * dvp_prover_set_transcript_binding: may be called between proofs; every path that derives alpha follows it (dvp_prove, dvp_prove_dev
 * with the device or the host transcript, device lists, dvp_prove_challenge, dvp_prove_challenge_partial).  The circuit hash may be
 * dvp_prover_circuit_hash (below) or any 32 bytes a host defines: dvp_blake3 / dvp_blake3_dev hash whatever a host decides on.
 * dvp_transcript_challenge_bound: dvp_transcript_challenge under a binding (host only).
 *
 * dvp_prover_circuit_hash: BLAKE3 of the stream the commented-out body of Transcript::circuit_info_hash would build
 * (src/proving.rs:111-134) on the instance Proof::prove hands it, i.e. after update_to_include_vandermode_matrix_d
 * (src/gnark_r1cs.rs:333-386).  With m constraints, k public inputs, the coefficient table c[0, n0) and d_i the i-th element of D:
 * i1 = the first index with c[i1] == p - 1, or n0 with p - 1 appended when there is none (for k = 0 as well); n1 = the table's length
 * then; the updated table is c[0, n1) followed by -(d_i^j) mod p at index n1 + i (k - 1) + (j - 1) for i in [0, m), j in [1, k): N
 * entries.  The stream is, for i = 0 .. m - 1, the coeff_ids of row i of A, of B and of C, then (k >= 1) i1, then the ids
 * n1 + i (k - 1) + (j - 1) for j = 1 .. k - 1, each a u32 little-endian (:130 hashes the rows first); then the table as
 * Vec<Fr>::serialize_uncompressed: N as u64 little-endian and every entry as 29 bytes little-endian canonical, the payload layout of
 * the Fr vector files.  WIRE IDS ARE NOT PART OF IT, because the reference wrote only the coeff_ids; the SRS hash depends on the
 * wiring through g_m.  Generated and hashed on the device through a bounded staging window (DVP_CIRCUIT_HASH_WINDOW); nothing of the
 * stream reaches the host.  Needs the coefficients and all three matrices (DVP_EINVAL otherwise, and when a stored coefficient id lies
 * outside the table, as dvp_prove would answer) and no SRS; N > 2^32 is DVP_EINVAL (the reference's `as u32` would wrap silently).
 * Waits for the result; call it between proofs, not beside a proof on the same handle. */
int dvp_prover_circuit_hash(dvp_prover* p, uint8_t out[32]);
int dvp_prover_srs_hash(dvp_prover* p, uint8_t out[32]);
int dvp_prover_set_transcript_binding(dvp_prover* p, const uint8_t srs_hash[32], const uint8_t circuit_hash[32]);
int dvp_transcript_challenge_bound(const uint8_t commit_p[30], const uint64_t* public_inputs, uint32_t n_public,
                                   const uint8_t srs_hash[32], const uint8_t circuit_hash[32], uint64_t out[4]);
/* The verifier's side: process-wide like dvp_codec_set_rule; every dvp_verify* entry reads it once per call (a call in flight keeps
 * the value it started with).  NULL, NULL restores the default.  The seed-less key of dvp_verify_batch_rlc does not change (it covers
 * the proof bytes already).  get: the pair in force, BLAKE3("") for a hash that is not set. */
int dvp_verify_set_binding(const uint8_t srs_hash[32], const uint8_t circuit_hash[32]);
int dvp_verify_get_binding(uint8_t srs_hash[32], uint8_t circuit_hash[32]);

/* SRS::verify(secrets, public_inputs, proof) (src/srs.rs:374-428) on the GPU: the designated verifier's check, one lane per proof,
 * sharing the codec (dvp_codec_set_rule), the transcript and the curve code with the prover.  Proof bytes: Proof::to_bytes,
 * commit_p[30] | kzg_k[30] | a0[29] | b0[29].  A proof is accepted (verdict 0) exactly when the reference returns true; otherwise
 * the verdict is an OR of DVP_VERIFY_* bits: the reference's four validity flags, a non-canonical public input (the _dev flavour
 * only), and DVP_VERIFY_EQUATION, set only when every input was valid and v0 K + u0 G != P.  Bad proof bytes never give an error
 * status.  tau, delta, epsilon: canonical host values (>= p: DVP_EINVAL; zero is allowed, as in the reference).  The host
 * flavours reject a non-canonical public input with DVP_EINVAL, dvp_last_error_index() = its flat index.  n_public <=
 * DVP_VERIFY_MAX_PUBLIC (hashed on the device, multi-chunk beyond 35); n = 0 is DVP_OK. */
#define DVP_VERIFY_BAD_COMMIT_P 0x01u
#define DVP_VERIFY_BAD_KZG_K 0x02u
#define DVP_VERIFY_BAD_A0 0x04u
#define DVP_VERIFY_BAD_B0 0x08u
#define DVP_VERIFY_BAD_PUBLIC 0x10u
#define DVP_VERIFY_EQUATION 0x20u
#define DVP_VERIFY_MAX_PUBLIC 8192u
/* one proof: *accepted = 1 / 0, *reasons (optional) = DVP_VERIFY_* bits */
int dvp_verify(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
               uint32_t n_public, const uint8_t proof[118], int* accepted, uint32_t* reasons);
/* n proofs (n x 118 B) against one trapdoor; public_inputs: n x n_public canonical Fr (row i for proof i); verdicts: n bytes */
int dvp_verify_batch(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                     uint32_t n_public, const uint8_t* proofs, size_t n, uint8_t* verdicts);
/* the same on device buffers, enqueued on `stream` on the current device (one kernel launch once the generator table of the
 * device exists; the first call on a device builds it and waits for it).  A non-canonical public input is the verdict bit
 * DVP_VERIFY_BAD_PUBLIC of its proof. */
int dvp_verify_batch_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                         uint32_t n_public, const void* d_proofs, size_t n, void* d_verdicts, void* stream);
/* Batch verification by ONE random linear combination: the arguments, verdicts and errors of dvp_verify_batch(_dev), plus `seed`
 * and a report word.  Each proof j is decoded and range-checked as there; a proof with a validity flag gets the same bits and is
 * left out.  The well-formed proofs W are checked together by one multi-scalar multiplication of 2n + 1 points:
 *     sum_W (r_j v0_j) K_j + sum_W (p - r_j) P_j + (sum_W r_j u0_j) G == O,
 *     r_j = (first 16 bytes of BLAKE3(key || LE64(j) || proof_j[0..118) || H_pub_j), read little-endian) | 2^127,
 * H_pub_j = BLAKE3 of proof j's public inputs as 29 little-endian bytes each (the transcript's digest).  key = seed (32 bytes), or
 * for seed == NULL key = BLAKE3("dv-pari verify rlc v1" || tau || delta || epsilon), each as 32 little-endian bytes: deterministic,
 * and secret as long as the trapdoor is.  If the sum is O, every proof in W gets verdict 0 (report DVP_VERIFY_RLC_COMBINED).
 * Otherwise the per-lane check of dvp_verify_batch runs over the whole batch and its verdicts are returned (report
 * DVP_VERIFY_RLC_FALLBACK): a batch with a bad proof costs the combined check plus the per-lane check.  With no well-formed proof
 * neither bit is set.  The verdicts differ from dvp_verify_batch's only if the sum is O while some proof of W fails its own
 * equation: at most 2^-127 per call (BLAKE3 read as a random oracle; fix every coefficient but one -- at most one value mod p of
 * the last cancels the error, and it takes 2^127 values).  n <= DVP_VERIFY_RLC_MAX_PROOFS (the one-shot MSM's 2^27 points);
 * larger n is DVP_EINVAL.  Measured on one MI355X (tools/README.md): faster than dvp_verify_batch_dev at every size measured, one
 * proof (0.46 against 4.4 ms) to 2^20 (10.4 against 117 ms), so there is no crossover; a 2^16 batch with one bad proof takes
 * 9.0 ms against 7.3 ms. */
#define DVP_VERIFY_RLC_COMBINED 0x1u
#define DVP_VERIFY_RLC_FALLBACK 0x2u
#define DVP_VERIFY_RLC_MAX_PROOFS ((1u << 26) - 1u)
int dvp_verify_batch_rlc(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                         uint32_t n_public, const uint8_t* proofs, size_t n, const uint8_t seed[32] /* NULL: key from the trapdoor */,
                         uint8_t* verdicts, uint32_t* report /* optional */);
/* the same on device buffers, enqueued on `stream`; d_report (optional): one u32 on the device.  Nothing waits on the host: the
 * per-lane launch is always enqueued and ends at once when the combined check held.  Two host threads may verify on one device at
 * the same time. */
int dvp_verify_batch_rlc_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                             uint32_t n_public, const void* d_proofs, size_t n, const uint8_t seed[32], void* d_verdicts,
                             void* d_report /* optional u32 */, void* stream);

/* Accepted proofs from the trapdoor alone, without a circuit, an SRS or a witness (test vectors for a verifier, distinct proofs for a
 * benchmark): for proof j the discrete logs are chosen and the verifier's equation is solved for them, one lane per proof, one kernel
 * launch per call once the generator table of the device exists.  Deterministic:
 *   key        = seed (32 bytes), or for seed == NULL BLAKE3("dv-pari simulate v1" || tau || delta || epsilon), each as 32 LE bytes
 *   draw(j, g) = the first 29 bytes of BLAKE3(key || LE64(index_base + j) || g), g one byte, read little-endian, masked to 230 bits
 *   p = draw(j, 1), or 1 if that is 0;  b0 = draw(j, 2) unless the caller gives b0;  t = draw(j, 3)
 *   the case:    P_ZERO p = 0;  T_HALF t = p / 2;  U0_ZERO t = 0;  K_ZERO t = p
 *   commit_p   = enc(p G) under the codec rule in force;  alpha = the verifier's transcript over commit_p and row j of the public
 *                inputs under the binding dvp_verify_set_binding holds;  v0 = (tau - alpha) epsilon;  v0 = 0: status DVP_SIM_V0_ZERO
 *   the case:    K_PLUS_G t = p - v0;  K_MINUS_G t = p + v0
 *   kzg_k      = enc(k G), k = (p - t) / v0;  i0 = sum_i pub_i alpha^i;  if 1 + delta^2 b0 = 0 then b0 := b0 + 1;
 *   a0         = (t / epsilon - delta b0 + delta^2 i0) / (1 + delta^2 b0)
 *   proof j    = commit_p[30] | kzg_k[30] | a0 as 29 LE bytes | b0 as 29 LE bytes
 * so that u0 = t and v0 K + u0 G = (p - t) G + t G = P: dvp_verify_batch accepts every proof with status DVP_SIM_OK, under the
 * trapdoor, public inputs, binding and codec rule it was made with.  The cases reach the exceptional branches of the verifier's
 * addition chain.  dlogs (optional): p then k per proof, canonical.  A proof with a nonzero status is 118 zero bytes and its
 * discrete logs are zero.  DVP_EINVAL before any device work: a trapdoor element >= p, epsilon = 0 (u0 = v0 = 0 leaves nothing to
 * solve), n_public > DVP_VERIFY_MAX_PUBLIC, a NULL required pointer, and in the host flavour a non-canonical public input
 * (dvp_last_error_index() = its flat index), a case byte > 6 or a non-canonical b0 (= the proof's index).  n = 0 is DVP_OK and
 * touches nothing. */
#define DVP_SIM_GENERIC 0   /* P, b0, u0 drawn from the key */
#define DVP_SIM_T_HALF 1    /* u0 = p/2: v0 K == u0 G, the final addition is a doubling */
#define DVP_SIM_P_ZERO 2    /* P = O: v0 K == -u0 G */
#define DVP_SIM_U0_ZERO 3
#define DVP_SIM_K_PLUS_G 4  /* K = G */
#define DVP_SIM_K_MINUS_G 5 /* K = -G */
#define DVP_SIM_K_ZERO 6    /* K = O */
#define DVP_SIM_OK 0x00u
#define DVP_SIM_V0_ZERO 0x01u    /* alpha == tau: no K exists for this P; the 118 bytes are zero */
#define DVP_SIM_BAD_PUBLIC 0x02u /* _dev only */
#define DVP_SIM_BAD_CASE 0x04u   /* _dev only */
#define DVP_SIM_BAD_B0 0x08u     /* _dev only */
int dvp_simulate_batch(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4],
                       const uint64_t* public_inputs /* n x n_public x 4 */, uint32_t n_public, size_t n,
                       const uint8_t seed[32] /* NULL: key from the trapdoor */, uint64_t index_base,
                       const uint8_t* cases /* n bytes, NULL = all generic */, const uint64_t* b0 /* n x 4, NULL = drawn */,
                       uint8_t* proofs /* n x 118 */, uint8_t* status /* n */, uint64_t* dlogs /* optional, n x 8: p then k */);
/* the same on device buffers, enqueued on `stream` on the current device; only the first call on a device waits (it builds the
 * generator table).  The three input faults are status bits of their proof here, which is then zero bytes; its neighbours are
 * not affected. */
int dvp_simulate_batch_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                           uint32_t n_public, size_t n, const uint8_t seed[32], uint64_t index_base, const void* d_cases,
                           const void* d_b0, void* d_proofs, void* d_status, void* d_dlogs /* optional */, void* stream);

/* The stage values of SRS::verify per proof, for whoever has to find where a prover and a verifier part (or writes this verifier a
 * second time): the arguments and errors of dvp_verify_batch(_dev) with one record per proof in place of the verdict byte.
 * `verdict` is exactly dvp_verify_batch's byte.  With a validity bit set every other field is zero.  Otherwise the record holds the
 * transcript challenge alpha, i0 = sum_i pub_i alpha^i, r0 = a0 b0 - i0, u0 and v0 (canonical limbs), the decoded commit_p and
 * kzg_k, and v0 K, u0 G and their sum, every point in the affine form used everywhere in this header (x then y), a point at infinity
 * with zero coordinates and its flag set; DVP_VERIFY_EQUATION is set exactly when (sum_inf, sum_xy) != (p_inf, p_xy). */
typedef struct dvp_verify_trace {
  uint64_t alpha[4], i0[4], r0[4], u0[4], v0[4]; /* canonical limbs */
  uint64_t p_xy[8], k_xy[8];                     /* decoded commit_p, kzg_k */
  uint64_t vk_xy[8], ug_xy[8], sum_xy[8];        /* v0 K, u0 G, v0 K + u0 G */
  uint8_t p_inf, k_inf, vk_inf, ug_inf, sum_inf, verdict, pad[2];
} dvp_verify_trace;
#ifdef __cplusplus
static_assert(sizeof(dvp_verify_trace) == 488, "dvp_verify_trace is 488 bytes");
#else
_Static_assert(sizeof(dvp_verify_trace) == 488, "dvp_verify_trace is 488 bytes");
#endif
int dvp_verify_trace_batch(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const uint64_t* public_inputs,
                           uint32_t n_public, const uint8_t* proofs, size_t n, dvp_verify_trace* out);
/* the same on device buffers (d_out: n x 488 bytes), enqueued on `stream`; a non-canonical public input is DVP_VERIFY_BAD_PUBLIC */
int dvp_verify_trace_batch_dev(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const void* d_public_inputs,
                               uint32_t n_public, const void* d_proofs, size_t n, void* d_out, void* stream);
/* sp1_generate_scalar_from_raw_public_input (src/gnark_r1cs.rs:214-229), host only: BLAKE3 of the 8-byte LE raw value, digest
 * bytes 0..3 cleared, read big-endian (< 2^224, canonical) */
int dvp_sp1_public_input(uint64_t raw, uint64_t out[4]);

/* BLAKE3 of an Fr vector in the reference's serialisation, Vec<Fr>::serialize_uncompressed: n as u64 little-endian, then every entry
 * as 29 bytes little-endian canonical -- byte for byte the file dvp_file_fr_vec_write writes, so one blake3::hash per Vec<Fr> on the
 * Rust side compares a whole vector.  n = 0 hashes the 8 count bytes.  The stream is never materialised: it is packed on the device
 * from the 32-byte entries into a bounded window of whole 1 KiB chunks (DVP_FR_DIGEST_WINDOW of them, 61440 = 60 MiB by default, never
 * more than the stream needs) and hashed chunk-parallel as dvp_blake3_dev hashes; device scratch = that window + 32 bytes per chunk.
 * Host entry: limbs = n x 4 u64 canonical; an entry >= p is DVP_EINVAL with dvp_last_error_index() = its index. */
int dvp_fr_vec_digest(const uint64_t* limbs, size_t n, uint8_t out[32]);
/* the same over n x 32 bytes on the device, enqueued on `stream` (scratch comes from and returns to the stream's pool; nothing waits).
 * montgomery != 0: the entries are a R mod p and are converted on their way into the stream.  Nothing is range-checked: the low 29
 * bytes of every (converted) entry are hashed as they are.  d_out32: 32 bytes on the device. */
int dvp_fr_vec_digest_dev(const void* d_fr, size_t n, int montgomery, void* d_out32, void* stream);

/* The stages of a prover's LAST proof, the mirror of dvp_verify_trace for Proof::prove (src/proving.rs:426-688): when the 118 bytes of
 * this library and of the reference differ, the record says at which stage they part.  Nothing on the proof path produces it: the call
 * reads what a completed proof leaves resident in the prover.
 *   header   log2_m, n_wires, n_public, the codec rule in force (dvp_codec_get_rule), parts as delivered, mismatch
 *   scalars  (DVP_TRACE_SCALARS) canonical limbs: the challenge alpha, z_alpha = Z_D(alpha), a0, b0, i0, r0
 *   points   (DVP_TRACE_POINTS) msm_gm = <assignment, g_m>, msm_q = <q_vals2, g_q>, commit_p; kzg_a = <k_scalar_a, g_k_0>, kzg_b =
 *            <k_scalar_b, g_k_1>, kzg_r = <k_scalar_r, g_k_2>, kzg_k.  commit_p and kzg_k are the proof's own (their encodings are its
 *            bytes 0..59); the five partial commitments are computed now, through the one-shot MSM (dvp_msm_affine_dev's path) over
 *            sub-ranges of the resident bases and scalars -- never through the fixed-base tables, so no table is built and no budget
 *            touched, and the table path is checked against an independent one: mismatch bit 0 = commit_p != msm_gm + msm_q, bit 1 =
 *            kzg_k != kzg_a + kzg_b + kzg_r, both sums taken on the device with the complete addition.
 *   digests  (DVP_TRACE_DIGESTS) dvp_fr_vec_digest_dev of every intermediate vector under the name src/proving.rs gives it:
 *            assignment (n_wires entries), evals.a/b/c/i on D and evals2.a/b/c/i on D' (m each; c is the matrix C with the Vandermonde
 *            fold, as the reference's updated instance has it; evals2.i is in place on the Horner route too, written by the quotient
 *            kernel), r_vals2, q_vals2, denom_invs, denom_invs2, k_scalar_a, k_scalar_b (m each), k_scalar_r (2m, interleaved
 *            [D_i, D'_i] as :644-654).  r_vals on D is never materialised here (the K scalars fold it in) and is not part of the record.
 * A part that was not asked for is zero.  Valid only while the prover holds a COMPLETE proof: dvp_prove / _dev / _be32 / _ark /
 * _cache_dir* and dvp_prove_finish (behind a full begin and dvp_prove_challenge) mark it on success, every begin clears it; DVP_EINVAL
 * before the first proof, after any proof that returned an error (DVP_EUNSAT, DVP_ECHALLENGE, ..), after dvp_prove_challenge_partial /
 * an extend-free begin (their vectors are partial), after any call since the proof that overwrote what it left -- a staged phase entry,
 * dvp_prover_check_witness* (it reduces its argument into the assignment's buffer; also through dvp_check_witness_cache_dir_witness_file
 * on an open prover), dvp_prover_set_srs_* (the commitments are no longer sums over the resident bases) --, after a
 * dvp_codec_set_rule to another rule than the proof's (its two encodings and the five made now would disagree; codec_rule in the
 * header is the one rule of all seven), for parts == 0 or unknown bits, and under dvp_set_devices with more than one device (the
 * sharded prover is out of scope).  The call runs on `stream`, waits for it, changes nothing a later proof reads, and two
 * traces of one proof are identical.  It costs more than the proof: five one-shot MSMs and about 17 m x 29 bytes of hashing. */
#define DVP_TRACE_SCALARS 0x1u
#define DVP_TRACE_DIGESTS 0x2u
#define DVP_TRACE_POINTS 0x4u
#define DVP_TRACE_ALL 0x7u
#define DVP_TRACE_MISMATCH_COMMIT 0x1u /* commit_p != msm_gm + msm_q */
#define DVP_TRACE_MISMATCH_KZG 0x2u    /* kzg_k != kzg_a + kzg_b + kzg_r */
typedef struct dvp_trace_point {
  uint64_t xy[8];  /* affine x then y; zero for the point at infinity */
  uint8_t enc[30]; /* under the codec rule of the header */
  uint8_t inf, pad;
} dvp_trace_point;
typedef struct dvp_prove_trace {
  uint32_t log2_m, n_wires, n_public, codec_rule, parts, mismatch;
  uint64_t alpha[4], z_alpha[4], a0[4], b0[4], i0[4], r0[4];
  dvp_trace_point msm_gm, msm_q, commit_p, kzg_a, kzg_b, kzg_r, kzg_k;
  uint8_t assignment[32], evals_a[32], evals_b[32], evals_c[32], evals_i[32], evals2_a[32], evals2_b[32], evals2_c[32], evals2_i[32],
      r_vals2[32], q_vals2[32], denom_invs[32], denom_invs2[32], k_scalar_a[32], k_scalar_b[32], k_scalar_r[32];
} dvp_prove_trace;
#ifdef __cplusplus
static_assert(sizeof(dvp_trace_point) == 96 && sizeof(dvp_prove_trace) == 1400, "dvp_prove_trace is 1400 bytes");
#else
_Static_assert(sizeof(dvp_trace_point) == 96 && sizeof(dvp_prove_trace) == 1400, "dvp_prove_trace is 1400 bytes");
#endif
int dvp_prover_trace_last(dvp_prover* p, uint32_t parts, dvp_prove_trace* out, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* cache_dir formats: the files the reference's setup / prover exchange.          */
/* Host-only code; the counted readers take out == NULL to query the element count.            */
/* ------------------------------------------------------------------------------------------ */
/* u64-LE n || n x 29 B canonical LE: write_fr_vec_to_file / read_fr_vec_from_file, src/io_utils.rs:42-70,122-179 */
int dvp_file_fr_vec_write(const char* path, const uint64_t* limbs, size_t n);
int dvp_file_fr_vec_read(const char* path, uint64_t* out, size_t cap, size_t* n);
/* u64-LE n || n x 30 B: write_point_vec_to_file / read_point_vec_from_file, src/io_utils.rs:83-111,187-239 */
int dvp_file_point_vec_write(const char* path, const uint8_t* enc, size_t n);
int dvp_file_point_vec_read(const char* path, uint8_t* out, size_t cap, size_t* n);
/* u32-BE n || n x 32 B big-endian, reduced mod p: load_witness_from_file, src/gnark_r1cs.rs:58-77,188-210 */
int dvp_file_witness_read(const char* path, uint64_t* out, size_t cap, size_t* n);
int dvp_file_witness_write(const char* path, const uint64_t* limbs, size_t n);
/* gnark/SP1 sparse R1CS dump (src/gnark_r1cs.rs:84-91,121-185) -> coefficient table (from_be_bytes_mod_order,
 * :282-289) + L/R/O as CSR.  n_wires = max wire id + 1 (accumulate_m_values, src/srs.rs:56-62).  Two calls: sizes,
 * then fill caller-allocated arrays (row_ptr[k]: n_rows+1, wire[k]/coeff_id[k]: nnz[k]). */
int dvp_r1cs_dump_sizes(const uint8_t* buf, size_t len, uint32_t* n_coeffs, uint32_t* n_rows, uint64_t nnz[3], uint32_t* n_wires);
int dvp_r1cs_dump_fill(const uint8_t* buf, size_t len, uint64_t* coeffs, uint32_t* const row_ptr[3], uint32_t* const wire[3],
                       uint32_t* const coeff_id[3]);
/* FFTR tree files (src/tree_io.rs:1-15,144-214,353-433): the sectioned container the reference stores its FFTrees in.
 * The prover never needs one (twiddles are regenerated from the curve constants); these entries let a host CHECK a
 * reference-built tree2n / treen against the regenerated domain and write files in the same container.  depth = number
 * of subtree links (section 12) to follow from the root node.  Blob layout assumed: ark-serialize Vec of field elements,
 * u64-LE count || count x 29-byte LE canonical (Mat2x2 = 4 elements); anything else is DVP_EIO (csrc/tree_io.cpp). */
int dvp_fftr_sections(const char* path, uint32_t depth, uint8_t ids[13], uint64_t lens[13], uint32_t* n_sections);
int dvp_fftr_read_fr(const char* path, uint32_t depth, uint8_t section_id, uint64_t* out, size_t cap, size_t* n_elems);
int dvp_fftr_write(const char* path, uint32_t n_sections, const uint8_t* ids, const uint64_t* const* data, const uint64_t* elems);

/* SRS::verifier_runs_setup(trapdoor, cache_dir, num_public_inputs, ..) (src/srs.rs:177-361 -> compute_srs_matrices,
 * src/srs.rs:112-167): reads cache_dir/r1cs_to_dvsnark, computes the five SRS scalar vectors on the device (Lagrange values
 * at tau on D, D' and the unified domain through the barycentric formula, accumulate_m_values over the transposed matrices,
 * the Vandermonde fold on the public wires), multiplies them onto the generator in batches and writes g_m, g_q, g_k_0,
 * g_k_1, g_k_2 as point-vector files (src/io_utils.rs:42-124).  write_precomputes != 0 also writes z_poly, z_polyd, bar_wts,
 * bar_wtsd, z_vals2inv, z_vals2dinv (Fr-vector files, src/artifacts.rs:86-110), so the directory is complete for a
 * reference prover / verifier.  tau, delta, epsilon: canonical, non-zero (src/srs.rs:199-201: DVP_EINVAL otherwise, and when
 * tau lies in an evaluation domain).  The is_fresh_setup / checksum bookkeeping of the reference is not part of this entry. */
int dvp_setup_cache_dir(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const char* cache_dir,
                        uint32_t n_public, int write_precomputes);

/* The audit of an SRS by whoever holds its trapdoor (the verifier after a transfer or a restore, an auditor of an opened instance):
 * are g_m, g_q, g_k_0, g_k_1, g_k_2 in cache_dir the SRS of (tau, delta, epsilon) for cache_dir/r1cs_to_dvsnark and n_public?  The
 * five scalar vectors are computed as dvp_setup_cache_dir computes them; each file is mapped, decoded on the GPU (under the codec rule
 * in force) and handed with its scalars to dvp_points_check_dlog_dev: one combined MSM per vector instead of n_wires + 5m fixed-base
 * multiplications and a file comparison, and a wrong entry is named.  All five vectors are always checked, so one call reports every
 * bad vector.  The files are only read.
 * A missing file, a wrong entry count or an undecodable encoding is that vector's status (with first_bad = the first entry that is
 * missing or surplus / the first bad encoding), not a failure of the call.  The call fails with DVP_EINVAL for a zero trapdoor
 * element or a tau inside an evaluation domain, as the setup does, and with DVP_EIO for an unreadable dump.
 * seed == NULL: vector v is checked under the key BLAKE3("dv-pari srs check v1" || tau || delta || epsilon || LE32(v)), each trapdoor
 * element as 32 little-endian bytes; otherwise under BLAKE3(seed || LE32(v)).  DVP_SRS_CHECK_EXACT = DVP_DLOG_CHECK_EXACT for every
 * vector.  Needs no prover; frees what it allocated (the scalars zeroed first); at most one decoded vector and one workspace are live. */
#define DVP_SRS_CHECK_EXACT 0x1u
#define DVP_SRS_VEC_MISSING 1u   /* the file cannot be opened */
#define DVP_SRS_VEC_LENGTH 2u    /* its entry count is not the expected one, or it is shorter than its count says */
#define DVP_SRS_VEC_DECODE 3u    /* an encoding the decoder rejects */
#define DVP_SRS_VEC_BAD_POINT 4u /* DVP_DLOG_BAD_POINT (the decoder cannot produce one) */
#define DVP_SRS_VEC_WRONG 5u     /* DVP_DLOG_WRONG: well-formed points, not this trapdoor's SRS */
typedef struct dvp_srs_check_report {
  uint32_t verdict;      /* 0 = the directory holds the SRS of (tau, delta, epsilon) for its r1cs dump and n_public; else 1 */
  uint32_t bad_vectors;  /* bit v (0..4 = g_m, g_q, g_k_0, g_k_1, g_k_2): vector v failed */
  uint32_t path[5];      /* per vector: DVP_DLOG_PATH_*, 0 when the vector never reached the check */
  uint32_t status[5];    /* per vector: 0 or DVP_SRS_VEC_* */
  int64_t first_bad[5];  /* per vector: index of its first offending entry, -1 when none */
  uint64_t count[5];     /* entries expected: n_wires, m, m, m, 2m */
} dvp_srs_check_report;
int dvp_srs_check_cache_dir(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const char* cache_dir,
                            uint32_t n_public, const uint8_t* seed /* 32 bytes or NULL */, uint32_t flags, dvp_srs_check_report* report);

/* prover_prepares_precomputes(cache_dir, validate_precompute) (src/proving.rs:225-325): cache_dir/z_poly must exist (its length
 * fixes m; DVP_EIO when it does not, DVP_EINVAL when m is not a power of two); tree2n is read when present, else generated as a
 * minimal tree (the sections FFTree::extend needs, src/tree_io.rs:353-433) and written; bar_wts and z_vals2inv are produced when
 * missing (from the isogeny chain, in milliseconds -- the reference builds treen / treend and evaluates z_poly on them, and
 * leaves those two tree files behind; this entry does not).  validate_precompute != 0: z_poly must not be all zero and must
 * vanish on D (the reference's two asserts; DVP_EINVAL, dvp_last_error_index() = the first point of D where it does not) and,
 * beyond the reference, every file that was FOUND (tree2n with its matrices, bar_wts, z_vals2inv) is compared with the
 * regenerated values (DVP_EINVAL).  *report (optional) = DVP_PREP_* bits, set on every return. */
#define DVP_PREP_WROTE_TREE2N 0x1u
#define DVP_PREP_WROTE_BAR_WTS 0x2u
#define DVP_PREP_WROTE_Z_VALS2INV 0x4u
#define DVP_PREP_Z_POLY_NOT_MONIC 0x8u /* informational: c Z_D with c != 1 passes the reference's check too; bar_wts / z_vals2inv are then
                                        * written (and found files compared) as the monic tables times 1 / c, i.e. what the reference derives
                                        * from THAT z_poly; a zero leading coefficient is DVP_PREP_BAD_Z_POLY */
#define DVP_PREP_BAD_Z_POLY 0x100u
#define DVP_PREP_BAD_BAR_WTS 0x200u
#define DVP_PREP_BAD_Z_VALS2INV 0x400u
#define DVP_PREP_BAD_TREE2N 0x800u
int dvp_prover_prepares_precomputes(const char* cache_dir, int validate_precompute, uint32_t* report);
/* write_fftree_to_file (src/tree_io.rs:144-214) of the minimal tree of a regenerated `tree`: sections f, recombine_matrices,
 * decompose_matrices in the reference's BinaryTree order (layout restated in csrc/setup.hip; third-party, see dvp_fftr_* above) */
int dvp_ecfft_write_tree_file(dvp_ecfft* tree, const char* path);
/* a (reference-built) tree file against the regenerated `tree`: the leaves -- and with matrices != 0 the inner layers of f and
 * both matrix sections -- entry for entry.  DVP_OK identical; DVP_EINVAL differs (*bad_section 0/1/2, *bad_entry the first
 * differing element of f / matrix; both optional); DVP_EIO unreadable or of another size */
int dvp_ecfft_check_tree_file(dvp_ecfft* tree, const char* path, int matrices, int* bad_section, int64_t* bad_entry);

/* The loading half of Proof::prove (src/proving.rs:435-470,509-511,666-672): reads cache_dir/r1cs_to_dvsnark and the
 * SRS vectors g_m, g_q, g_k_0, g_k_1, g_k_2 (src/artifacts.rs:18-27,76), decodes the points on the GPU
 * (DVP_EDECODE = the reference's assert!(valid)) and returns a ready prover; the witness length is |g_m|. */
int dvp_prover_open_cache_dir(const char* cache_dir, uint32_t n_public, dvp_prover** out);
/* Proof::prove(cache_dir, public_inputs, private_inputs) itself: opens cache_dir on first use and keeps the prover in
 * a process-wide table keyed by (cache_dir, n_public, current HIP device); dvp_cache_dir_release(NULL) drops every entry.
 * Thread safety: concurrent calls are allowed; one prover = one set of device buffers, so concurrent callers of one entry take
 * turns on it (the default).  With DVP_CACHE_REPLICAS=2 in the environment an entry opens a SECOND prover from the same files
 * when two calls on it overlap after the first prover has completed a proof AND free device memory exceeds 1.25 x what is in
 * use (two proofs in flight on the GPU), callers taking whichever prover frees first; measured at the end of round 4 that is
 * SLOWER than taking turns when the witness comes from host memory, so it is opt-in.  A release during a
 * prove takes effect when that prove returns.  Files that change on disk after the first
 * call are not re-read: release the entry first.  Only SRS files whose 30-byte encodings follow this library's codec
 * rule are supported until that rule is pinned against xs233 (tools/pin_xsk233.py). */
int dvp_prove_cache_dir(const char* cache_dir, const uint64_t* public_inputs, uint32_t n_public, const uint64_t* private_inputs,
                        uint32_t n_private, uint8_t proof[118]);
/* Proof::prove(cache_dir, public_inputs: Vec<Fr>, private_inputs: &[Fr]), src/proving.rs:426, with both vectors as the caller's memory
 * holds them: dvp_prove_ark on the entry's prover, under the locking and replica rules of dvp_prove_cache_dir.  A NULL vector with a
 * non-zero count is DVP_EINVAL before cache_dir is opened. */
int dvp_prove_cache_dir_ark(const char* cache_dir, const uint64_t* public_ark, uint32_t n_public, const uint64_t* private_ark,
                            uint32_t n_private, uint8_t proof[118]);
/* load_witness_from_file + Proof::prove in one call (src/gnark_r1cs.rs:188-211 -> src/proving.rs:426): the witness file
 * (witness_path == NULL reads <cache_dir>/witness_to_dvsnark) is mapped and proved through dvp_prove_be32 on the entry's prover, under
 * the locking and replica rules of dvp_prove_cache_dir; its elements are reduced on the device.  The header is checked by the rules
 * of dvp_file_witness_read (DVP_EIO for a missing or short file), the count must reach 1 + n_public and element 0 must be 1
 * (DVP_EINVAL, index 0) -- all of it before cache_dir is opened, so these answers need no device.  A file longer than the commitment
 * key is truncated, a shorter one is DVP_EINVAL.  public_inputs_out (optional, n_public x 4): elements 1 .. n_public, canonical. */
int dvp_prove_cache_dir_witness_file(const char* cache_dir, uint32_t n_public, const char* witness_path, uint8_t proof[118],
                                     uint64_t* public_inputs_out);
void dvp_cache_dir_release(const char* cache_dir);
/* dvp_prover_set_transcript_binding for the prover(s) dvp_prove_cache_dir keeps for (cache_dir, n_public), opened if need be:
 * bind_srs != 0 with srs_hash == NULL computes dvp_prover_srs_hash of the opened prover and binds that; a second prover
 * (DVP_CACHE_REPLICAS=2) inherits the binding.  Waits for a proof in flight on the entry's first prover when it has to compute the hash;
 * takes effect with the next proof that starts; a release of the entry drops it. */
int dvp_cache_dir_set_binding(const char* cache_dir, uint32_t n_public, const uint8_t* srs_hash, const uint8_t* circuit_hash, int bind_srs);
/* dvp_prover_circuit_hash (Transcript::circuit_info_hash, src/proving.rs:111-134, on the instance src/gnark_r1cs.rs:333-386 leaves) from
 * <cache_dir>/r1cs_to_dvsnark alone -- the verifier's way to the value, since it ran the setup from the same dump.  No other file of
 * the directory is read.  When dvp_prove_cache_dir's prover of (cache_dir, n_public) is open on the current device it is used (the
 * call takes its turn like a proof); otherwise a prover without SRS is built from the dump (log2 m by next_power_of_two of the row
 * count, n_wires as dvp_r1cs_dump_sizes reports it) and destroyed.  DVP_EIO for a missing or malformed dump. */
int dvp_circuit_hash_cache_dir(const char* cache_dir, uint32_t n_public, uint8_t out[32]);
/* dvp_prover_check_witness_be32 on a witness file (witness_path == NULL reads <cache_dir>/witness_to_dvsnark), with the prover found
 * as dvp_circuit_hash_cache_dir finds it: the open prover of (cache_dir, n_public), taking its turn like a proof, or else one built
 * from the dump without SRS and destroyed -- no SRS file is read.  The file's header follows dvp_prove_cache_dir_witness_file (DVP_EIO
 * for a missing or short file, DVP_EINVAL for a count below 1 + n_public or below the prover's n_wires; a longer file is truncated);
 * element 0 is not refused but reported.  NULL report or a NULL array with a non-zero cap: DVP_EINVAL before any file is opened. */
int dvp_check_witness_cache_dir_witness_file(const char* cache_dir, uint32_t n_public, const char* witness_path, dvp_unsat_row* rows,
                                             size_t rows_cap, dvp_suspect_wire* wires, size_t wires_cap, dvp_witness_report* report);
/* One prover, many verifiers, from directories (SRS per Trapdoor, src/srs.rs:31-50,177): the SRS of a further verifier -- the point files
 * g_m, g_q, g_k_0, g_k_1, g_k_2 of srs_dir (src/artifacts.rs:18-27), same reader and decoder as dvp_prover_open_cache_dir, strict-points
 * mode honoured -- goes into a new SRS slot of the FIRST prover dvp_prove_cache_dir keeps for (cache_dir, n_public), opened if need be;
 * *slot = its index (slot 0 is cache_dir's own SRS).  Adding the same srs_dir (same path string) again returns the slot it has.  If
 * srs_dir holds an R1CS dump, its dvp_circuit_hash_cache_dir must equal cache_dir's: DVP_EINVAL otherwise.  A missing or short point
 * file is DVP_EIO, a count that is not cache_dir's DVP_EINVAL; after any failure no slot has been added.  Takes the prover's turn
 * like a proof.  A release of the entry drops the slots with it. */
int dvp_cache_dir_add_srs_dir(const char* cache_dir, uint32_t n_public, const char* srs_dir, uint32_t* slot);
/* dvp_cache_dir_set_binding for ONE slot (src/srs.rs:31-50,177: the binding is a function of the SRS under bind_srs): slot 0 is
 * dvp_cache_dir_set_binding itself; any other slot is bound at once, on the first prover, taking its turn; bind_srs != 0 with
 * srs_hash == NULL binds dvp_prover_srs_hash of that slot.  An unknown slot is DVP_EINVAL. */
int dvp_cache_dir_slot_set_binding(const char* cache_dir, uint32_t n_public, uint32_t slot, const uint8_t* srs_hash,
                                   const uint8_t* circuit_hash, int bind_srs);
/* dvp_prove_multi / dvp_prove_multi_ark / dvp_prove_multi_be32 (Proof::prove, src/proving.rs:426-688, once per SRS, src/srs.rs:31-50,177)
 * on the first prover of (cache_dir, n_public), under the locking rules of dvp_prove_cache_dir (never on a second prover: it holds slot 0
 * only).  The witness-file form checks the file as dvp_prove_cache_dir_witness_file does, before cache_dir is opened. */
int dvp_prove_cache_dir_multi(const char* cache_dir, uint32_t n_public, const uint32_t* slots, uint32_t n_slots, const uint64_t* public_inputs,
                              const uint64_t* private_inputs, uint32_t n_private, uint8_t* proofs /* n_slots x 118 */, int32_t* status);
int dvp_prove_cache_dir_multi_ark(const char* cache_dir, uint32_t n_public, const uint32_t* slots, uint32_t n_slots, const uint64_t* public_ark,
                                  const uint64_t* private_ark, uint32_t n_private, uint8_t* proofs, int32_t* status);
int dvp_prove_cache_dir_multi_witness_file(const char* cache_dir, uint32_t n_public, const uint32_t* slots, uint32_t n_slots,
                                           const char* witness_path, uint8_t* proofs, int32_t* status, uint64_t* public_inputs_out);
/* the cached prover of (cache_dir, n_public), opened if need be -- borrowed, for inspection only (debug reads, plans) */
int dvp_cache_dir_prover(const char* cache_dir, uint32_t n_public, dvp_prover** out);

#ifdef __cplusplus
}
#endif
#endif /* DVPARI_H */
