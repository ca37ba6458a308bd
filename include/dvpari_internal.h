/*
 * dvpari_internal.h -- entry points of libdvpari_hip.so that are NOT part of the drop-in boundary.
 *
 * include/dvpari.h is what a host of the reference prover binds (one entry per seam of alpenlabs/dv-pari).  The
 * symbols below exist for this repository's own tests, sweeps and measurement harness (tests/, tools/, bench.py):
 * tuning knobs, per-kernel timers, microbenchmarks and read-outs of intermediates.  They may change between builds;
 * a host program (examples/dvp_prove_cli.cpp) must build against dvpari.h alone.
 */
#ifndef DVPARI_INTERNAL_H
#define DVPARI_INTERNAL_H

#include "dvpari.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knobs for tests, sweeps and A/B runs (tools/README.md lists them; the defaults are the measured optima and
 * the environment variables of the same names are read once, at first use).  dvp_tune_set returns DVP_EINVAL for an
 * unknown name; dvp_tune_reset goes back to defaults + environment; dvp_tune_get reads the current value.  Not
 * thread-safe against running calls. */
int dvp_tune_set(const char* name, long long value);
int dvp_tune_get(const char* name, long long* value);
void dvp_tune_reset(void);

/* Per-kernel HIP-event timers for the measurement harness (bench.py): off by default.  Names:
 * "msm_affine_round0" (first k_affine_round of an MSM, the dominant kernel: it gathers the bases), "msm_affine_rest"
 * (the later pair rounds), "msm_sort" (recode + counting sort), "msm_tail" (merge tree, Frobenius tail), "msm_total",
 * "extend_total", "prove_total"; and two counters that are always on (launches = count since dvp_profile_reset, total_ms = 0):
 * "host_waits_stream" (synchronisations of the proof's own stream: the GPU idles until the host has reacted) and
 * "host_waits_side" (an MSM's largest-bucket read, taken on a side stream while its first pair round runs). */
void dvp_profile_enable(int on);
void dvp_profile_reset(void);
int dvp_profile_read(const char* name, double* total_ms, uint64_t* launches);
/* The launch census: every kernel launch of the library is counted per variant, always (one relaxed host increment per launch).  A
 * variant is one kernel with its instantiated template arguments, named "<file>:<kernel><args>" as the compiler spells the
 * instantiation, without blanks and with every argument written out: "msm.hip:k_merge<16,false>", "msm.hip:k_affine_round<false,false,true>",
 * "ecfft.hip:k_leaf_matmul8".  dvp_debug_launch_names writes the newline-separated list of all names (every variant host code can
 * launch, known when the library is loaded) into buf (truncated to cap, NUL-terminated) and returns the bytes needed; it touches no
 * device.  dvp_profile_read("launch:<name>", &ms, &n) gives n = launches of that variant since the last dvp_profile_reset and ms = 0;
 * an unknown name is DVP_EINVAL. */
int dvp_debug_launch_names(char* buf, size_t cap);
/* the length the device wrote into the rest list (k_bucket_pairs' buckets / k_accum_affine_fast's tasks that met an exceptional pair)
 * during the calling thread's last MSM, read from its workspace after waiting for that MSM's stream.  DVP_EINVAL before the first MSM. */
int dvp_debug_msm_rest_len(uint32_t* n);

/* TEST ONLY: the intermediate arrays of ONE MSM, stage by stage (tests/msm_stage_cases.py parses the blob and restates every stage).
 * dvp_debug_msm_capture_arm(arena_bytes) arms the calling thread's NEXT MSM -- one-shot or dvp_msm_ctx_run, host or _dev entry -- and
 * allocates a device arena of that size (0 = disarm and free).  That MSM runs as any other, plus device-to-device copies into the arena
 * enqueued on its own stream at the stage boundaries (no kernel, no event, no wait); an MSM of a thread that has not armed does nothing
 * of this.  dvp_debug_msm_capture_fetch waits for that MSM's stream and writes one blob of 32-bit words:
 *   header, 136 words: [0] 0x43505644, [1] version 2, [2] 136, [3] flavour (bit 0 fixed-base, bit 1 signed digits), [4] c, [5] W,
 *     [6] n_narrow, [7] nkeys, [8] sign mask of an item, [9] n_total (row stride of the table; one-shot: n), [10] i0, [11] n, [12] ra
 *     (pair rounds run), [13] ra_plan, [14] dense descriptors, [15] bookkeeping (0 per round, 1 all rounds on a side stream, 2 all rounds
 *     on the caller's), [16] workgroup size of the rounds, [17] aff_cap (resident round threads), [18] bmax, [19] bmin, [20] leftover
 *     route (0 k_bucket_gather_items, 1 k_bucket_gather_aff, 2 k_bucket_pairs + k_bucket_rest, 3 fan-in-K reducer with the exception-free
 *     first level, 4 with the general one), [21] K, [22] the largest bucket, [23] items_len = off[nkeys], [24 + r] round r shared its
 *     inversions, [64 + r] total_r = output slots of round r; since version 2: [104] merge levels run, [105] the tail's shape (0 k_tail<true>
 *     with n_narrow = -3, 1 k_tail<false> with -3, 2 k_tail<false> alone over the Frobenius powers, 3 k_tail_groups + k_tail<false> with
 *     -4), [106] nparts = group sums of k_tail_groups (0 unless shape 3), [107] 1 if a 30-byte encoding was written, [108] the codec rule
 *     it was written under, [109 .. 111] zero, [112 + j] GROUP = lanes per addition of merge level j (1, 4 or 16), j < 24;
 *   after the sort: cnt[nkeys], off[nkeys + 1], items[items_len];
 *   per round r < ra: its output counts [nkeys] and offsets [nkeys + 1], its descriptor words as the kernel read them (round 0: none,
 *     it reads the item list; later rounds total_r words, 2 total_r on the dense path), its output points total_r x 16 words (x, y);
 *   after the leftover reducer: bkt[nkeys] x 24 words, raw (X, Y, Z);
 *   per merge level j < levels: the whole bucket array behind that k_merge launch, nkeys x 24 words, lambda-projective (X, L, Z) -- level 0
 *     converts every bucket on its way in, so no slot of these copies is Lopez-Dahab;
 *   signed digits (sign mask != 0) only: save0, 24 words: bucket 0 as level 0 kept it aside, raw Lopez-Dahab (X, Y, Z);
 *   tail shape 3 only: nparts x 24 words, the group sums k_tail_groups left (Lopez-Dahab), copied before k_tail reuses their memory;
 *   the result as the last tail kernel wrote it: 16 words (x, y), 1 word inf, and, if [107], 8 words holding the 30 encoding bytes (the
 *     last two bytes zero).
 * fetch(NULL, 0, &need) reports the blob's size and keeps the capture; a buffer smaller than that is DVP_EINVAL, nothing written.  An
 * arena too small for what the MSM had to copy: DVP_EINVAL, no blob at all, dvp_last_error_index() = the arena bytes it wanted.  A
 * fetch without a captured MSM is DVP_EINVAL.  A successful fetch, a failed one and a new arming free the arena. */
int dvp_debug_msm_capture_arm(size_t arena_bytes);
int dvp_debug_msm_capture_fetch(void* out, size_t cap_bytes, size_t* need);
/* TEST ONLY: one MSM whose tail kernel also writes the result's 30-byte encoding under the current codec rule, from the inversion it
 * shares with the affine conversion -- what a prover asks of its commitment MSMs, here on inputs of the caller's choice.  ctx != NULL: the
 * context's bases [lo, hi) (bases_xy unused); ctx == NULL: a one-shot MSM over bases_xy[0 .. hi), lo = 0.  scalars: hi - lo canonical
 * scalars.  A neutral result: out_is_infinity = 1 and 30 zero bytes. */
int dvp_debug_msm_enc(dvp_msm_ctx* ctx, const uint64_t* scalars, const uint64_t* bases_xy, size_t lo, size_t hi, uint64_t out_xy[8],
                      int* out_is_infinity, uint8_t out_enc[30]);

/* "msm_affine_round0" split by launch shape: entry k = (pairs of the MSM, summed ms, launches) for every distinct MSM size
 * since the last reset; returns the number of shapes (fills at most `cap`), < 0 on error */
int dvp_profile_round0_shapes(uint64_t* pairs, double* total_ms, uint64_t* launches, int cap);

/* microbenchmark of the MSM kernels' GF(2^233) multiplier alone (products per second, whole chip, the pair rounds'
 * occupancy): the ceiling of bench.py's work model, measured in the same run */
int dvp_ubench_gf_mul(int reps, double* products_per_s);
/* the same for the ECFFT's multiplier: multiply-adds r = a b / R' + c per second of the lazy 30-bit-limb Fr multiplier (pairs of
 * independent chains, as the twisted butterflies issue them), whole chip: the ceiling of bench.py's work model for extend / enter /
 * exit (BASELINE configs #3 and #4) */
int dvp_ubench_fr_mul(int reps, double* muladds_per_s);
/* k_points_check against k_decode on the same count in one run (tools/points_check.py): device events around each kernel alone, one
 * warm-up launch and then the median of `reps` (odd, 1 .. 99).  d_xy / d_inf: n affine points; d_enc: n x 30 B encodings; d_scratch:
 * n x 65 bytes the decode kernel writes its points and flags into.  Waits for the result. */
int dvp_ubench_points_check(const void* d_xy, const void* d_inf, const void* d_enc, size_t n, void* d_scratch, int reps,
                            double* check_ms, double* decode_ms);
/* dvp_points_mul_dev (at the DVP_POINTS_MUL_W in force) against its yardstick k_mulgen on the same scalars and count in one run
 * (tools/points_mul.py): device events around each alone, one warm-up and then the median of `reps` (odd, 1 .. 99).  d_scalars: n x 32 B
 * canonical; d_xy: n affine points of E[r]; d_scratch: n x 65 bytes both write their points and flags into.  Waits for the result. */
int dvp_ubench_points_mul(const void* d_scalars, const void* d_xy, size_t n, void* d_scratch, int reps, double* mul_ms, double* mulgen_ms);
/* Wave-level trace of the batched-affine pair rounds (dvp::k_affine_round, tools/wave_trace.py).  d_buf = device buffer of
 * 64 + 64 * n_records bytes zeroed by the caller, NULL = off.  While set, every pair round appends one 64-byte record per
 * wave (8 u64: s_memrealtime at wave start / after pass 1 / after the shared inversion / at the end; s_memtime at start / end;
 * HW_ID | XCC_ID << 32; blockIdx | launch tag << 32 | slots per thread << 48 | the wave's number in its workgroup << 56 | this wave
 * ran the workgroup's inversion << 60 | the launch shares its inversions << 61); word 0 of the buffer counts them. */
int dvp_debug_wave_trace(void* d_buf, uint32_t n_records);
/* random 64-byte gathers per second (whole chip, two independent lines in flight per lane and step, as the first pair
 * round issues them) out of a device table of `table_bytes` bytes starting at d_table; d_table = NULL allocates a scratch
 * table of that size.  The ceiling of bench.py's gather model for dvp::k_affine_round<true>. */
int dvp_ubench_gather(const void* d_table, size_t table_bytes, int reps, double* gathers_per_s);
/* device address and size of the pre-rotated base table MSM `which` of a prover reads in its first pair round
 * (NULL / 0 before the first proof) -- what dvp_ubench_gather is pointed at */
int dvp_prover_msm_table_ptr(const dvp_prover* p, int which, const void** d_table, uint64_t* bytes);

/* The table-budget planner of dvp_prover_set_table_budget as a pure host function (no device is touched): size0 / size1 = the
 * terms of MSM 0 / MSM 1 of a prover, budget_bytes = its budget.  covered[w] = leading bases of MSM w that get a table, bytes[w] =
 * that table's size: rows x covered[w] x 64 with the row count the fixed-base context settles on for that many bases
 * (DVP_MSM_FIXED_C, DVP_MSM_ALIGNED_SIGNED and DVP_MSM_FIXED_MIN apply as they do to a prover).  bytes[0] + bytes[1] <= budget_bytes;
 * MSM 1 is served first and at most one of the two is partly covered. */
int dvp_table_plan(size_t size0, size_t size1, uint64_t budget_bytes, size_t covered[2], uint64_t bytes[2]);

/* Whether a batched-affine pair round takes its field inversion once per workgroup (1) or once per wave (0), as a pure host function
 * (no device is touched): mode = DVP_MSM_AFF_SHARE_INV (0 never, 1 always, 2 by size), tpb = the rounds' workgroup size
 * (DVP_MSM_AFF_TPB; 64 threads are one wave and never share), planned = the additions the round plans, share_min =
 * DVP_MSM_AFF_SHARE_MIN, chip_full = resident pair-round threads x DVP_MSM_AFF_BMIN, the threshold that stands in for share_min = 0.
 * dvp_profile_read("rounds_inv_shared" / "rounds_inv_private") counts the launches of either form. */
int dvp_aff_share_plan(long long mode, uint32_t tpb, uint64_t planned, uint64_t share_min, uint64_t chip_full);

/* parity-test access to the recode of the default fixed-base flavour alone (signed aligned windows): out_words[w * n + i] = 0 (digit 0) or 0x80000000 | 0x10000000 when the
 * digit is negative | w << 20 | |digit| (|digit| = 2^(c-1) is stored as key 0); *windows = ceil(234 / c_bits) */
int dvp_debug_recode_signed(const uint64_t* scalars, size_t n, int c_bits, uint32_t* out_words, int* windows);

/* parity-test access to the width-w tau-NAF recoder of dvp_points_mul alone (w = 3, 4, 5), run on the device: digits[i * *n_digits + j] =
 * the signed digit of scalar i at position j (+-u, u odd < 2^(w-1); 0 for none), *n_digits = the PROVEN bound on the positions (csrc/tau.cuh:
 * TnafDigits), alpha[2 e], alpha[2 e + 1] = (beta, gamma) of the representative alpha_(2e+1) = beta + gamma tau the kernel's table holds,
 * e < 2^(w-2).  digits == NULL: only *n_digits and alpha (no device call).  A non-canonical scalar: DVP_EINVAL and its index. */
int dvp_debug_recode_tnaf(const uint64_t* scalars, size_t n, int w, int8_t* digits, int* n_digits, int32_t* alpha /* 2^(w-2) x (beta, gamma) */);

/* TEST / HARNESS ONLY: the SRS scalars (discrete logs of the bases: trapdoor material) of an IN-MEMORY circuit -- CSR matrices L, R, O
 * over n_rows <= 2^log2_m rows (row_ptr[k]: n_rows + 1 entries), coefficient table (n_coeffs x 4 u64, canonical), n_wires -- in
 * file order g_m | g_q | g_k_0 | g_k_1 | g_k_2 ((n_wires + 5 m) x 4 u64, out_cap in elements).  The same device pipeline
 * dvp_setup_cache_dir runs on a parsed dump; dv-pari_amd/srs.py: srs_scalars (bench.py's synthetic circuit, the tests) calls it. */
int dvp_setup_scalars(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], uint32_t log2_m, uint32_t n_public,
                      uint32_t n_rows, uint32_t n_wires, const uint64_t* coeffs, uint32_t n_coeffs, const uint32_t* const row_ptr[3],
                      const uint32_t* const wire_ids[3], const uint32_t* const coeff_ids[3], uint64_t* out_scalars, size_t out_cap);

/* TEST-ONLY (never bind this in a host): dvp_setup_cache_dir that also returns the discrete logs of the bases it wrote -- trapdoor
 * material, which dvp_setup_cache_dir itself zeroes on the device before it returns -- (host, (n_wires + 5 m) x 4 u64, file order
 * g_m | g_q | g_k_0 | g_k_1 | g_k_2; NULL = not wanted; out_cap in elements) and the circuit's sizes: parity tests pin the SRS
 * and the proof's commitments with them */
int dvp_setup_cache_dir_ex(const uint64_t tau[4], const uint64_t delta[4], const uint64_t epsilon[4], const char* cache_dir,
                           uint32_t n_public, int write_precomputes, uint64_t* out_scalars, size_t out_cap, uint32_t* out_n_wires,
                           uint32_t* out_log2_m);

/* the device flavour of the Fiat-Shamir transcript (what dvp_prove_dev runs between its two MSMs since round 5) on caller-supplied
 * inputs: alpha (canonical, to be compared with dvp_transcript_challenge) and -Z_D(alpha) (canonical) for this prover's domain;
 * n_public <= 35 (one BLAKE3 chunk of 29-byte inputs) */
int dvp_prover_debug_transcript_dev(dvp_prover* p, const uint8_t commit_p[30], const uint64_t* public_inputs, uint32_t n_public,
                                    uint64_t out_alpha[4], uint64_t out_neg_z_alpha[4]);

/* TEST ONLY: a canonical alpha (four LE u64, below p) replaces the transcript's output in every later proof on this prover -- every
 * entry that derives alpha: dvp_prove*, dvp_prove_multi*, dvp_prove_challenge, dvp_prove_challenge_partial -- so that the refusal of a
 * challenge in D u D' (DVP_ECHALLENGE, src/proving.rs:548-556), which a 224-bit hash never meets, can be reached.  NULL clears it;
 * alpha >= p is DVP_EINVAL.  Host-side only: the host flavour swaps the value it hashed, the device flavour copies alpha and its
 * Montgomery form into the prover's block in the place of k_transcript's launch; everything downstream runs unchanged. */
int dvp_prover_debug_force_alpha(dvp_prover* p, const uint64_t alpha[4]);

/* TEST ONLY: the two halves of dvp_blake3_dev apart, so that a long stream can be hashed piecewise (what dvp_prover_srs_hash does with
 * its staging windows).  leaves: the chaining values of the 1 KiB chunks of d_data[0, len), len > 0, a piece of a stream that starts at
 * chunk `chunk_base` of it (so at a multiple of 1024 bytes; every piece but the last is a multiple of 1024 bytes long) -> d_cvs, 32
 * bytes per chunk.  reduce: n >= 2 chaining values -> the digest; d_cvs is overwritten, d_tmp holds 32 bytes per tree_run values
 * (rounded up).  tree_run: the chaining values one workgroup of the tree kernel reduces per launch. */
uint32_t dvp_debug_blake3_tree_run(void);
int dvp_debug_blake3_leaves_dev(const void* d_data, size_t len, uint64_t chunk_base, void* d_cvs, void* stream);
int dvp_debug_blake3_reduce_dev(void* d_cvs, size_t n, void* d_tmp, void* d_out32, void* stream);

/* intermediates of the last proof, for parity tests (names: see prove.hip) */
int dvp_prover_debug_read(dvp_prover* p, const char* name, uint64_t* out, size_t n_elems);

/* the 2x2 butterfly matrices extend() runs on, for parity tests against the oracle and against FFTR tree files
 * (ecfft::FFTree::{decompose,recombine}_matrices, src/tree_io.rs:353-433): direction to_even = 0 is
 * FFTree::extend(.., Moiety::S1) (even leaves -> odd leaves), 1 the mirrored one; which = 0 decompose, 1 recombine.
 * out holds (n - 1) matrices of 4 canonical Fr (row-major m00 m01 m10 m11), n = leaves / 2, layer d (n >> (d+1) matrices
 * built from the pairs (L_d[2i+s], L_d[2i+s+n_d]) of the layer-d leaves) at matrix offset n - (n >> d). */
int dvp_debug_ecfft_matrices(dvp_ecfft* ctx, int to_even, int which, uint64_t* out);
/* layer d of the isogeny chain (FFTree::f.get_layers()[d]): leaves >> d canonical Fr, d = 0 .. log2_leaves */
int dvp_debug_ecfft_layer(const dvp_ecfft* ctx, uint32_t d, uint64_t* out);

/* TEST ONLY: one function of the Fr arithmetic (csrc/fr.cuh) per element, for the carry-boundary tests (tests/fr_cases.py holds the
 * integer reference).  Every value is a raw 256-bit integer (4 x u64, little-endian) handed to the function untouched: "Montgomery
 * in / out" functions see their operand as it is, e.g. MUL gives a b / 2^232 mod p.  in[k] / out[k]: n values each; pointers beyond an
 * op's count are not read.  on_device = 1: a kernel, one element per lane, 256-thread workgroups -- the device build of the function
 * as the kernels get it; on_device = 0: a host loop over the same functions that makes no HIP call (runs without a GPU).  An element
 * outside the op's precondition -> DVP_EINVAL, dvp_last_error_index() = its index, before anything is computed.  R = 2^232, R' = 2^240;
 * 29- and 30-bit-limb operands are sliced from the 256-bit value inside the op (fr29_from / fr30_from) and lazy results are re-sliced
 * with fr30_to_fr. */
enum dvp_fr_op {
  DVP_FROP_ADD = 0,      /* in a, b < p: fr_add */
  DVP_FROP_SUB,          /* a, b < p: fr_sub */
  DVP_FROP_NEG,          /* a < p: fr_neg */
  DVP_FROP_DBL,          /* a < p: fr_dbl */
  DVP_FROP_COND_SUB_P,   /* a < 2p: fr_cond_sub_p */
  DVP_FROP_IS_CANONICAL, /* any a: 1 if a < p else 0 */
  DVP_FROP_MUL,          /* a, b < p: fr_mul = a b / R mod p */
  DVP_FROP_SQR,          /* a < p: fr_sqr */
  DVP_FROP_TO_MONT,      /* a < p: a R mod p */
  DVP_FROP_FROM_MONT,    /* a < p: a / R mod p */
  DVP_FROP_DOT2,         /* a0, b0, a1, b1 < p: fr_dot2 = (a0 b0 + a1 b1) / R mod p */
  DVP_FROP_MULADD29,     /* a, b, c < p: fr_muladd29 = a b / R + c mod p */
  DVP_FROP_MUL29,        /* a, b < p: fr_mul29 */
  DVP_FROP_ROUNDTRIP29,  /* a < 2^232: fr_from29(fr_to29(a)) */
  DVP_FROP_ROUNDTRIP30,  /* a < 2^240: fr30_to_fr(fr30_from(a)) */
  DVP_FROP_CONST30,      /* a < p (it goes through fr_mul, which drops bit 232): fr30_const = a 2^8 mod p, fully reduced */
  DVP_FROP_CANON30,      /* a < 2p: fr30_canon */
  DVP_FROP_SUB_LAZY30,   /* e0 < 2^239, e1 < 128 p: fr30_sub_lazy = e0 - e1 + 128 p exactly */
  DVP_FROP_MULADD30,     /* a < p; b, c < 2^240 with the exact result (a b + m p) / R' + c < 2^240: fr30_muladd */
  DVP_FROP_MULADD30_X2,  /* (a0, b0, c0, a1, b1, c1), each triple as MULADD30: fr30_muladd_x2 -> out[0], out[1] */
  DVP_FROP_INV,          /* a < p: fr_inv = R^2 / a mod p; 0 -> 0 */
  DVP_FROP_INV_GCD_RAW,  /* a < p: fr_inv_gcd_raw = 1 / a mod p; 0 -> 0 */
  DVP_FROP_INV_FERMAT,   /* a < p: fr_inv_fermat = R^2 / a mod p; 0 -> 0 */
  DVP_FROP_POW_U64,      /* a < p, e < 2^64: fr_pow_u64 = a^e R^(1 - e) mod p */
  DVP_FROP_LIMBS29,      /* a < 2^232: the eight 29-bit limbs of fr_to29, one per 32-bit word of the output */
  DVP_FROP_LIMBS30,      /* a < 2^240: the eight limbs of fr30_from likewise (limb 7 keeps bits 210 and up) */
  DVP_FROP_COUNT
};
int dvp_debug_fr_op(int op, const uint64_t* const in[6], size_t n, int on_device, uint64_t* const out[2]);
/* TEST ONLY: the HOST build of the function k_fr_from_be32 runs per element (csrc/fr_wire.cuh) over n x 32 big-endian bytes -> n x 4
 * limbs; makes no HIP call (runs without a GPU).  The public entries are dvp_fr_from_be32 / dvp_fr_from_be32_dev. */
int dvp_debug_fr_from_be32_host(const uint8_t* be32, size_t n, uint64_t* out);
/* TEST ONLY: the HOST build of the functions k_fr_from_ark (to_ark = 0) and k_fr_to_ark (to_ark != 0) run per element
 * (csrc/fr_ark.cuh) over n x 4 limbs at any alignment; makes no HIP call (runs without a GPU).  dvp_debug_fr_ark_is_one: fr_ark_is_one
 * on the 32 bytes at `ark` (1 / 0; DVP_EINVAL for NULL).  The public entries are dvp_fr_from_ark / dvp_fr_to_ark and their _dev flavours. */
int dvp_debug_fr_ark_host(int to_ark, const uint64_t* in, size_t n, uint64_t* out);
int dvp_debug_fr_ark_is_one(const uint8_t* ark);

/* TEST ONLY: one function of the GF(2^233) arithmetic (csrc/gf233.cuh) or of the K-233 point formulas (csrc/k233.cuh) per element, on
 * the device (tests/gf_cases.py holds the case sets; oracle/pyref.py is the reference).  Every value is a raw 256-bit integer (4 x u64,
 * little-endian: bit i = coefficient of z^i); a point is two affine fields (x, y) or three projective ones (X, Y, Z), one in[] each.
 * `form` selects the multiplier the function runs on; an (op, form) pair the list below does not name is DVP_EINVAL.  The kernels launch
 * as production does (256-thread workgroups, GF_LDSK_BYTES_PER_WAVE / GF_LDS_BYTES_PER_WAVE of dynamic LDS per wave, the tables of
 * gf_sqr_tables()), and a lane (group) works through several elements one after the other in the same LDS region: element e belongs to
 * group e mod S of the S groups launched, S = 64 / G x max(1, ceil(n G / 128)).  For the quad and row forms one element occupies a
 * group of G = 4 / 16 lanes and out[k] holds n x G values, value e G + r from lane r of the group: the test sees every lane's copy.
 * A group without an element retires as a whole before any cross-lane operation.
 * Preconditions are checked on the host before any device call (nothing out of range reaches a kernel): a field operand >= 2^233 (every
 * input but REDUCE16's), or word 15 of REDUCE16_14's input non-zero -> DVP_EINVAL, dvp_last_error_index() = the element; a `param` out of
 * range (k > 232, an unknown table, a table the current DVP_GF_INV_TABS does not provide) -> DVP_EINVAL, dvp_last_error_index() = -1.
 * Flags (0 / 1 in word 0) go to out[3]; out[] beyond an op's values (and out[3] without a flag) is not written and may be NULL. */
enum dvp_gf_form {
  DVP_GFFORM_REG = 0, /* gf_mul(a, b): registers only (the k233.cuh functions without a multiplier argument) */
  DVP_GFFORM_LDS,     /* GfLds: the 16 KB comb */
  DVP_GFFORM_LDSQ,    /* GfLdsQ: a quad of lanes per product */
  DVP_GFFORM_LDSH,    /* GfLdsH: a row of 16 lanes per product */
  DVP_GFFORM_LDSK,    /* GfLdsK: Karatsuba over 8 KB half tables */
  DVP_GFFORM_COUNT
};
enum dvp_gf_op {
  /* field: forms REG only unless stated */
  DVP_GFOP_ADD = 0,     /* a, b -> a + b */
  DVP_GFOP_MUL,         /* a, b -> a b; every form */
  DVP_GFOP_MUL2,        /* a1, a2, b -> a1 b, a2 b (gf_mul2); the four LDS forms */
  DVP_GFOP_SQR,         /* a -> a^2 */
  DVP_GFOP_SQR_N,       /* a -> a^(2^param), param <= 232 (gf_sqr_n) */
  DVP_GFOP_REDUCE16_15, /* (low 256 bits, high 256 bits) of a 512-bit polynomial -> gf_reduce16<15> */
  DVP_GFOP_REDUCE16_14, /* the same through gf_reduce16<14>: word 15 must be zero */
  DVP_GFOP_SQR_TAB,     /* a -> one table pass: param & 0xff = 0 t29, 1 t58, 2 t116, 3 half-trace, 4 t14, 5 t7; param & 0x100: gf_sqr_tab_wide */
  DVP_GFOP_SQR_N_FAST,  /* a -> a^(2^param), param <= 232 (gf_sqr_n_fast) */
  DVP_GFOP_INV,         /* a -> 1 / a, 0 -> 0 (gf_inv, the register chain) */
  DVP_GFOP_INV_FAST,    /* a -> 1 / a, 0 -> 0 (gf_inv_fast: honours DVP_GF_INV_TABS); the four LDS forms */
  DVP_GFOP_SQRT,        /* a -> sqrt(a) */
  DVP_GFOP_TRACE,       /* a -> Tr(a) in word 0 */
  DVP_GFOP_HALFTRACE,   /* a -> H(a) (gf_halftrace, the squaring loop) */
  /* points: p = in[0..2] (X, Y, Z), q = in[3..4] (x, y) or in[3..5] (X, Y, Z); result (X, Y, Z) -> out[0..2] */
  DVP_GFOP_LD_DBL,         /* p -> 2 p; every form */
  DVP_GFOP_LD_MADD,        /* p, q affine -> p + q (ld_madd; the LDS forms go through ld_madd_ip); every form */
  DVP_GFOP_LD_MADD_FAST,   /* p, q affine -> p + q, flag = 1; p == +-q: p untouched, flag = 0; LDS forms */
  DVP_GFOP_LD_ADD_AFF_AFF, /* p = in[0..1], q = in[2..3], both affine, p.x != q.x -> p + q; LDS forms */
  DVP_GFOP_LD_ADD,         /* p, q -> p + q (ld_add; the LDS forms go through ld_add_ip); every form */
  DVP_GFOP_LD_ADD_NODBL,   /* p, q -> p + q, flag = 1; p == q: p untouched, flag = 0; LDS forms */
  DVP_GFOP_LAM_FROM_LD,    /* Lopez-Dahab -> lambda-projective; LDS forms */
  DVP_GFOP_LAM_TO_LD,      /* lambda-projective -> Lopez-Dahab; LDS forms */
  DVP_GFOP_LAM_DBL,        /* lambda-projective doubling; LDS forms */
  DVP_GFOP_LAM_ADD,        /* lambda-projective p, q -> p + q, flag = 1; p == q: p untouched, flag = 0; LDS forms */
  DVP_GFOP_LD_FROB_N,      /* p -> tau^param p, param <= 232; REG */
  DVP_GFOP_LD_TO_AFF,      /* p -> (x, y) in out[0..1], flag = 0 for infinity; REG */
  DVP_GFOP_COUNT
};
int dvp_debug_gf_op(int op, int form, const uint64_t* const in[6], size_t n, uint64_t param, uint64_t* const out[4]);

#ifdef __cplusplus
}
#endif
#endif /* DVPARI_INTERNAL_H */
