// ECFFT over Fr on gfx950: domain/twiddle generation and the extend / enter / exit butterflies.
//
// Replaces the third-party `ecfft` crate as the reference uses it:
//   build_ec_fftrees / build_sect_ecfft_tree   src/ec_fft.rs:93-170,197-239   -> dvp_ecfft_create
//   FFTree::extend(evals, Moiety::S1)           src/proving.rs:410-422         -> dvp_ecfft_extend
//   FFTree::enter / FFTree::exit                src/ec_fft.rs:266,317,411      -> dvp_ecfft_enter/exit
//
// Math (Ben-Sasson, Carmon, Kopparty, Levit, "ECFFT part I"):
//   layer d has N_d = N >> d leaves L_d; psi_d(x) = x + t_d/(x - x0_d) is the x-map of the
//   2-isogeny with kernel <(x0_d,0)> (the one lowering the 2-adicity of the generator,
//   src/ec_fft.rs:131-148); L_{d+1}[i] = psi_d(L_d[i]) = psi_d(L_d[i + N_d/2]).
//   A polynomial P of degree < n on n points decomposes as
//        P(x) = (P0(psi(x)) + x P1(psi(x))) * (x - x0)^(n/2-1)
//   so moving n evaluations from the even leaves to the odd leaves of a 2n-leaf layer is
//   log2(n) "decompose" butterfly passes (2x2 inverse matrices built from even-leaf pairs) followed
//   by log2(n) "recombine" passes (2x2 matrices built from odd-leaf pairs).  At pass d the vector
//   is 2^d independent blocks that all share the layer-d matrices.
//
// Data stays CANONICAL in HBM; matrices/tables are stored in Montgomery form so that
// mont_mul(const, data) is already the canonical product (see fr.cuh).
//
// ONE translation unit: this file includes the stage headers ecfft_*.cuh in the order of the algorithm; every kernel is launched from
// this unit and counted as "ecfft.hip:<kernel>" (common.h: DVP_LAUNCH).  Stage -> text:
//   context      ecfft_internal.h      struct dvp_ecfft: the domain and every table built for it, one lock, one destructor; vanish_chain
//   domain       ecfft_domain.cuh      curve constants, SwPt / sw_add, k_leaves, k_next_layer, ecfft_init
//   constants    ecfft_twiddle.cuh     k_build_mats, k_build_twiddles, k_twist_layer, k_twist_finish, build_matset
//   butterflies  ecfft_butterfly.cuh   Tw, ld30 / st30, bf_*, tw_in2 / tw_out2, radix4, k_butterfly, k_butterfly4, k_butterfly8
//   LDS kernels  ecfft_lds.cuh         ExtIo, io_load2 / io_store2, lds_bfly / lds_bfly4, k_extend_fused, TwTile, k_extend_top
//   extend       ecfft_extend.cuh      ExtIoSpec, ext_io_ok, with_batch / with_sm, extend_io, extend_inplace, extend_from
//   enter, exit  ecfft_enter_exit.cuh  the pointwise and table kernels (k_enter_*, k_leaf_matmul8, k_exit_*, k_rho, ..), get_xnn, the
//                                      leaf-8 / enter / exit table builders, enter_core, exit_levels, exit_core, ecfft_device_consts
//   read-outs    ecfft_debug.cuh       k_mats_export, dvp_debug_ecfft_matrices, layer_to_host, dvp_debug_ecfft_layer
//   here         the C ABI entries with their input check (check_canonical_dev) and host round trip
#include <vector>
#include <map>
#include <mutex>
#include <cstring>

#include "common.h"
#include "host_api.h"
#include "fr.cuh"
#include "ecfft_internal.h"

using namespace dvp;

#include "ecfft_domain.cuh"
#include "ecfft_twiddle.cuh"
#include "ecfft_butterfly.cuh"
#include "ecfft_lds.cuh"
#include "ecfft_extend.cuh"
#include "ecfft_enter_exit.cuh"
#include "ecfft_debug.cuh"

// ---- C ABI ---------------------------------------------------------------------------------------
extern "C" int dvp_ecfft_create(uint32_t log_n, int shifted, uint32_t base_log, dvp_ecfft** out) {
  if (!out || log_n < 1 || log_n > (uint32_t)ECFFT_LOG_ORDER) return DVP_EINVAL;
  if (base_log == 0) base_log = log_n;
  if (base_log < log_n || base_log > (uint32_t)ECFFT_LOG_ORDER) return DVP_EINVAL;
  dvp_ecfft* c = new dvp_ecfft();
  int rc = ecfft_init(c, log_n, shifted, base_log);
  if (rc != DVP_OK) {
    dvp_ecfft_destroy(c);
    return rc;
  }
  *out = c;
  return DVP_OK;
}
extern "C" void dvp_ecfft_destroy(dvp_ecfft* c) { delete c; }  // ~dvp_ecfft frees every table (ecfft_internal.h)

extern "C" uint32_t dvp_ecfft_log2_leaves(const dvp_ecfft* c) { return c ? (uint32_t)c->log_n : 0; }

extern "C" int dvp_ecfft_leaves(const dvp_ecfft* c, uint64_t* out) { return layer_to_host(c, 0, out); }

static int check_canonical_dev(const Fr* d, size_t n, hipStream_t st) {
  ErrWord bad;
  DVP_TRY(bad.arm(st));
  DVP_LAUNCH(k_check_canonical, dim3(cdiv(n, TPB)), dim3(TPB), 0, st, d, n, bad.word());
  return bad.verdict(st, DVP_EINVAL);
}

extern "C" int dvp_ecfft_extend_dev(dvp_ecfft* c, const void* d_in, uint32_t batch, void* d_out, void* stream) {
  if (!c || !d_in || !d_out || batch == 0) return DVP_EINVAL;
  return extend_from(c, 0, 0, (const Fr*)d_in, (Fr*)d_out, batch, (hipStream_t)stream);  // the first pass reads d_in, everything after it d_out
}

extern "C" int dvp_ecfft_extend(dvp_ecfft* c, const uint64_t* evals, uint32_t batch, uint64_t* out) {
  if (!c || !evals || !out || batch == 0) return DVP_EINVAL;
  size_t bytes = (size_t)batch * (c->n_leaves >> 1) * sizeof(Fr);
  DevBuf buf;
  DVP_TRY(buf.up(evals, bytes));
  DVP_TRY(check_canonical_dev(buf.as<Fr>(), bytes / sizeof(Fr), 0));
  DVP_TRY(extend_inplace(c, 0, 0, buf.as<Fr>(), batch, 0));
  return buf.down(out, bytes);
}

// enter / exit on the whole tree: the entries take the context's lock, enter_core / exit_core and the table builders run under it
extern "C" int dvp_ecfft_enter_dev(dvp_ecfft* c, const void* d_coeffs, void* d_out, void* stream) {
  if (!c || !d_coeffs || !d_out) return DVP_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  return enter_core(c, 0, (const Fr*)d_coeffs, (Fr*)d_out, (hipStream_t)stream);
}
extern "C" int dvp_ecfft_exit_dev(dvp_ecfft* c, const void* d_evals, void* d_out, void* stream) {
  if (!c || !d_evals || !d_out) return DVP_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  return exit_core(c, 0, (const Fr*)d_evals, (Fr*)d_out, (hipStream_t)stream);
}

static int host_roundtrip(dvp_ecfft* c, const uint64_t* in, uint64_t* out, bool is_exit) {
  if (!c || !in || !out) return DVP_EINVAL;
  size_t bytes = (size_t)c->n_leaves * sizeof(Fr);
  DevBuf i, o;
  DVP_TRY(i.up(in, bytes));
  DVP_TRY(o.alloc(bytes));
  DVP_TRY(check_canonical_dev(i.as<Fr>(), c->n_leaves, 0));
  DVP_TRY(is_exit ? dvp_ecfft_exit_dev(c, i.p, o.p, nullptr) : dvp_ecfft_enter_dev(c, i.p, o.p, nullptr));
  return o.down(out, bytes);
}
extern "C" int dvp_ecfft_enter(dvp_ecfft* c, const uint64_t* coeffs, uint64_t* out) { return host_roundtrip(c, coeffs, out, false); }
extern "C" int dvp_ecfft_exit(dvp_ecfft* c, const uint64_t* evals, uint64_t* out) { return host_roundtrip(c, evals, out, true); }

// Z_D(x) (which = 0: even leaves) or Z_D'(x) (which = 1: odd leaves); the isogeny chain on the host, O(log N) field ops
extern "C" int dvp_ecfft_vanish_at(const dvp_ecfft* c, int which, const uint64_t x[4], uint64_t out[4]) {
  if (!c || !x || !out || (which != 0 && which != 1)) return DVP_EINVAL;
  Fr xc;
  if (!fr_load(x, &xc)) return DVP_EINVAL;
  int kk = c->log_n - 1;
  Fr cpt[2];  // the two leaves of layer kk (Montgomery): even leaves collapse to [0], odd leaves to [1]
  DVP_HIP(hipMemcpy(cpt, c->layer(kk), 2 * sizeof(Fr), hipMemcpyDeviceToHost));
  Fr z = fr_from_mont(vanish_chain(fr_to_mont(xc), c->x0.data(), c->t.data(), kk, cpt[which]));
  memcpy(out, z.v, 32);
  return DVP_OK;
}
