// Proof::prove on gfx950 -- the orchestration of src/proving.rs:426-688 with every vector stage on
// the device; since round 5 the BLAKE3 transcript (src/proving.rs:79-198) runs there too (k_transcript; the host
// flavour stays behind DVP_PROVE_HOST_TRANSCRIPT) and the host only assembles the 118 bytes.  Stage map (reference line -> kernel):
//   get_matrix_evaluations_from_witness   :348-403  -> k_r1cs_eval  (CSR rows, one thread per row; the
//                                                      Vandermonde fold C' = C - D is applied on the fly)
//   multi_scalar_mul(assignment, g_m)     :462-463  \  one MSM over [w | q2] x [g_m | g_q]
//   multi_scalar_mul(q_vals2, g_q)        :511-512  /  (commit_p = msm_q + msm_gm, :515)
//   extend_evals                          :410-422  -> dvp_ecfft batched extend (4 vectors)
//   r_vals2 / q_vals2                     :492-508  -> k_quotient
//   transcript -> alpha                   :517-558  -> k_transcript (or host BLAKE3) + k_alpha_denoms (domain check)
//   barycentric evaluations a0,b0,i0      :561-594  -> k_bary3_partial_range / k_bary3_final
//     (Z(alpha) comes from the isogeny chain instead of a Horner pass over z_poly)
//   denom_invs, denom_invs2               :599-616  -> k_alpha_denoms + batch inverse
//   k_scalar_a / _b / r_vals / k_scalar_r :619-654  -> k_kscalars (interleaved [D_i, D'_i])
//   multi_scalar_mul(srs_s_k, srs_g_k)    :666-680  -> MSM over 4m points
// The prover-side precomputes of prover_prepares_precomputes (:225-325) -- barycentric weights and
// 1/Z_D on D' -- are regenerated on the device from the isogeny chain (k_domain_tables), so neither
// z_poly nor the FFTR tree cache is needed.
//
// ONE translation unit: this file includes the phase headers prove_*.cuh in the order of a proof; every kernel is launched from this
// unit and counted as "prove.hip:<kernel>" (common.h: DVP_LAUNCH).  Phase -> text:
//   kernels     prove_kernels.cuh     every __global__ kernel and device helper of the stage map above
//   state       prove_state.cuh       DevCsr, the result block, struct dvp_prover, PT, HORNER_MAX_PUB, host_vanish, prover_ready
//   slots       prove_slots.cuh       SRS slots: the state model, add / select / drop / bytes
//   setup       prove_setup.cuh       create / init / destroy, set_coeffs, set_matrix, the SRS setters
//   transcript  prove_transcript.cuh  host transcript, challenge entries, binding, SRS / circuit hash, dvp_blake3
//   begin       prove_begin.cuh       begin, extend by vector, quotient
//   MSMs        prove_msm.cuh         prover_msm_partial (table budget), the multi-GPU shards, prove_msm, plan / table / budget entries
//   challenge   prove_challenge.cuh   vector stages, device and host challenge, _partial / _finish, dvp_prove_finish
//   check       prove_check.cuh       the witness check (unsatisfied rows, entries >= p, suspect wires) with its own kernels, dvp_prover_row_terms
//   trace       prove_trace.cuh       dvp_prover_trace_last: scalars, partial commitments and vector digests of the last proof
//   multi       prove_multi.cuh       dvp_prove_multi*: one begin, then the rest of a proof once per SRS slot
//   here        dvp_prove_dev and its two flavours, the host-witness entries, dvp_prover_debug_read, the domain-table entries
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "blake3.h"
#include "blake3_dev.cuh"
#include "common.h"
#include "ecfft_internal.h"
#include "fr_wire.cuh"
#include "host_api.h"
#include "k233.cuh"

#include "prove_kernels.cuh"

using namespace dvp;

#include "prove_state.cuh"
#include "prove_slots.cuh"
#include "prove_setup.cuh"
#include "prove_transcript.cuh"
#include "prove_begin.cuh"
#include "prove_msm.cuh"
#include "prove_challenge.cuh"
#include "prove_check.cuh"
#include "prove_trace.cuh"

// Proof::prove with the assignment already resident in HBM (the timed configuration of bench.py)
// Host-transcript flavour (rounds 1-4; still what a device list, n_public > 35 or DVP_PROVE_HOST_TRANSCRIPT=1 gets): the host waits for
// the commitment MSM, hashes, and enqueues the challenge phase.
// Both flavours are begin + rest: dvp_prove_multi_dev (prove_multi.cuh) runs the begin once and the rest once per SRS slot.
// *witness_fault (optional) is set where the failure is the witness's own -- an unsatisfied row, a scalar >= p in the commitment
// MSM -- and not the slot's (alpha in D u D', the K MSM's status).
static int prove_dev_host_rest(dvp_prover* p, ProfScope& ps, uint8_t proof[118], void* stream, bool* witness_fault = nullptr) {
  hipStream_t st = (hipStream_t)stream;
  {
    const int rc = prove_msm(p, 0, p->pts, p->pts_inf32, stream);
    if (witness_fault) *witness_fault = true;
    if (rc == DVP_OK && p->enc_fused[0]) {  // fin_host = [a0 b0 i0 r0 | flags | encodings] as of the MSM's end
      const unsigned long long f0 = p->fin_host->flags[0];
      if (f0 != ~0ull) {
        g_last_error_index = (int64_t)f0;
        return DVP_EUNSAT;
      }
    } else {  // sharded MSM (no block on the host), or an MSM error: the unsatisfied row is reported first, as before
      DVP_TRY(prove_check_unsat(p, st));
      if (witness_fault) *witness_fault = rc == DVP_EINVAL;  // the MSM's scalar-range check; any other status is the slot's
      DVP_TRY(rc);
    }
    if (witness_fault) *witness_fault = false;
  }
  DVP_TRY(dvp_prove_challenge(p, p->pts, p->pts_inf32, stream));
  DVP_TRY(prove_msm(p, 1, p->pts + 1, p->pts_inf32 + 1, stream));
  ps.stop();
  return dvp_prove_finish(p, p->pts + 1, p->pts_inf32 + 1, proof, stream);
}
static int prove_dev_host_transcript(dvp_prover* p, const void* d_assignment, uint8_t proof[118], void* stream) {
  ProfScope ps(PROF_PROVE_TOTAL, (hipStream_t)stream);
  DVP_TRY(prove_begin_impl(p, d_assignment, 1, stream, true));
  return prove_dev_host_rest(p, ps, proof, stream);
}
// Device-transcript flavour (round 5, the default on one device): begin -> commitment MSM (deferred: no final synchronisation, its
// tail kernel leaves commit_p's 30 bytes and its scalar-range word in the prover's block) -> k_transcript -> challenge phase -> K MSM,
// whose own final synchronisation -- the ONE wait of the proof on its stream -- brings the block
// [a0 b0 i0 r0 | flags | commit_p kzg_k | alpha | commitment MSM's word] to the host.  (Inside each MSM the host still reads the largest
// bucket on a side stream while the first pair round runs; that read never idles the GPU.)  Errors are reported in the reference's
// order from that block: unsatisfied row (src/proving.rs:389-395), scalar >= p in the witness (multi_scalar_mul's fr_to_le_bytes),
// alpha in D u D' (:548-556), then the K MSM's own status.
static int prove_dev_device_rest(dvp_prover* p, ProfScope& ps, uint8_t proof[118], void* stream, bool* witness_fault = nullptr) {
  hipStream_t st = (hipStream_t)stream;
  if (witness_fault) *witness_fault = false;
  DVP_TRY(prover_msm_partial(p, 0, 0, dvp_prover_msm_size(p, 0), p->pts, p->pts_inf32, p->blk->enc, stream, p->blk->msm_err));
  // from here on the commitment MSM is in flight on `st` and in its workspace: every error return below drains the stream first
  {
    const int rc_c = challenge_dev(p, st);
    if (rc_c != DVP_OK) {
      (void)hipStreamSynchronize(st);
      return rc_c;
    }
  }
  // the block in pinned host memory still holds the PREVIOUS proof's words: mark the flags so that a K MSM which returns before its
  // copy (plan limits, an allocation failure) is not mistaken for one that brought this proof's block along
  constexpr unsigned long long FIN_STALE = ~0ull - 1;  // the device writes ~0 (fine) or an index < 2^32
  ProverBlock* h = p->fin_host;
  h->flags[0] = h->flags[1] = FIN_STALE;
  const int rc_k = prover_msm_partial(p, 1, 0, dvp_prover_msm_size(p, 1), p->pts + 1, p->pts_inf32 + 1, p->blk->enc + 30, stream);
  ps.stop();
  const int64_t k_idx = g_last_error_index;
  const unsigned long long f[2] = {h->flags[0], h->flags[1]}, e0 = h->msm_err[0];
  if (f[0] == FIN_STALE || f[1] == FIN_STALE) {  // nothing was brought to the host
    (void)hipStreamSynchronize(st);
    g_last_error_index = k_idx;
    return rc_k != DVP_OK ? rc_k : DVP_EHIP;
  }
  memcpy(p->abir0_host, h->abir0, sizeof(h->abir0));
  memcpy(p->commit_p_host, h->enc, 30);
  p->alpha_canon = h->alpha;
  if (witness_fault) *witness_fault = f[0] != ~0ull || e0 != ~0ull;
  if (f[0] != ~0ull) { g_last_error_index = (int64_t)f[0]; return DVP_EUNSAT; }
  if (e0 != ~0ull) { g_last_error_index = (int64_t)(e0 & 0xffffffffull); return DVP_EINVAL; }
  if (f[1] != ~0ull) { g_last_error_index = (int64_t)f[1]; return DVP_ECHALLENGE; }
  if (rc_k != DVP_OK) { g_last_error_index = k_idx; return rc_k; }
  assemble_proof(p, h->enc + 30, proof);
  p->trace_mark();
  return DVP_OK;
}
static int prove_dev_device_transcript(dvp_prover* p, const void* d_assignment, uint8_t proof[118], void* stream) {
  if (!p->shards.empty()) shards_release(p);
  ProfScope ps(PROF_PROVE_TOTAL, (hipStream_t)stream);
  DVP_TRY(prove_begin_impl(p, d_assignment, 1, stream, true, /*pub_to_host=*/false));
  return prove_dev_device_rest(p, ps, proof, stream);
}
// the flavour of a proof on this prover now: the device transcript on one device, up to TRANSCRIPT_DEV_MAX_PUB public inputs
static bool prove_flavour_device(const dvp_prover* p) {
  return mgpu_devices().size() <= 1 && p->n_pub <= TRANSCRIPT_DEV_MAX_PUB && !tune().prove_host_transcript;
}
extern "C" int dvp_prove_dev(dvp_prover* p, const void* d_assignment, uint8_t proof[118], void* stream) {
  if (!p || !d_assignment || !proof) return DVP_EINVAL;
  if (prove_flavour_device(p)) return prove_dev_device_transcript(p, d_assignment, proof, stream);
  return prove_dev_host_transcript(p, d_assignment, proof, stream);
}

// ---- the host-witness seam: the entries below carry no stream argument and run on the prover's own stream ----
static int witness_stream(dvp_prover* p) {
  if (!prover_ready(p)) return DVP_EINVAL;
  if (!p->own_stream) DVP_HIP(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
  return DVP_OK;
}
// assignment = [1, public, private] (src/proving.rs:449-452) into p->w: 32 bytes per element as the caller holds them, the constant wire
// the library's own canonical 1
static int stage_witness(dvp_prover* p, const uint64_t* pub, uint32_t n_public, const uint64_t* prv, uint32_t n_private, const uint8_t* proof) {
  if (!p || !proof || n_public != p->n_pub || 1 + n_public + n_private != p->n_wires) return DVP_EINVAL;
  if ((n_public && !pub) || (n_private && !prv)) return DVP_EINVAL;
  DVP_TRY(witness_stream(p));
  Fr one = fr_one_canon();
  DVP_HIP(hipMemcpyAsync(p->w, &one, sizeof(Fr), hipMemcpyHostToDevice, p->own_stream));
  if (n_public) DVP_HIP(hipMemcpyAsync(p->w + 1, pub, (size_t)n_public * 32, hipMemcpyHostToDevice, p->own_stream));
  if (n_private) DVP_HIP(hipMemcpyAsync(p->w + 1 + n_public, prv, (size_t)n_private * 32, hipMemcpyHostToDevice, p->own_stream));
  DVP_HIP(hipStreamSynchronize(p->own_stream));  // `one` lives on this stack frame, and the caller's buffers are free again on return anyway
  return DVP_OK;
}

// Proof::prove(cache_dir, public_inputs, private_inputs) -> Proof, src/proving.rs:426-688 (host witness).
// proof = commit_p[30] | kzg_k[30] | a0[29 LE] | b0[29 LE]  (the byte image of Proof::to_bits, :691-718)
extern "C" int dvp_prove(dvp_prover* p, const uint64_t* public_inputs, uint32_t n_public, const uint64_t* private_inputs,
                         uint32_t n_private, uint8_t proof[118]) {
  DVP_TRY(stage_witness(p, public_inputs, n_public, private_inputs, n_private, proof));
  return dvp_prove_dev(p, p->w, proof, p->own_stream);
}

// The same from the witness as the file holds it (load_witness_from_file's payload, src/gnark_r1cs.rs:188-211 -> Proof::prove,
// src/dvsnark_test.rs:189-229): n >= n_wires elements of 32 bytes big-endian, unreduced.  dvp_prove step for step, except that the raw
// bytes go into p->w and k_fr_from_be32 (fr_wire.hip) reduces them there, in place: no staging buffer.  The kernel is enqueued behind
// the wait for the copy, so it runs while the host enqueues the proof.  The host looks at element 0 only (it must be the constant 1).
extern "C" int dvp_prove_be32(dvp_prover* p, const uint8_t* witness_be32, size_t n, uint8_t proof[118]) {
  if (!p || !proof || !witness_be32 || n < p->n_wires) return DVP_EINVAL;
  if (!fr_be32_is_one(witness_be32)) {
    g_last_error_index = 0;
    return DVP_EINVAL;
  }
  DVP_TRY(witness_stream(p));
  DVP_HIP(hipMemcpyAsync(p->w, witness_be32, (size_t)p->n_wires * 32, hipMemcpyHostToDevice, p->own_stream));
  DVP_HIP(hipStreamSynchronize(p->own_stream));  // the caller's buffer is free again on return
  DVP_TRY(dvp_fr_from_be32_dev(p->w, p->n_wires, p->w, p->own_stream));
  return dvp_prove_dev(p, p->w, proof, p->own_stream);
}

// dvp_prove with both vectors as arkworks holds them (Proof::prove's Vec<Fr> and &[Fr], src/proving.rs:426-452; four LE u64 of
// a 2^256 mod p each, src/curve.rs:16-22).  dvp_prove step for step, except that k_fr_from_ark (fr_ark.hip) converts elements
// 1 .. n_wires-1 in p->w, in place, in one launch behind the wait for the copy: the kernel runs while the host enqueues the proof, and
// the proof still has one host wait.
extern "C" int dvp_prove_ark(dvp_prover* p, const uint64_t* public_ark, uint32_t n_public, const uint64_t* private_ark, uint32_t n_private,
                             uint8_t proof[118]) {
  DVP_TRY(stage_witness(p, public_ark, n_public, private_ark, n_private, proof));
  DVP_TRY(dvp_fr_from_ark_dev(p->w + 1, (size_t)p->n_wires - 1, p->w + 1, p->own_stream));
  return dvp_prove_dev(p, p->w, proof, p->own_stream);
}

#include "prove_multi.cuh"

// Parity-test access to the intermediates of the last dvp_prove call.  name in:
//  "a","b","c","i" (m each), "a2","b2","c2","i2", "r2", "q2", "ka","kb" (m), "kr" (2m),
//  "alpha","a0","b0","i0","r0" (1), "bar_wts","z_vals2inv","D","D2" (m, canonical)
extern "C" int dvp_prover_debug_read(dvp_prover* p, const char* name, uint64_t* out, size_t n_elems) {
  if (!p || !name || !out) return DVP_EINVAL;
  const size_t m = p->m;
  std::string s(name);
  const Fr* src = nullptr;
  size_t n = m;
  bool mont = false;
  if (s == "a") src = p->E; else if (s == "b") src = p->E + m; else if (s == "c") src = p->E + 2 * m; else if (s == "i") src = p->E + 3 * m;
  else if (s == "a2") src = p->E2; else if (s == "b2") src = p->E2 + m; else if (s == "c2") src = p->E2 + 2 * m; else if (s == "i2") src = p->E2 + 3 * m;
  else if (s == "r2") src = p->r2; else if (s == "q2") src = p->SA + p->n_wires;
  else if (s == "ka") src = p->SK; else if (s == "kb") src = p->SK + m; else if (s == "kr") { src = p->SK + 2 * m; n = 2 * m; }
  else if (s == "bar_wts") { src = p->barw; mont = true; } else if (s == "z_vals2inv") { src = p->z2inv; mont = true; }
  else if (s == "D") { src = p->dD; mont = true; } else if (s == "D2") { src = p->dD2; mont = true; }
  else if (s == "alpha") { if (n_elems != 1) return DVP_EINVAL; memcpy(out, p->alpha_canon.v, 32); return DVP_OK; }
  else if (s == "a0" || s == "b0" || s == "i0" || s == "r0") {
    if (n_elems != 1) return DVP_EINVAL;
    int k = s == "a0" ? 0 : s == "b0" ? 1 : s == "i0" ? 2 : 3;
    DVP_HIP(hipDeviceSynchronize());  // straight from the device: valid after the challenge phase, before finish
    DVP_HIP(hipMemcpy(out, p->blk->abir0 + k, 32, hipMemcpyDeviceToHost));
    return DVP_OK;
  } else return DVP_EINVAL;
  if (n_elems != n) return DVP_EINVAL;
  if (mont) {
    DevBuf tmp;
    DVP_TRY(tmp.alloc(n * sizeof(Fr)));
    DVP_LAUNCH(k_from_mont_vec, dim3(cdiv(n, PT)), dim3(PT), 0, 0, src, tmp.as<Fr>(), n);
    DVP_TRY(tmp.down(out, n * sizeof(Fr)));
  } else {
    DVP_HIP(hipMemcpy(out, src, n * sizeof(Fr), hipMemcpyDeviceToHost));
  }
  return DVP_OK;
}

// Domain tables for setup-side callers (compute_barycentric_weights / evaluate_vanishing_poly_at_domain +
// batch_inversion, src/ec_fft.rs:284-335,407-419): which = 0 -> (1/Z_D'(D), 1/Z_D(D')), which = 1 -> mirrored.
// device flavour (setup.hip): canonical outputs, m = leaves / 2 entries each
int ecfft_domain_tables_dev(dvp_ecfft* t, int which, Fr* d_bar_weights, Fr* d_zinv_other, hipStream_t st) {
  if (!t || !d_bar_weights || !d_zinv_other || (which != 0 && which != 1) || t->log_n < 2) return DVP_EINVAL;
  const size_t m = t->n_leaves / 2;
  const int kk = t->log_n - 1;
  DVP_TRY(ecfft_device_consts(t));
  DVP_LAUNCH(k_domain_tables, dim3(cdiv(m, PT)), dim3(PT), 0, st, t->layer(0), (uint32_t)m, t->d_x0, t->d_t, kk, t->layer(kk),
                     which, d_bar_weights, d_zinv_other);
  DVP_LAUNCH(k_from_mont_vec, dim3(cdiv(m, PT)), dim3(PT), 0, st, d_bar_weights, d_bar_weights, m);
  DVP_LAUNCH(k_from_mont_vec, dim3(cdiv(m, PT)), dim3(PT), 0, st, d_zinv_other, d_zinv_other, m);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}
extern "C" int dvp_ecfft_domain_tables(dvp_ecfft* t, int which, uint64_t* bar_weights, uint64_t* zinv_other) {
  if (!t || !bar_weights || !zinv_other || (which != 0 && which != 1) || t->log_n < 2) return DVP_EINVAL;
  const size_t m = t->n_leaves / 2;
  DevBuf bw, zi;
  DVP_TRY(bw.alloc(m * sizeof(Fr)));
  DVP_TRY(zi.alloc(m * sizeof(Fr)));
  DVP_TRY(ecfft_domain_tables_dev(t, which, bw.as<Fr>(), zi.as<Fr>(), 0));
  DVP_TRY(bw.down(bar_weights, m * sizeof(Fr)));
  return zi.down(zinv_other, m * sizeof(Fr));
}
extern "C" int dvp_prover_domain_tables(dvp_prover* p, int which, uint64_t* bar_weights, uint64_t* zinv_other) {
  if (!p) return DVP_EINVAL;
  return dvp_ecfft_domain_tables(p->tree, which, bar_weights, zinv_other);
}

extern "C" int dvp_prover_domains(dvp_prover* p, uint64_t* d, uint64_t* d2) {
  if (!p || !d || !d2) return DVP_EINVAL;
  DVP_TRY(dvp_prover_debug_read(p, "D", d, p->m));
  return dvp_prover_debug_read(p, "D2", d2, p->m);
}
