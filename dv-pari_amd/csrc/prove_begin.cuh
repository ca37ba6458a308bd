// Phase 1 of a proof: begin, the extends by vector, the quotient.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
#pragma once
#include "prove_state.cuh"

// ---- Proof::prove in phases ------------------------------------------------------------------------
// The two MSMs are the only stages that shard across GPUs, so prove is exposed as
//   begin -> [commitment MSM, possibly partial per rank] -> challenge -> [K MSM] -> finish
// and dvp_prove / dvp_prove_dev run the phases back to back on one device.

// vectors a proof extends: a, b, c', and i unless its few coefficients make Horner on D' cheaper (k_quotient<HORNER>).
// Horner is the extend's value only while i(X) has degree < m: with n_pub > m the reference extends the m evaluations of i on D
// (src/proving.rs:369-376, 415), i.e. the interpolant of degree < m, which is NOT i on D' -- so such a circuit always extends i,
// whatever the knob says, and gets the reference's proof (one its verifier rejects).  This is the ONE place the route is chosen:
// the extends by vector, the quotient, dvp_prove_multi* and the trace's digests all follow it.
static uint32_t prover_n_ext(const dvp_prover* p) {
  uint32_t hmax = HORNER_MAX_PUB;
  if (tune().horner_max_pub >= 0) hmax = (uint32_t)tune().horner_max_pub;  // tests force either route
  return p->n_pub <= hmax && p->n_pub <= p->m ? 3u : 4u;
}
// the host's look at the unsatisfied-row flag (assert_eq!(a*b, c+i), src/proving.rs:389-395)
static int prove_check_unsat(dvp_prover* p, hipStream_t st) {
  unsigned long long f0[2];
  DVP_HIP(hipMemcpyAsync(f0, p->blk->flags, 16, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  count_host_wait(0);
  if (f0[0] != ~0ull) {
    g_last_error_index = (int64_t)f0[0];
    return DVP_EUNSAT;
  }
  return DVP_OK;
}
// defer_unsat (dvp_prove_dev only): the flag is NOT waited for here -- the commitment MSM does not need the host to know it, and its
// own final synchronisation brings the flag block along (one host round trip less per proof; an unsatisfied witness then costs an
// MSM before it is reported)
static int prove_begin_impl(dvp_prover* p, const void* d_assignment, int need_extend, void* stream, bool defer_unsat, bool pub_to_host = true) {
  if (!p || !d_assignment || !prover_ready(p)) return DVP_EINVAL;
  p->last_begin_extended = false;  // set by dvp_prove_quotient once every extended vector is in place
  p->ext_filled = 0;
  p->trace_ok = p->challenge_sliced = false;
  p->enc_fused[0] = p->enc_fused[1] = false;  // a staged caller may have abandoned a proof after an MSM into the prover's own slot
  hipStream_t st = (hipStream_t)stream;
  const uint32_t m = p->m;
  const size_t nw = p->n_wires;
  // the witness goes straight into the scalar vector of the first MSM, [w | q2], and every stage reads it there (p->w is only the
  // staging buffer of the host-pointer seam): one 32 B / wire copy per proof instead of two
  if (d_assignment != p->SA) DVP_HIP(hipMemcpyAsync(p->SA, d_assignment, nw * sizeof(Fr), hipMemcpyDeviceToDevice, st));
  p->pub_host.resize((size_t)p->n_pub * 4);
  if (p->n_pub && pub_to_host) DVP_HIP(hipMemcpyAsync(p->pub_host.data(), p->SA + 1, (size_t)p->n_pub * 32, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipMemsetAsync(p->blk->flags, 0xff, 16, st));
  Csr A{p->mat[0].row_ptr, p->mat[0].wire, p->mat[0].coeff, p->mat[0].n_rows};
  Csr B{p->mat[1].row_ptr, p->mat[1].wire, p->mat[1].coeff, p->mat[1].n_rows};
  Csr C{p->mat[2].row_ptr, p->mat[2].wire, p->mat[2].coeff, p->mat[2].n_rows};
  dim3 gm(cdiv(m, PT)), bt(PT);
  DVP_LAUNCH(k_r1cs_eval, gm, bt, 0, st, A, B, C, p->coeffs_m, p->SA, p->dD, p->n_pub, m, p->E, p->blk->flags);
  DVP_HIP(hipGetLastError());
  if (need_extend) {
    DVP_TRY(dvp_prove_extend_vectors(p, (1u << prover_n_ext(p)) - 1, stream));
    DVP_TRY(dvp_prove_quotient(p, stream));
  }
  if (defer_unsat) return DVP_OK;
  return prove_check_unsat(p, st);
}
// phase 1 (src/proving.rs:434-508): assignment -> a,b,c',i -> extend -> q2; leaves SA = [w | q2].
// d_assignment: n_wires canonical Fr = [1, public.., private..] already in HBM.
extern "C" int dvp_prove_begin(dvp_prover* p, const void* d_assignment, void* stream) {
  return dvp_prove_begin_partial(p, d_assignment, 1, stream);
}
// need_extend == 0: the caller's MSM shards lie inside [w] and [k_a | k_b] only, which need neither q2 nor r2, so the
// three extends and the quotient are skipped (multi-GPU load balancing, distributed.py::shard_plan).  q2 / r2 and the
// k_r part of the second MSM's scalars are then NOT valid on this prover until the next full begin.
extern "C" int dvp_prove_begin_partial(dvp_prover* p, const void* d_assignment, int need_extend, void* stream) {
  return prove_begin_impl(p, d_assignment, need_extend, stream, false);
}

// ---- the extends by VECTOR (option A) ------------------------------------------------------------------------
// The extends of a, b, c' (and i, when it is not evaluated by Horner) are independent (src/proving.rs:410-422), so the ranks
// of a multi-process prove that need q2 / r2 each extend only the vectors of `mask` (bit v = vector v of [a, b, c', i]),
// exchange the extended vectors (distributed.py: one broadcast per vector inside the extender group, straight out of and
// into dvp_prover_extended_ptr) and then run the quotient.  dvp_prove_begin_partial(need_extend = 1) is
// begin(need_extend = 0) + extend_vectors(all) + quotient.
extern "C" uint32_t dvp_prover_extend_count(const dvp_prover* p) { return p ? prover_n_ext(p) : 0; }
extern "C" int dvp_prover_extended_ptr(dvp_prover* p, uint32_t v, void** d_ptr) {
  if (!p || v > 3 || !d_ptr) return DVP_EINVAL;
  *d_ptr = p->E2 + (size_t)v * p->m;
  return DVP_OK;
}
extern "C" int dvp_prove_extend_vectors(dvp_prover* p, uint32_t mask, void* stream) {
  if (!p || !prover_ready(p)) return DVP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t m = p->m, n_ext = prover_n_ext(p);
  if (mask >> n_ext) return DVP_EINVAL;
  p->trace_ok = false;  // E2 is rewritten
  // runs of consecutive selected vectors share one batched extend (the matrices are read once per run)
  for (uint32_t v = 0; v < n_ext;) {
    if (!((mask >> v) & 1)) { ++v; continue; }
    uint32_t e = v;
    while (e < n_ext && ((mask >> e) & 1)) ++e;
    ProfScope pe(PROF_EXTEND_TOTAL, st);
    DVP_TRY(extend_from(p->tree, 0, 0, p->E + (size_t)v * m, p->E2 + (size_t)v * m, e - v, st));  // E (a, b, c' on D) stays as it is
    pe.stop();
    v = e;
  }
  p->ext_filled |= mask;
  return DVP_OK;
}
// extended vector v of the CURRENT proof has been written into dvp_prover_extended_ptr(v) by the caller (a broadcast from the
// rank that extended it): dvp_prove_quotient refuses to run until every vector is either extended here or marked
extern "C" int dvp_prove_mark_extended(dvp_prover* p, uint32_t v) {
  if (!p || v >= prover_n_ext(p)) return DVP_EINVAL;
  p->ext_filled |= 1u << v;
  return DVP_OK;
}
// r2 = a2 b2 - i2, q2 = (r2 - c2) / Z_D on D' (src/proving.rs:492-508) from the extended vectors in place
extern "C" int dvp_prove_quotient(dvp_prover* p, void* stream) {
  if (!p || !prover_ready(p)) return DVP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t m = p->m;
  const size_t nw = p->n_wires;
  if (p->ext_filled != (1u << prover_n_ext(p)) - 1) return DVP_EINVAL;  // a missed broadcast would otherwise give a silently wrong q2
  p->trace_ok = false;  // r2, q2 and (by Horner) E2's fourth vector are rewritten
  dim3 gm(cdiv(m, PT)), bt(PT);
  if (prover_n_ext(p) == 3)
    DVP_LAUNCH(k_quotient<true>, gm, bt, 0, st, p->E2, p->z2inv, m, p->SA, p->dD2, p->n_pub, p->r2, p->SA + nw);
  else
    DVP_LAUNCH(k_quotient<false>, gm, bt, 0, st, p->E2, p->z2inv, m, p->SA, p->dD2, p->n_pub, p->r2, p->SA + nw);
  DVP_HIP(hipGetLastError());
  p->last_begin_extended = true;
  return DVP_OK;
}
