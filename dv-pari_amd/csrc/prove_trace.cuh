// The trace of a prover's last proof (dvp_prover_trace_last, include/dvpari.h): scalars, partial commitments and vector digests of
// Proof::prove's stages, read from what a completed proof leaves resident.  Nothing here runs on the proof path: the proof's entries
// only keep dvp_prover::trace_ok (prove_state.cuh: set where a whole proof succeeds; cleared by every begin, by every staged phase entry,
// and by the entries outside a proof that overwrite what is read here -- the witness check reduces into SA, the SRS setters replace bases).
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
//
// Where each field comes from (all vectors canonical, as dvp_prover_debug_read reads them):
//   alpha, Z_D(alpha)        the block's alpha_m and neg_z (Montgomery; written by k_transcript / k_zalpha or copied in by dvp_prove_challenge)
//   a0 b0 i0 r0, encodings   the block's abir0 and enc
//   assignment | q_vals2     SA = [w | q2]: the MSMs take their scalars as const and recode into their own workspace, SA is not rewritten
//   evals.a/b/c/i            E;   evals2.a/b/c/i: E2 -- k_quotient<true> stores the i(d') it evaluates by Horner, so E2's fourth vector is
//                            in place on both routes and nothing has to be re-evaluated here
//   r_vals2                  r2;  denom_invs | denom_invs2: den | den2, inverted in place and only read afterwards
//   k_scalar_a | _b | _r     SK (k_r interleaved [D_i, D'_i], the order of g_k_2)
//   r_vals on D              never materialised (k_kscalars folds a b - i into k_r): not part of the record
// The five partial commitments go through msm_affine_dev, the one-shot MSM, on sub-ranges of the resident bases: no table is built or
// read and no budget consulted, so the proof's own (table) path is checked against an independent one.
#pragma once
#include "prove_challenge.cuh"

static void trace_limbs(uint64_t out[4], const Fr& a) { memcpy(out, a.v, 32); }

extern "C" int dvp_prover_trace_last(dvp_prover* p, uint32_t parts, dvp_prove_trace* out, void* stream) {
  if (!p || !out || !parts || (parts & ~DVP_TRACE_ALL)) return DVP_EINVAL;
  if (!p->trace_ok || mgpu_devices().size() > 1 || !p->shards.empty()) return DVP_EINVAL;
  // commit_p's and kzg_k's encodings were written by the proof, the five partial ones are written here: one rule for all seven
  if (codec_rule_now() != p->trace_rule) return DVP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const size_t m = p->m, nw = p->n_wires;
  memset(out, 0, sizeof *out);
  out->log2_m = p->log_m;
  out->n_wires = p->n_wires;
  out->n_public = p->n_pub;
  out->codec_rule = (uint32_t)codec_rule_now();
  out->parts = parts;

  ProverBlock h;  // a private copy: the pinned mirror belongs to the proof path
  DVP_HIP(hipMemcpyAsync(&h, p->blk, sizeof h, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  if (parts & DVP_TRACE_SCALARS) {
    trace_limbs(out->alpha, fr_from_mont(h.alpha_m));
    trace_limbs(out->z_alpha, fr_from_mont(fr_neg(h.neg_z)));
    trace_limbs(out->a0, h.abir0[0]);
    trace_limbs(out->b0, h.abir0[1]);
    trace_limbs(out->i0, h.abir0[2]);
    trace_limbs(out->r0, h.abir0[3]);
  }

  if (parts & DVP_TRACE_DIGESTS) {
    struct Vec { const Fr* v; size_t n; uint8_t* dst; };
    const Vec vecs[16] = {
        {p->SA, nw, out->assignment},
        {p->E, m, out->evals_a}, {p->E + m, m, out->evals_b}, {p->E + 2 * m, m, out->evals_c}, {p->E + 3 * m, m, out->evals_i},
        {p->E2, m, out->evals2_a}, {p->E2 + m, m, out->evals2_b}, {p->E2 + 2 * m, m, out->evals2_c}, {p->E2 + 3 * m, m, out->evals2_i},
        {p->r2, m, out->r_vals2}, {p->SA + nw, m, out->q_vals2},
        {p->den, m, out->denom_invs}, {p->den2, m, out->denom_invs2},
        {p->SK, m, out->k_scalar_a}, {p->SK + m, m, out->k_scalar_b}, {p->SK + 2 * m, 2 * m, out->k_scalar_r},
    };
    DevBuf work, dig;  // one scratch for all sixteen: they run one after the other on st
    DVP_TRY(work.alloc(fr_digest_work_bytes(std::max(nw, 2 * m))));
    DVP_TRY(dig.alloc(16 * 32));
    for (int k = 0; k < 16; ++k) DVP_TRY(fr_vec_digest_dev(vecs[k].v, vecs[k].n, false, work.p, dig.as<uint32_t>() + 8 * k, st));
    uint8_t hd[16 * 32];
    DVP_HIP(hipMemcpyAsync(hd, dig.p, sizeof hd, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 16; ++k) memcpy(vecs[k].dst, hd + 32 * k, 32);
  }

  if (parts & DVP_TRACE_POINTS) {
    // device: 9 points of 64 bytes (0..4 the partial commitments, 5 and 6 the two sums, 7 and 8 the proof's own), their 9 flags, and
    // the 5 encodings of the partial commitments at a stride of 32 bytes
    constexpr size_t OFF_INF = 9 * 64, OFF_ENC = OFF_INF + 64, BYTES = OFF_ENC + 5 * 32;
    DevBuf d;
    DVP_TRY(d.alloc(BYTES));
    DVP_HIP(hipMemsetAsync(d.p, 0, BYTES, st));
    Aff* pt = d.as<Aff>();
    uint32_t* inf = (uint32_t*)((char*)d.p + OFF_INF);
    uint8_t* enc = (uint8_t*)d.p + OFF_ENC;
    struct Part { const Fr* sc; const Aff* bs; const uint8_t* inf; size_t n; };
    const Part part[5] = {
        {p->SA, p->bases_a, p->inf_a, nw},
        {p->SA + nw, p->bases_a + nw, p->inf_a + nw, m},
        {p->SK, p->bases_k, p->inf_k, m},
        {p->SK + m, p->bases_k + m, p->inf_k + m, m},
        {p->SK + 2 * m, p->bases_k + 2 * m, p->inf_k + 2 * m, 2 * m},
    };
    for (int k = 0; k < 5; ++k) {
      DVP_TRY(msm_affine_dev(part[k].sc, part[k].bs, part[k].inf, part[k].n, MsmOut{pt + k, inf + k}, st));
      DVP_TRY(encode_point_dev(pt + k, inf + k, enc + 32 * k, st));
    }
    DVP_TRY(msm_sum_points_dev(pt, 64, inf, 2, 1, pt + 5, inf + 5, st));
    DVP_TRY(msm_sum_points_dev(pt + 2, 64, inf + 2, 3, 1, pt + 6, inf + 6, st));
    DVP_HIP(hipMemcpyAsync(pt + 7, p->pts, 2 * sizeof(Aff), hipMemcpyDeviceToDevice, st));
    DVP_HIP(hipMemcpyAsync(inf + 7, p->pts_inf32, 8, hipMemcpyDeviceToDevice, st));
    uint8_t hb[BYTES];
    DVP_HIP(hipMemcpyAsync(hb, d.p, BYTES, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipStreamSynchronize(st));
    const uint32_t* hinf = (const uint32_t*)(hb + OFF_INF);
    auto fill = [&](dvp_trace_point* t, int slot, const uint8_t* e30) {
      t->inf = hinf[slot] ? 1 : 0;
      if (!t->inf) memcpy(t->xy, hb + 64 * slot, 64);
      memcpy(t->enc, e30, 30);
    };
    dvp_trace_point* dst[5] = {&out->msm_gm, &out->msm_q, &out->kzg_a, &out->kzg_b, &out->kzg_r};
    for (int k = 0; k < 5; ++k) fill(dst[k], k, hb + OFF_ENC + 32 * k);
    fill(&out->commit_p, 7, h.enc);
    fill(&out->kzg_k, 8, h.enc + 30);
    auto same = [&](int a, int b) {
      const bool ia = hinf[a] != 0, ib = hinf[b] != 0;
      return ia == ib && (ia || !memcmp(hb + 64 * a, hb + 64 * b, 64));
    };
    if (!same(5, 7)) out->mismatch |= DVP_TRACE_MISMATCH_COMMIT;
    if (!same(6, 8)) out->mismatch |= DVP_TRACE_MISMATCH_KZG;
  }
  return DVP_OK;
}
