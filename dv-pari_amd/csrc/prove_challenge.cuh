// Phases 2 and 3 of a proof: the challenge phase's vector stages, its device and host flavours, the index-sharded _partial / _finish,
// and dvp_prove_finish.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
#pragma once
#include "prove_transcript.cuh"

// the vector stages of the challenge phase (src/proving.rs:561-654) once alpha (Montgomery) is in the block's alpha_m: denominators,
// one batch inversion over D and D', the three barycentric sums, a0 b0 i0 r0, the K scalars.  -Z_D(alpha) (the block's neg_z) is needed
// by k_bary3_final only: the host flavour copies it in with alpha; the device flavour computes it on the prover's side stream
// meanwhile (z_on_side_stream: the stream joins the side stream in front of k_bary3_final).
static int challenge_vector_stages(dvp_prover* p, hipStream_t st, bool z_on_side_stream) {
  const uint32_t m = p->m;
  dim3 gm(cdiv(m, PT)), bt(PT);
  DVP_LAUNCH(k_alpha_denoms, gm, bt, 0, st, p->dD, p->dD2, &p->blk->alpha_m, m, p->den, p->den2, p->blk->flags + 1);
  DVP_TRY(batch_inverse_dev(p->den, 2 * (size_t)m, st));  // den2 = den + m
  uint32_t nb = cdiv(m, PT);
  if (nb > 1024) nb = 1024;
  DVP_LAUNCH(k_bary3_partial_range, dim3(nb), bt, 0, st, p->E, p->barw, p->den, m, 0u, m, p->partial);
  if (z_on_side_stream) DVP_HIP(hipStreamWaitEvent(st, p->ev_negz, 0));
  DVP_LAUNCH(k_bary3_final, dim3(1), bt, 0, st, p->partial, nb, &p->blk->neg_z, p->blk->abir0);
  DVP_LAUNCH(k_kscalars, gm, bt, 0, st, p->E, p->r2, p->den, p->den2, p->blk->abir0, m, p->SK);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}
// the same phase with the transcript on the device: commit_p's 30 bytes are where the commitment MSM's tail kernel wrote them
// (the block's enc), the public inputs in the witness vector; no host round trip
static int challenge_dev(dvp_prover* p, hipStream_t st) {
  if (p->alpha_forced) {  // dvp_prover_debug_force_alpha: the pair where k_transcript would have left it (the prover outlives the copies)
    DVP_HIP(hipMemcpyAsync(&p->blk->alpha, &p->alpha_forced_pair[0], sizeof(Fr), hipMemcpyHostToDevice, st));
    DVP_HIP(hipMemcpyAsync(&p->blk->alpha_m, &p->alpha_forced_pair[1], sizeof(Fr), hipMemcpyHostToDevice, st));
  } else {
    DVP_LAUNCH(k_transcript, dim3(1), dim3(64), 0, st, (const uint32_t*)p->blk->enc, p->SA + 1, p->n_pub, p->h_ct, &p->blk->alpha, &p->blk->alpha_m);
  }
  DVP_HIP(hipEventRecord(p->ev_alpha, st));
  DVP_HIP(hipStreamWaitEvent(p->side, p->ev_alpha, 0));
  DVP_LAUNCH(k_zalpha, dim3(1), dim3(64), 0, p->side, &p->blk->alpha_m, p->tree->d_x0, p->tree->d_t, (int)p->log_m, p->tree->layer((int)p->log_m),
                     &p->blk->neg_z);
  DVP_HIP(hipEventRecord(p->ev_negz, p->side));
  return challenge_vector_stages(p, st, /*z_on_side_stream=*/true);
}

// commitment -> alpha on the host, for both host flavours of phase 2: the commitment into the prover's slot, its 30 bytes (from the MSM's
// fused encoding, or encoded here at the price of ONE host wait), the transcript.  Sets alpha_canon; *alpha_m = alpha (Montgomery),
// *neg_z = -Z_D(alpha) (Montgomery).
static int challenge_alpha_host(dvp_prover* p, const void* d_commit_xy, const void* d_commit_inf, hipStream_t st, Fr* alpha_m, Fr* neg_z) {
  if (d_commit_xy != p->pts) DVP_HIP(hipMemcpyAsync(p->pts, d_commit_xy, sizeof(Aff), hipMemcpyDeviceToDevice, st));
  if (d_commit_inf != p->pts_inf32) DVP_HIP(hipMemcpyAsync(p->pts_inf32, d_commit_inf, 4, hipMemcpyDeviceToDevice, st));
  if (d_commit_xy == p->pts && d_commit_inf == p->pts_inf32 && p->enc_fused[0]) {
    memcpy(p->commit_p_host, p->fin_host->enc, 30);  // encoded by the MSM's tail, on the host since the MSM's own sync
  } else {
    DVP_TRY(encode_point_dev(p->pts, p->pts_inf32, p->blk->enc, st));
    DVP_HIP(hipMemcpyAsync(p->commit_p_host, p->blk->enc, 30, hipMemcpyDeviceToHost, st));
    DVP_HIP(hipStreamSynchronize(st));
    count_host_wait(0);
  }
  p->enc_fused[0] = false;
  uint8_t ch[32];
  transcript_challenge(p->commit_p_host, p->pub_host.data(), p->n_pub, (const uint8_t*)p->h_ct.w, ch);
  Fr alpha;
  (void)fr_load(ch, &alpha);  // 224 bits: always below p
  if (p->alpha_forced) alpha = p->alpha_forced_pair[0];  // dvp_prover_debug_force_alpha
  p->alpha_canon = alpha;
  *alpha_m = fr_to_mont(alpha);
  *neg_z = fr_neg(host_vanish(p, 0, *alpha_m));
  return DVP_OK;
}

// phase 2 (src/proving.rs:515-654): commit_p -> alpha -> a0,b0,i0,r0 -> K scalars SK.
extern "C" int dvp_prove_challenge(dvp_prover* p, const void* d_commit_xy, const void* d_commit_inf, void* stream) {
  if (!p || !d_commit_xy || !d_commit_inf) return DVP_EINVAL;
  p->trace_ok = false;  // den, SK and the block are rewritten: dvp_prove_finish marks the proof again
  hipStream_t st = (hipStream_t)stream;
  ProverBlock* h = p->fin_host;  // its (alpha_m, neg_z) are pinned staging, rewritten only after this proof's final synchronisation
  DVP_TRY(challenge_alpha_host(p, d_commit_xy, d_commit_inf, st, &h->alpha_m, &h->neg_z));
  DVP_HIP(hipMemcpyAsync(&p->blk->alpha_m, &h->alpha_m, 2 * sizeof(Fr), hipMemcpyHostToDevice, st));  // alpha_m and neg_z
  return challenge_vector_stages(p, st, /*z_on_side_stream=*/false);
}

// ---- phase 2 for index-sharded provers (one process per GPU; SURVEY 8e "pointwise / batch-inverse / barycentric": slice by
// index, all-gather of the partial Fr sums + local add, batch inversion per shard) ------------------------------------------
// part 1: alpha from the commitment; 1/(d - alpha) only where this rank needs it -- its slice [d_lo, d_hi) of the barycentric
// sums and the part of D / D' its K-scalar range [k_lo, k_hi) reads -- and the rank's 128-byte record: three partial sums
// (Montgomery) + its alpha-in-domain flag.  part 2 (after the ranks exchanged their records, any order): a0 b0 i0 r0 from
// the n records, then the K scalars of [k_lo, k_hi) only.  dvp_prove_challenge == part 1 over everything + part 2 on the own
// record; the rest of S and of den / den2 is NOT valid on this prover afterwards.
extern "C" int dvp_prove_challenge_partial(dvp_prover* p, const void* d_commit_xy, const void* d_commit_inf, size_t d_lo, size_t d_hi,
                                           size_t k_lo, size_t k_hi, void* d_record_out, void* stream) {
  if (!p || !d_commit_xy || !d_commit_inf || !d_record_out) return DVP_EINVAL;
  const uint32_t m = p->m;
  if (d_lo > d_hi || d_hi > m || k_lo > k_hi || k_hi > 4 * (size_t)m) return DVP_EINVAL;
  p->challenge_sliced = true;
  p->trace_ok = false;
  hipStream_t st = (hipStream_t)stream;
  dim3 bt(PT);
  Fr alpha_m;
  DVP_TRY(challenge_alpha_host(p, d_commit_xy, d_commit_inf, st, &alpha_m, &p->neg_z_alpha_m));
  // index intervals of D whose inverse denominators this rank reads: its barycentric slice, k_a, k_b and the even half of
  // k_r ([D_i, D'_i] interleaved); of D': the odd half of k_r.  Overlaps are merged (inverting twice would undo it).
  std::vector<std::pair<size_t, size_t>> iv;
  auto clip = [&](size_t a, size_t b, size_t base) {  // [k_lo, k_hi) n [a, b), rebased
    size_t lo = std::max(k_lo, a), hi = std::min(k_hi, b);
    return lo < hi ? std::make_pair(lo - base, hi - base) : std::make_pair((size_t)0, (size_t)0);
  };
  iv.push_back({d_lo, d_hi});
  iv.push_back(clip(0, m, 0));
  iv.push_back(clip(m, 2 * (size_t)m, m));
  std::pair<size_t, size_t> kr = clip(2 * (size_t)m, 4 * (size_t)m, 2 * (size_t)m);
  std::pair<size_t, size_t> kri = {kr.first >> 1, (kr.second + 1) >> 1};
  if (kr.first == kr.second) kri = {0, 0};
  iv.push_back(kri);
  std::sort(iv.begin(), iv.end());
  std::vector<std::pair<size_t, size_t>> merged;
  for (auto& x : iv) {
    if (x.first == x.second) continue;
    if (!merged.empty() && x.first <= merged.back().second) merged.back().second = std::max(merged.back().second, x.second);
    else merged.push_back(x);
  }
  for (auto& x : merged) {
    const uint32_t cnt = (uint32_t)(x.second - x.first);
    DVP_LAUNCH(k_alpha_denoms_range, dim3(cdiv(cnt, PT)), bt, 0, st, p->dD, alpha_m, (uint32_t)x.first, (uint32_t)x.second, p->den, p->blk->flags + 1);
    DVP_TRY(batch_inverse_dev(p->den + x.first, cnt, st));
  }
  if (kri.first < kri.second) {
    const uint32_t cnt = (uint32_t)(kri.second - kri.first);
    DVP_LAUNCH(k_alpha_denoms_range, dim3(cdiv(cnt, PT)), bt, 0, st, p->dD2, alpha_m, (uint32_t)kri.first, (uint32_t)kri.second, p->den2, p->blk->flags + 1);
    DVP_TRY(batch_inverse_dev(p->den2 + kri.first, cnt, st));
  }
  uint32_t nb = 0;
  if (d_lo < d_hi) {
    nb = cdiv((uint32_t)(d_hi - d_lo), PT);
    if (nb > 1024) nb = 1024;
    DVP_LAUNCH(k_bary3_partial_range, dim3(nb), bt, 0, st, p->E, p->barw, p->den, m, (uint32_t)d_lo, (uint32_t)d_hi, p->partial);
  }
  DVP_LAUNCH(k_bary3_record, dim3(1), bt, 0, st, p->partial, nb, p->blk->flags + 1, (Fr*)d_record_out);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}
extern "C" int dvp_prove_challenge_finish(dvp_prover* p, const void* d_records, uint32_t n_records, size_t k_lo, size_t k_hi, void* stream) {
  if (!p || !d_records || !n_records) return DVP_EINVAL;
  const uint32_t m = p->m;
  if (k_lo > k_hi || k_hi > 4 * (size_t)m) return DVP_EINVAL;
  p->trace_ok = false;
  hipStream_t st = (hipStream_t)stream;
  DVP_LAUNCH(k_bary3_from_records, dim3(1), dim3(64), 0, st, (const Fr*)d_records, n_records, p->neg_z_alpha_m, p->blk->abir0, p->blk->flags + 1);
  if (k_lo < k_hi)
    DVP_LAUNCH(k_kscalars_range, dim3(cdiv(k_hi - k_lo, PT)), dim3(PT), 0, st, p->E, p->r2, p->den, p->den2, p->blk->abir0, m, k_lo, k_hi, p->SK);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

// proof = commit_p | kzg_k | a0 | b0 (the byte image of Proof::to_bits, src/proving.rs:691-718) from the prover's host copies
static void assemble_proof(const dvp_prover* p, const uint8_t kzg30[30], uint8_t proof[118]) {
  memcpy(proof, p->commit_p_host, 30);
  memcpy(proof + 30, kzg30, 30);
  memcpy(proof + 60, p->abir0_host[0].v, 29);  // FrBits::from_fr(a0): 232 LE bits, src/curve.rs:30-40
  memcpy(proof + 89, p->abir0_host[1].v, 29);
}

// phase 3 (src/proving.rs:682-687): kzg_k -> bytes; proof = commit_p | kzg_k | a0 | b0.
extern "C" int dvp_prove_finish(dvp_prover* p, const void* d_kzg_xy, const void* d_kzg_inf, uint8_t proof[118], void* stream) {
  if (!p || !d_kzg_xy || !d_kzg_inf || !proof) return DVP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (d_kzg_xy != p->pts + 1) DVP_HIP(hipMemcpyAsync(p->pts + 1, d_kzg_xy, sizeof(Aff), hipMemcpyDeviceToDevice, st));
  if (d_kzg_inf != p->pts_inf32 + 1) DVP_HIP(hipMemcpyAsync(p->pts_inf32 + 1, d_kzg_inf, 4, hipMemcpyDeviceToDevice, st));
  if (!(d_kzg_xy == p->pts + 1 && d_kzg_inf == p->pts_inf32 + 1 && p->enc_fused[1])) {
    DVP_TRY(encode_point_dev(p->pts + 1, p->pts_inf32 + 1, p->blk->enc + 30, st));
    DVP_HIP(hipMemcpyAsync(p->fin_host, p->blk, FIN_BYTES, hipMemcpyDeviceToHost, st));  // pinned: one DMA, no staging
    DVP_HIP(hipStreamSynchronize(st));
    count_host_wait(0);
  }  // else: the K MSM's tail encoded kzg_k and fin_host was filled before that MSM's final sync (a0 b0 i0 r0 and the flags were final by then)
  p->enc_fused[1] = false;
  const ProverBlock* h = p->fin_host;
  memcpy(p->abir0_host, h->abir0, sizeof(h->abir0));
  if (h->flags[1] != ~0ull) {
    g_last_error_index = (int64_t)h->flags[1];
    return DVP_ECHALLENGE;  // alpha in D u D', src/proving.rs:548-556
  }
  assemble_proof(p, h->enc + 30, proof);
  if (p->last_begin_extended && !p->challenge_sliced) p->trace_mark();
  return DVP_OK;
}
