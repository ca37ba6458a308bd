// The host transcript and the hash entries: transcript_challenge, the challenge entries, the binding setter, the SRS and circuit hashes,
// the parity-test access to the device transcript, dvp_blake3.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
#pragma once
#include "prove_state.cuh"

// Transcript::output, src/proving.rs:164-197; h_ct = H(srs_hash || circuit_hash) (b3::compile_hash: hashes of EMPTY buffers in the
// reference, :86-105,113-132)
static void transcript_challenge(const uint8_t commit_p[30], const uint64_t* pub, uint32_t npub, const uint8_t h_ct[32], uint8_t out32[32]) {
  uint8_t h_wc[32], h_pi[32], h_rt[32], buf[64];
  b3::hash(commit_p, 30, h_wc);
  std::vector<uint8_t> pi((size_t)npub * 29);
  for (uint32_t j = 0; j < npub; ++j) memcpy(pi.data() + 29 * (size_t)j, (const uint8_t*)(pub + 4 * (size_t)j), 29);
  b3::hash(pi.data(), pi.size(), h_pi);
  memcpy(buf, h_wc, 32); memcpy(buf + 32, h_pi, 32);
  b3::hash(buf, 64, h_rt);
  memcpy(buf, h_ct, 32); memcpy(buf + 32, h_rt, 32);
  b3::hash(buf, 64, out32);
  out32[28] = out32[29] = out32[30] = out32[31] = 0;  // 224-bit challenge
}

extern "C" int dvp_transcript_challenge(const uint8_t commit_p[30], const uint64_t* public_inputs, uint32_t n_public, uint64_t out[4]) {
  if (!commit_p || (n_public && !public_inputs) || !out) return DVP_EINVAL;
  return dvp_transcript_challenge_bound(commit_p, public_inputs, n_public, nullptr, nullptr, out);
}
extern "C" int dvp_transcript_challenge_bound(const uint8_t commit_p[30], const uint64_t* public_inputs, uint32_t n_public,
                                              const uint8_t srs_hash[32], const uint8_t circuit_hash[32], uint64_t out[4]) {
  if (!commit_p || (n_public && !public_inputs) || !out) return DVP_EINVAL;
  uint8_t h_ct[32], h[32];
  b3::compile_hash(srs_hash, circuit_hash, h_ct);
  transcript_challenge(commit_p, public_inputs, n_public, h_ct, h);
  memcpy(out, h, 32);
  return DVP_OK;
}
extern "C" int dvp_prover_set_transcript_binding(dvp_prover* p, const uint8_t srs_hash[32], const uint8_t circuit_hash[32]) {
  if (!p) return DVP_EINVAL;
  uint8_t h[32];
  b3::compile_hash(srs_hash, circuit_hash, h);
  memcpy(p->h_ct.w, h, 32);
  return DVP_OK;
}

// BLAKE3 of the stream the commented-out loop of Transcript::srs_hash would build (src/proving.rs:91-101): to_bytes() of g_k[0], g_k[1],
// g_k[2], g_q, g_m -- on the device encode_dev over bases_k[0, 4m), bases_a[n_wires, n_wires + m), bases_a[0, n_wires).  The stream
// (1.3 GB at 2^23 constraints) is never materialised: it is encoded into a window of whole points AND whole chunks (a multiple of
// lcm(30, 1024) = 15360 bytes), each window's chunks are hashed with their position in the stream as the counter base, and the chaining
// values are reduced once.  Reads the home device's copies, which shards_build leaves in place: the hash does not depend on the device list.
static constexpr size_t SRS_HASH_WINDOW_POINTS = (size_t)512 * 4096;  // 60 MiB of encodings = 61440 chunks: 960 waves of k_b3_leaves
extern "C" int dvp_prover_srs_hash(dvp_prover* p, uint8_t out[32]) {
  if (!p || !out) return DVP_EINVAL;
  for (int k = 0; k < 5; ++k)
    if (!p->have_srs[k]) return DVP_EINVAL;
  const size_t m = p->m, nw = p->n_wires;
  struct Seg { const Aff* b; const uint8_t* inf; size_t n; };
  const Seg seg[3] = {{p->bases_k, p->inf_k, 4 * m}, {p->bases_a + nw, p->inf_a + nw, m}, {p->bases_a, p->inf_a, nw}};
  const size_t total_pts = 5 * m + nw, total_bytes = 30 * total_pts, nchunks = (total_bytes + 1023) / 1024;
  const size_t win_pts = std::min(SRS_HASH_WINDOW_POINTS, total_pts);
  hipStream_t st = nullptr;
  DevBuf win, cvs, tmp, dout;
  DVP_TRY(win.alloc(win_pts * 30));
  DVP_TRY(dout.alloc(32));
  if (nchunks > 1) {
    DVP_TRY(cvs.alloc(nchunks * 32));
    DVP_TRY(tmp.alloc(b3_reduce_tmp_bytes(nchunks)));
  }
  for (size_t lo = 0; lo < total_pts; lo += win_pts) {
    const size_t hi = std::min(lo + win_pts, total_pts);
    size_t s0 = 0;  // first stream index of segment k
    for (int k = 0; k < 3; s0 += seg[k].n, ++k) {
      const size_t a = std::max(lo, s0), b = std::min(hi, s0 + seg[k].n);
      if (a < b) DVP_TRY(encode_dev(seg[k].b + (a - s0), seg[k].inf + (a - s0), b - a, win.as<uint8_t>() + 30 * (a - lo), st));
    }
    if (nchunks == 1) DVP_TRY(b3_single_chunk_dev(win.as<uint8_t>(), total_bytes, dout.as<uint32_t>(), st));
    else DVP_TRY(b3_leaves_dev(win.as<uint8_t>(), 30 * (hi - lo), 30 * lo / 1024, cvs.as<uint32_t>() + 8 * (30 * lo / 1024), st));
  }
  if (nchunks > 1) DVP_TRY(b3_reduce_dev(cvs.as<uint32_t>(), nchunks, tmp.as<uint32_t>(), dout.as<uint32_t>(), st));
  DVP_HIP(hipMemcpyAsync(out, dout.p, 32, hipMemcpyDeviceToHost, st));
  DVP_HIP(hipStreamSynchronize(st));
  return DVP_OK;
}

// BLAKE3 of the stream the commented-out body of Transcript::circuit_info_hash would build (src/proving.rs:111-134) on the instance after
// update_to_include_vandermode_matrix_d (src/gnark_r1cs.rs:333-386): generated from mat[], coeffs_m and dD by circuit_hash.hip, which
// states the stream.  Needs no SRS; the matrix conditions are prover_ready's.
extern "C" int dvp_prover_circuit_hash(dvp_prover* p, uint8_t out[32]) {
  if (!p || !out) return DVP_EINVAL;
  if (!(p->coeffs_m && p->mat[0].row_ptr && p->mat[1].row_ptr && p->mat[2].row_ptr)) return DVP_EINVAL;
  ChCsr mats;
  uint64_t nnz[3];
  for (int k = 0; k < 3; ++k) {
    if (p->mat[k].nnz && p->mat[k].max_coeff_id >= p->n_coeffs) return DVP_EINVAL;
    mats.rp[k] = p->mat[k].row_ptr;
    mats.cid[k] = p->mat[k].coeff;
    mats.n_rows[k] = p->mat[k].n_rows;
    nnz[k] = p->mat[k].nnz;
  }
  return circuit_hash_dev(mats, nnz, p->coeffs_m, p->n_coeffs, p->dD, p->m, p->n_pub, tune().circuit_hash_window, out, nullptr);
}

// parity-test access to the DEVICE flavour of the transcript (k_transcript, k_zalpha) on caller-supplied inputs: alpha (canonical) and
// -Z_D(alpha) (canonical) for this prover's domain, to be compared with dvp_transcript_challenge / the oracle
extern "C" int dvp_prover_debug_transcript_dev(dvp_prover* p, const uint8_t commit_p[30], const uint64_t* public_inputs, uint32_t n_public,
                                               uint64_t out_alpha[4], uint64_t out_neg_z_alpha[4]) {
  if (!p || !commit_p || (n_public && !public_inputs) || !out_alpha || !out_neg_z_alpha || n_public > TRANSCRIPT_DEV_MAX_PUB) return DVP_EINVAL;
  DevBuf in, out;
  DVP_TRY(in.alloc(64 + (size_t)(n_public ? n_public : 1) * sizeof(Fr)));
  DVP_TRY(out.alloc(4 * sizeof(Fr)));
  uint8_t head[64];
  memset(head, 0xa5, sizeof(head));  // the bytes behind the 30 must not matter
  memcpy(head, commit_p, 30);
  DVP_HIP(hipMemcpy(in.p, head, 64, hipMemcpyHostToDevice));
  if (n_public) DVP_HIP(hipMemcpy((char*)in.p + 64, public_inputs, (size_t)n_public * sizeof(Fr), hipMemcpyHostToDevice));
  Fr* o = out.as<Fr>();
  DVP_LAUNCH(k_transcript, dim3(1), dim3(64), 0, 0, (const uint32_t*)in.p, (const Fr*)((char*)in.p + 64), n_public, p->h_ct, o, o + 1);
  DVP_LAUNCH(k_zalpha, dim3(1), dim3(64), 0, 0, o + 1, p->tree->d_x0, p->tree->d_t, (int)p->log_m, p->tree->layer((int)p->log_m), o + 2);
  DVP_LAUNCH(k_from_mont_vec, dim3(1), dim3(PT), 0, 0, o + 2, o + 3, (size_t)1);
  DVP_HIP(hipGetLastError());
  DVP_HIP(hipDeviceSynchronize());
  DVP_HIP(hipMemcpy(out_alpha, o, sizeof(Fr), hipMemcpyDeviceToHost));
  DVP_HIP(hipMemcpy(out_neg_z_alpha, o + 3, sizeof(Fr), hipMemcpyDeviceToHost));
  return DVP_OK;
}

// test access to the refusal of alpha in D u D' (include/dvpari_internal.h): challenge_alpha_host and challenge_dev read the pair
extern "C" int dvp_prover_debug_force_alpha(dvp_prover* p, const uint64_t alpha[4]) {
  if (!p) return DVP_EINVAL;
  if (!alpha) {
    p->alpha_forced = false;
    return DVP_OK;
  }
  Fr a;
  if (!fr_load((const uint8_t*)alpha, &a)) return DVP_EINVAL;  // >= p
  p->alpha_forced_pair[0] = a;
  p->alpha_forced_pair[1] = fr_to_mont(a);
  p->alpha_forced = true;
  return DVP_OK;
}

extern "C" int dvp_blake3(const uint8_t* data, size_t len, uint8_t out[32]) {
  if ((len && !data) || !out) return DVP_EINVAL;
  b3::hash(data, len, out);
  return DVP_OK;
}
