// The prover's lifetime and inputs: init / create / destroy, set_coeffs, set_matrix, the SRS setters.
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
#pragma once
#include "prove_slots.cuh"

static int prover_init(dvp_prover* p, uint32_t log2_m, uint32_t n_public, uint32_t n_wires) {
  p->log_m = log2_m;
  p->m = 1u << log2_m;
  p->n_pub = n_public;
  p->n_wires = n_wires;
  const size_t m = p->m;
  DVP_HIP(hipGetDevice(&p->home_device));  // every buffer of this prover lives on the device that is current now
  DVP_TRY(dvp_ecfft_create(log2_m + 1, 0, log2_m + 1, &p->tree));  // TREE_2N, src/proving.rs:274
  DVP_TRY(ecfft_device_consts(p->tree));
  auto A = [&](void** q, size_t bytes) -> int { DVP_HIP(hipMalloc(q, bytes ? bytes : 16)); return DVP_OK; };
  DVP_TRY(A((void**)&p->dD, m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->dD2, m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->barw, m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->z2inv, m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->bases_a, (n_wires + m) * sizeof(Aff)));
  DVP_TRY(A((void**)&p->inf_a, n_wires + m));
  DVP_TRY(A((void**)&p->bases_k, 4 * m * sizeof(Aff)));
  DVP_TRY(A((void**)&p->inf_k, 4 * m));
  DVP_TRY(A((void**)&p->w, n_wires * sizeof(Fr)));
  DVP_TRY(A((void**)&p->E, 4 * m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->E2, 4 * m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->r2, m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->SA, (n_wires + m) * sizeof(Fr)));
  DVP_TRY(A((void**)&p->den, 2 * m * sizeof(Fr)));  // [den | den2]: one batch inversion covers both
  p->den2 = p->den + m;
  DVP_TRY(A((void**)&p->SK, 4 * m * sizeof(Fr)));
  DVP_TRY(A((void**)&p->partial, 3 * 1024 * sizeof(Fr)));
  // what the host reads back at the end of a proof, in ONE block and one copy: a0 b0 i0 r0 | flags | encoded points
  DVP_TRY(A((void**)&p->blk, sizeof(ProverBlock)));
  DVP_HIP(hipMemset(p->blk, 0, sizeof(ProverBlock)));
  DVP_HIP(hipHostMalloc((void**)&p->fin_host, sizeof(ProverBlock) + 16, hipHostMallocDefault));  // + the merged range word of a mixed MSM
  DVP_TRY(A((void**)&p->mix, MIX_BYTES));
  p->table_budget = tune().table_budget_bytes < 0 ? UINT64_MAX : (uint64_t)tune().table_budget_bytes;
  DVP_HIP(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
  DVP_HIP(hipEventCreateWithFlags(&p->ev_alpha, hipEventDisableTiming));
  DVP_HIP(hipEventCreateWithFlags(&p->ev_negz, hipEventDisableTiming));
  {
    uint8_t h[32];
    b3::compile_hash(nullptr, nullptr, h);
    memcpy(p->h_ct.w, h, 32);
  }
  DVP_TRY(A((void**)&p->pts, 2 * sizeof(Aff)));
  DVP_TRY(A((void**)&p->pts_inf32, 8));
  DVP_TRY(A((void**)&p->pts_inf8, 8));
  DVP_HIP(hipMemset(p->inf_a, 0, n_wires + m));
  DVP_HIP(hipMemset(p->inf_k, 0, 4 * m));
  dvp_ecfft* t = p->tree;
  int kk = (int)log2_m;
  DVP_LAUNCH(k_split_domains, dim3(cdiv(m, PT)), dim3(PT), 0, 0, t->layer(0), (uint32_t)m, p->dD, p->dD2);
  // bar weights of D and 1/Z_D on D'
  DVP_LAUNCH(k_domain_tables, dim3(cdiv(m, PT)), dim3(PT), 0, 0, t->layer(0), (uint32_t)m, t->d_x0, t->d_t, kk,
                     t->layer(kk), 0, p->barw, p->z2inv);
  DVP_HIP(hipGetLastError());
  DVP_HIP(hipMemcpy(p->ctop_host, t->layer(kk), 2 * sizeof(Fr), hipMemcpyDeviceToHost));
  DVP_HIP(hipDeviceSynchronize());
  return DVP_OK;
}

extern "C" int dvp_prover_create(uint32_t log2_m, uint32_t n_public, uint32_t n_wires, dvp_prover** out) {
  // 2^24 constraints is the largest size the MSM index ranges cover (4m bases x 14 pre-rotated windows must stay below
  // 2^32, msm.hip) -- the reference's own tree constants stop at 2^27 leaves (src/ec_fft.rs:205), its SP1 circuit is 2^23
  if (!out || log2_m < 1 || log2_m > DVP_MAX_LOG2_CONSTRAINTS || n_wires < 1 + n_public || (uint64_t)n_wires > (1ull << 25)) return DVP_EINVAL;
  dvp_prover* p = new dvp_prover();
  int rc = prover_init(p, log2_m, n_public, n_wires);
  if (rc != DVP_OK) {
    dvp_prover_destroy(p);  // releases whatever was allocated before the failure
    return rc;
  }
  *out = p;
  return DVP_OK;
}

extern "C" void dvp_prover_destroy(dvp_prover* p) {
  if (!p) return;
  void* ptrs[] = {p->dD, p->dD2, p->barw, p->z2inv, p->coeffs_m, p->bases_a, p->inf_a, p->bases_k, p->inf_k, p->w, p->E,
                  p->E2, p->r2, p->SA, p->den, p->SK, p->partial, p->blk, p->pts, p->pts_inf32,
                  p->pts_inf8, p->mix};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (p->fin_host) (void)hipHostFree(p->fin_host);
  if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
  if (p->side) (void)hipStreamDestroy(p->side);
  if (p->ev_alpha) (void)hipEventDestroy(p->ev_alpha);
  if (p->ev_negz) (void)hipEventDestroy(p->ev_negz);
  for (auto& mt : p->mat) {
    if (mt.row_ptr) (void)hipFree(mt.row_ptr);
    if (mt.wire) (void)hipFree(mt.wire);
    if (mt.coeff) (void)hipFree(mt.coeff);
  }
  msm_fixed_destroy(p->fx[0]);
  msm_fixed_destroy(p->fx[1]);
  const bool multi = slots_live(p) > 1;
  for (uint32_t k = 0; k < p->slots.size(); ++k)  // the parked slots; the active one's fields are released above
    if (k != p->active_slot) slot_free(&p->slots[k]);
  if (multi) multi_slot_provers_add(-1);
  shards_release(p);
  if (p->mg_parts) (void)hipFree(p->mg_parts);
  if (p->tree) dvp_ecfft_destroy(p->tree);
  delete p;
}

extern "C" int dvp_prover_set_coeffs(dvp_prover* p, const uint64_t* coeffs, uint32_t n) {
  if (!p || !coeffs || !n) return DVP_EINVAL;
  if (p->coeffs_m) (void)hipFree(p->coeffs_m);
  DVP_HIP(hipMalloc((void**)&p->coeffs_m, (size_t)n * sizeof(Fr)));
  DevBuf tmp;
  DVP_TRY(tmp.up(coeffs, (size_t)n * sizeof(Fr)));
  DVP_LAUNCH(k_to_mont_vec, dim3(cdiv(n, PT)), dim3(PT), 0, 0, tmp.as<Fr>(), p->coeffs_m, (size_t)n);
  DVP_HIP(hipDeviceSynchronize());
  p->n_coeffs = n;
  return DVP_OK;
}

// which: 0 = L (A), 1 = R (B), 2 = O (C) of src/gnark_r1cs.rs:112-119; CSR over n_rows <= m rows
extern "C" int dvp_prover_set_matrix(dvp_prover* p, int which, uint32_t n_rows, const uint32_t* row_ptr,
                                     const uint32_t* wire_ids, const uint32_t* coeff_ids) {
  if (!p || which < 0 || which > 2 || !row_ptr || n_rows > p->m) return DVP_EINVAL;
  // a well-formed CSR: row_ptr[0] == 0 and non-decreasing (k_r1cs_eval walks [row_ptr[i], row_ptr[i+1]) unchecked)
  if (row_ptr[0] != 0) { g_last_error_index = 0; return DVP_EINVAL; }
  for (uint32_t i = 0; i < n_rows; ++i)
    if (row_ptr[i + 1] < row_ptr[i]) { g_last_error_index = (int64_t)i; return DVP_EINVAL; }
  size_t nnz = row_ptr[n_rows];
  if (nnz && (!wire_ids || !coeff_ids)) return DVP_EINVAL;
  uint32_t max_cid = 0;
  for (size_t k = 0; k < nnz; ++k) {
    if (wire_ids[k] >= p->n_wires || (p->n_coeffs && coeff_ids[k] >= p->n_coeffs)) {
      g_last_error_index = (int64_t)k;
      return DVP_EINVAL;
    }
    if (coeff_ids[k] > max_cid) max_cid = coeff_ids[k];
  }
  DevCsr& mt = p->mat[which];
  if (mt.row_ptr) { (void)hipFree(mt.row_ptr); (void)hipFree(mt.wire); (void)hipFree(mt.coeff); }
  DVP_HIP(hipMalloc((void**)&mt.row_ptr, ((size_t)n_rows + 1) * 4));
  DVP_HIP(hipMalloc((void**)&mt.wire, (nnz ? nnz : 1) * 4));
  DVP_HIP(hipMalloc((void**)&mt.coeff, (nnz ? nnz : 1) * 4));
  DVP_HIP(hipMemcpy(mt.row_ptr, row_ptr, ((size_t)n_rows + 1) * 4, hipMemcpyHostToDevice));
  if (nnz) {
    DVP_HIP(hipMemcpy(mt.wire, wire_ids, nnz * 4, hipMemcpyHostToDevice));
    DVP_HIP(hipMemcpy(mt.coeff, coeff_ids, nnz * 4, hipMemcpyHostToDevice));
  }
  mt.n_rows = n_rows;
  mt.nnz = nnz;
  mt.max_coeff_id = max_cid;
  return DVP_OK;
}

// a base vector of MSM `slot` changed: its fixed-base tables (and every device shard) are stale
static void srs_changed(dvp_prover* p, int slot) {
  msm_fixed_destroy(p->fx[slot]);
  p->fx[slot] = nullptr;
  shards_release(p);
}
// how every setter opens: the slot of vector `which`, which must be n points long
static int srs_slot(dvp_prover* p, int which, size_t n, Aff** base, uint8_t** inf) {
  const size_t m = p->m, nw = p->n_wires;
  if (which < 0 || which > 4 || n != (which == 0 ? nw : which == 4 ? 2 * m : m)) return DVP_EINVAL;
  DVP_TRY(slot_alloc_bases(p));  // an added SRS slot gets its base vectors with its first setter
  size_t want;
  switch (which) {
    case 0: *base = p->bases_a; *inf = p->inf_a; want = nw; break;
    case 1: *base = p->bases_a + nw; *inf = p->inf_a + nw; want = m; break;
    case 2: *base = p->bases_k; *inf = p->inf_k; want = m; break;
    case 3: *base = p->bases_k + m; *inf = p->inf_k + m; want = m; break;
    case 4: *base = p->bases_k + 2 * m; *inf = p->inf_k + 2 * m; want = 2 * m; break;
    default: return DVP_EINVAL;
  }
  if (n != want) return DVP_EINVAL;
  p->trace_ok = false;  // the caller overwrites the slot: the last proof's commitments are not sums over these bases
  return DVP_OK;
}
// how every setter closes.  Its copies / fills ran on the default stream; proofs run on other (non-blocking) streams, which do not order
// themselves behind it: nothing of a setter may still be in flight when it returns
static int srs_set_done(dvp_prover* p, int which) {
  p->have_srs[which] = true;
  srs_changed(p, which < 2 ? 0 : 1);
  DVP_HIP(hipStreamSynchronize(nullptr));
  return DVP_OK;
}
// strict mode (dvp_points_set_strict; a no-op otherwise): the vector just copied into the prover must hold reduced points of E[r].  The
// slot has been overwritten by then, so a rejected vector leaves it UNSET and its tables stale -- a later proof fails as for a vector
// that was never given (prover_ready), not on the rejected or the previous bases.  Waits on the default stream, as the setters do anyway.
static int srs_strict_check(dvp_prover* p, int which, const Aff* base, const uint8_t* inf, size_t n) {
  int rc = points_check_strict(base, inf, n, nullptr);
  if (rc != DVP_OK) {
    p->have_srs[which] = false;
    srs_changed(p, which < 2 ? 0 : 1);
  }
  return rc;
}
// which: 0 g_m (n_wires), 1 g_q (m), 2 g_k_0 (m), 3 g_k_1 (m), 4 g_k_2 (2m) -- src/artifacts.rs names;
// enc = payload of the reference's point-vector file (n x 30 B, src/io_utils.rs:83-111), decoded ONCE
// into HBM-resident affine bases (the reference re-reads and re-decodes them on every prove()).
extern "C" int dvp_prover_set_srs_encoded(dvp_prover* p, int which, const uint8_t* enc, size_t n) {
  if (!p || !enc) return DVP_EINVAL;
  Aff* base; uint8_t* inf;
  DVP_TRY(srs_slot(p, which, n, &base, &inf));
  DevBuf de;
  DVP_TRY(de.up(enc, n * 30));
  DVP_TRY(decode_dev(de.as<uint8_t>(), n, base, inf, 0));
  return srs_set_done(p, which);
}
static int srs_set_affine(dvp_prover* p, int which, const void* xy, const void* inf_in, size_t n, hipMemcpyKind kind) {
  if (!p || !xy) return DVP_EINVAL;
  Aff* base; uint8_t* inf;
  DVP_TRY(srs_slot(p, which, n, &base, &inf));
  DVP_HIP(hipMemcpy(base, xy, n * sizeof(Aff), kind));
  if (inf_in) DVP_HIP(hipMemcpy(inf, inf_in, n, kind));
  else DVP_HIP(hipMemset(inf, 0, n));
  DVP_TRY(srs_strict_check(p, which, base, inf, n));
  return srs_set_done(p, which);
}
extern "C" int dvp_prover_set_srs_affine(dvp_prover* p, int which, const uint64_t* xy, const uint8_t* inf_in, size_t n) {
  return srs_set_affine(p, which, xy, inf_in, n, hipMemcpyHostToDevice);
}
// device-to-device flavour (bases produced on the GPU, e.g. by dvp_mulgen on the same device)
extern "C" int dvp_prover_set_srs_affine_dev(dvp_prover* p, int which, const void* d_xy, const void* d_inf, size_t n) {
  return srs_set_affine(p, which, d_xy, d_inf, n, hipMemcpyDeviceToDevice);
}
