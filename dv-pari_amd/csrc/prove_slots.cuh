// SRS slots: one prover, one circuit, one set of work buffers -- and one SRS per verifier (SRS per Trapdoor, src/srs.rs:31-50,177).
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
//
// State model.  The prover's own fields (bases_a, inf_a, bases_k, inf_k, have_srs, fx, fx_lo, fx_hi, table_budget, table_refused, h_ct)
// are the ACTIVE slot: the setters, the MSMs, the budget code, the hashes, the trace and the witness check read them as they always
// have.  dvp_prover::slots has one entry per index handed out; the entry of the active index is a placeholder.  Selecting a slot
// writes the fields into the placeholder and loads the chosen entry: a host-side swap of pointers and flags, no device work.
// A slot's bases are allocated by its first setter (slot 0's by dvp_prover_create, as before), its tables by its first proof.
#pragma once
#include "prove_state.cuh"

static void shards_release(dvp_prover* p);  // prove_msm.cuh, with the shards it releases

static void slot_store(const dvp_prover* p, SrsSlot* s) {
  s->bases_a = p->bases_a; s->inf_a = p->inf_a; s->bases_k = p->bases_k; s->inf_k = p->inf_k;
  s->table_budget = p->table_budget;
  s->h_ct = p->h_ct;
  for (int k = 0; k < 5; ++k) s->have_srs[k] = p->have_srs[k];
  for (int w = 0; w < 2; ++w) {
    s->fx[w] = p->fx[w]; s->fx_lo[w] = p->fx_lo[w]; s->fx_hi[w] = p->fx_hi[w]; s->table_refused[w] = p->table_refused[w];
  }
}
static void slot_load(dvp_prover* p, const SrsSlot& s) {
  p->bases_a = s.bases_a; p->inf_a = s.inf_a; p->bases_k = s.bases_k; p->inf_k = s.inf_k;
  p->table_budget = s.table_budget;
  p->h_ct = s.h_ct;
  for (int k = 0; k < 5; ++k) p->have_srs[k] = s.have_srs[k];
  for (int w = 0; w < 2; ++w) {
    p->fx[w] = s.fx[w]; p->fx_lo[w] = s.fx_lo[w]; p->fx_hi[w] = s.fx_hi[w]; p->table_refused[w] = s.table_refused[w];
  }
}
// a fresh slot: no bases, no tables, no limit on them, the reference's binding (hashes of empty buffers, src/proving.rs:86-105,113-132)
static SrsSlot slot_empty(bool live) {
  SrsSlot s;
  uint8_t h[32];
  b3::compile_hash(nullptr, nullptr, h);
  memcpy(s.h_ct.w, h, 32);
  s.live = live;
  return s;
}
// what a parked slot holds on the device; nothing may still read it
static void slot_free(SrsSlot* s) {
  void* ptrs[] = {s->bases_a, s->inf_a, s->bases_k, s->inf_k};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  msm_fixed_destroy(s->fx[0]);
  msm_fixed_destroy(s->fx[1]);
  *s = slot_empty(false);
}
// the active slot's base vectors, allocated by its first setter (flags cleared, as dvp_prover_create leaves slot 0's)
static int slot_alloc_bases(dvp_prover* p) {
  if (p->bases_a) return DVP_OK;
  const size_t na = (size_t)p->n_wires + p->m, nk = 4 * (size_t)p->m;
  Aff *ba = nullptr, *bk = nullptr;
  uint8_t *ia = nullptr, *ik = nullptr;
  const bool ok = hipMalloc((void**)&ba, na * sizeof(Aff)) == hipSuccess && hipMalloc((void**)&ia, na) == hipSuccess &&
                  hipMalloc((void**)&bk, nk * sizeof(Aff)) == hipSuccess && hipMalloc((void**)&ik, nk) == hipSuccess &&
                  hipMemset(ia, 0, na) == hipSuccess && hipMemset(ik, 0, nk) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    void* ptrs[] = {ba, ia, bk, ik};
    for (void* q : ptrs)
      if (q) (void)hipFree(q);
    return DVP_ENOMEM;
  }
  p->bases_a = ba; p->inf_a = ia; p->bases_k = bk; p->inf_k = ik;
  return DVP_OK;
}
static uint32_t slots_live(const dvp_prover* p) {
  uint32_t n = 0;
  for (const SrsSlot& s : p->slots) n += s.live ? 1 : 0;
  return n;
}
static bool slot_known(const dvp_prover* p, uint32_t slot) { return slot < p->slots.size() && p->slots[slot].live; }
// all five vectors of slot `slot` are set (the SRS half of prover_ready)
static bool slot_complete(const dvp_prover* p, uint32_t slot) {
  const bool* have = slot == p->active_slot ? p->have_srs : p->slots[slot].have_srs;
  for (int k = 0; k < 5; ++k)
    if (!have[k]) return false;
  return true;
}
// the swap itself; the caller has checked the index.  As after an SRS setter, the last proof's trace does not describe the new bases
static void slot_activate(dvp_prover* p, uint32_t slot) {
  if (slot == p->active_slot) return;
  slot_store(p, &p->slots[p->active_slot]);
  slot_load(p, p->slots[slot]);
  p->active_slot = slot;
  p->trace_ok = false;
}

// A device list (dvp_set_devices, more than one entry) shards ONE slot's bases over the devices: a prover with a second slot and a
// list in force exclude each other, from both sides (capi.cpp counts the provers that hold more than one slot).
extern "C" int dvp_prover_srs_slot_add(dvp_prover* p, uint32_t* slot) {
  if (!p || !slot || mgpu_devices().size() > 1) return DVP_EINVAL;
  shards_release(p);  // slices of the active slot's bases left behind by an earlier device list
  const bool first_extra = slots_live(p) == 1;
  uint32_t k = 0;
  while (k < p->slots.size() && p->slots[k].live) ++k;
  if (k == p->slots.size()) p->slots.push_back(slot_empty(true));
  else p->slots[k] = slot_empty(true);
  if (first_extra) multi_slot_provers_add(1);
  *slot = k;
  return DVP_OK;
}
extern "C" int dvp_prover_srs_slot_select(dvp_prover* p, uint32_t slot) {
  if (!p || !slot_known(p, slot)) return DVP_EINVAL;
  slot_activate(p, slot);
  return DVP_OK;
}
extern "C" uint32_t dvp_prover_srs_slot_active(const dvp_prover* p) { return p ? p->active_slot : 0; }
extern "C" uint32_t dvp_prover_srs_slot_count(const dvp_prover* p) { return p ? (uint32_t)p->slots.size() : 0; }
// Waits for the whole device: the prover cannot know which caller stream a proof over these bases was enqueued on.
extern "C" int dvp_prover_srs_slot_drop(dvp_prover* p, uint32_t slot) {
  if (!p || !slot_known(p, slot) || slot == p->active_slot) return DVP_EINVAL;
  DVP_HIP(hipDeviceSynchronize());
  slot_free(&p->slots[slot]);
  if (slots_live(p) == 1) multi_slot_provers_add(-1);
  return DVP_OK;
}
extern "C" int dvp_prover_srs_slot_bytes(const dvp_prover* p, uint32_t slot, uint64_t* bases, uint64_t* tables) {
  if (!p || !bases || !tables || slot >= p->slots.size()) return DVP_EINVAL;
  *bases = *tables = 0;
  if (!p->slots[slot].live) return DVP_OK;  // dropped: nothing held
  SrsSlot s = p->slots[slot];
  if (slot == p->active_slot) slot_store(p, &s);
  if (s.bases_a) *bases = ((uint64_t)p->n_wires + 5 * (uint64_t)p->m) * (sizeof(Aff) + 1);
  *tables = msm_fixed_table_bytes(s.fx[0], nullptr) + msm_fixed_table_bytes(s.fx[1], nullptr);
  return DVP_OK;
}
