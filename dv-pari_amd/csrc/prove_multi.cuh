// One witness, many verifiers: dvp_prove_multi* -- phase 1 once, then the rest of a proof once per SRS slot (prove_slots.cuh).
// Part of prove.hip's translation unit: included once, at global scope behind its `using namespace dvp` (map: top of prove.hip).
//
// What is shared and what is not.  The challenge phase reads E, r2, D, D' and writes den and SK; the commitment MSM reads SA = [w | q2]
// and leaves it as it is.  So everything prove_begin_impl produces -- the R1CS rows, the unsatisfied-row flag, the extends, the quotient --
// is computed once per call, and a slot costs what follows the begin in dvp_prove_dev: the commitment MSM over that slot's bases, the
// transcript under that slot's binding, the challenge phase, the K MSM, the 118 bytes.  The slots run one after the other on the
// caller's stream, in the order given, each by the very code of a single proof (prove_dev_device_rest / prove_dev_host_rest).
//
// Error order.  Arguments first (no device work): a NULL pointer, n_slots == 0, a slot index that was never handed out or has been
// dropped (DVP_EINVAL, dvp_last_error_index = its position in `slots`).  Then the witness: an unsatisfied row (DVP_EUNSAT, the row) or
// a scalar >= p (DVP_EINVAL, its index) shows at the first slot's wait, as in a single proof; the call returns it, proves no further
// slot and has written nothing to `proofs`.  Everything else is a slot's own outcome and goes to status[j] without stopping the
// others: a slot that lacks one of its five vectors (DVP_EINVAL, what a single proof on it answers), DVP_ECHALLENGE, an MSM's status.
// status[j] is written for every slot the call reached; proofs + 118 j only where status[j] == DVP_OK.
#pragma once
#include "prove_challenge.cuh"

// arguments, then the slot that goes first: the first listed slot that has all five vectors is made active (the begin and the
// witness staging ask prover_ready of the ACTIVE slot).  *restore = the slot to make active again; *none = no listed slot is
// complete -- every status is DVP_EINVAL and there is nothing to run.
static int multi_open(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint8_t* proofs, int32_t* status, uint32_t* restore, bool* none) {
  if (!p || !slots || !n_slots || !proofs || !status) return DVP_EINVAL;
  for (uint32_t j = 0; j < n_slots; ++j)
    if (!slot_known(p, slots[j])) {
      g_last_error_index = (int64_t)j;
      return DVP_EINVAL;
    }
  *restore = p->active_slot;
  *none = true;
  for (uint32_t j = 0; j < n_slots && *none; ++j)
    if (slot_complete(p, slots[j])) {
      slot_activate(p, slots[j]);
      *none = false;
    }
  if (*none)
    for (uint32_t j = 0; j < n_slots; ++j) status[j] = DVP_EINVAL;
  return DVP_OK;
}
// the slot that was active at the call is active again; the last proof's trace stays valid only if it is that slot's (keep_trace)
static void multi_close(dvp_prover* p, uint32_t restore, bool keep_trace) {
  const bool tr = p->trace_ok;
  slot_activate(p, restore);
  p->trace_ok = tr && keep_trace && p->active_slot == restore;
}
static int multi_run(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const void* d_assignment, uint8_t* proofs, int32_t* status,
                     void* stream, uint32_t restore) {
  hipStream_t st = (hipStream_t)stream;
  const bool dev = prove_flavour_device(p);  // chosen as dvp_prove_dev chooses it, once for the call
  int rc_call = DVP_OK;
  bool begun = false, last_ok = false;
  for (uint32_t j = 0; j < n_slots; ++j) {
    last_ok = false;
    if (!slot_complete(p, slots[j])) {
      status[j] = DVP_EINVAL;
      continue;
    }
    slot_activate(p, slots[j]);
    ProfScope ps(PROF_PROVE_TOTAL, st);
    if (!begun) {
      if (dev && !p->shards.empty()) shards_release(p);
      rc_call = prove_begin_impl(p, d_assignment, 1, stream, true, /*pub_to_host=*/!dev);
      if (rc_call != DVP_OK) break;
      begun = true;
    } else {
      // what a begin resets of the state a slot writes: the previous slot's proof is no longer what the buffers hold, its MSMs' fused
      // encodings are stale, and the alpha-in-domain flag is this slot's to raise (the unsatisfied-row flag stays: it is the witness's)
      p->trace_ok = p->challenge_sliced = false;
      p->enc_fused[0] = p->enc_fused[1] = false;
      const hipError_t e = hipMemsetAsync(p->blk->flags + 1, 0xff, 8, st);
      if (e != hipSuccess) {
        g_last_hip_error = e;
        rc_call = DVP_EHIP;
        break;
      }
    }
    bool witness_fault = false;
    uint8_t out[118];
    const int rc = dev ? prove_dev_device_rest(p, ps, out, stream, &witness_fault) : prove_dev_host_rest(p, ps, out, stream, &witness_fault);
    if (rc != DVP_OK && witness_fault) {
      rc_call = rc;
      break;
    }
    status[j] = rc;
    if (rc == DVP_OK) {
      memcpy(proofs + 118 * (size_t)j, out, 118);
      last_ok = true;
    }
  }
  multi_close(p, restore, rc_call == DVP_OK && last_ok && slots[n_slots - 1] == restore);
  return rc_call;
}

// Proof::prove for the SRS of every listed verifier (SRS per Trapdoor, src/srs.rs:31-50,177; Proof::prove, src/proving.rs:426-688) with
// the assignment already in HBM.  No stream wait beyond one per slot in the device-transcript flavour (the K MSM's own).
extern "C" int dvp_prove_multi_dev(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const void* d_assignment, uint8_t* proofs,
                                   int32_t* status, void* stream) {
  if (!d_assignment) return DVP_EINVAL;
  uint32_t restore = 0;
  bool none = false;
  DVP_TRY(multi_open(p, slots, n_slots, proofs, status, &restore, &none));
  if (none) return DVP_OK;
  return multi_run(p, slots, n_slots, d_assignment, proofs, status, stream, restore);
}
// the three host forms: the staging of dvp_prove / dvp_prove_be32 / dvp_prove_ark once, then dvp_prove_multi_dev's loop on the
// prover's own stream
extern "C" int dvp_prove_multi(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint64_t* public_inputs, uint32_t n_public,
                               const uint64_t* private_inputs, uint32_t n_private, uint8_t* proofs, int32_t* status) {
  uint32_t restore = 0;
  bool none = false;
  DVP_TRY(multi_open(p, slots, n_slots, proofs, status, &restore, &none));
  if (none) return DVP_OK;
  const int rc = stage_witness(p, public_inputs, n_public, private_inputs, n_private, proofs);
  if (rc != DVP_OK) {
    multi_close(p, restore, true);
    return rc;
  }
  return multi_run(p, slots, n_slots, p->w, proofs, status, p->own_stream, restore);
}
extern "C" int dvp_prove_multi_be32(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint8_t* witness_be32, size_t n,
                                    uint8_t* proofs, int32_t* status) {
  if (!p || !witness_be32 || n < p->n_wires) return DVP_EINVAL;
  if (!fr_be32_is_one(witness_be32)) {
    g_last_error_index = 0;
    return DVP_EINVAL;
  }
  uint32_t restore = 0;
  bool none = false;
  DVP_TRY(multi_open(p, slots, n_slots, proofs, status, &restore, &none));
  if (none) return DVP_OK;
  auto stage = [&]() -> int {
    DVP_TRY(witness_stream(p));
    DVP_HIP(hipMemcpyAsync(p->w, witness_be32, (size_t)p->n_wires * 32, hipMemcpyHostToDevice, p->own_stream));
    DVP_HIP(hipStreamSynchronize(p->own_stream));  // the caller's buffer is free again on return
    return dvp_fr_from_be32_dev(p->w, p->n_wires, p->w, p->own_stream);
  };
  const int rc = stage();
  if (rc != DVP_OK) {
    multi_close(p, restore, true);
    return rc;
  }
  return multi_run(p, slots, n_slots, p->w, proofs, status, p->own_stream, restore);
}
extern "C" int dvp_prove_multi_ark(dvp_prover* p, const uint32_t* slots, uint32_t n_slots, const uint64_t* public_ark, uint32_t n_public,
                                   const uint64_t* private_ark, uint32_t n_private, uint8_t* proofs, int32_t* status) {
  uint32_t restore = 0;
  bool none = false;
  DVP_TRY(multi_open(p, slots, n_slots, proofs, status, &restore, &none));
  if (none) return DVP_OK;
  int rc = stage_witness(p, public_ark, n_public, private_ark, n_private, proofs);
  if (rc == DVP_OK) rc = dvp_fr_from_ark_dev(p->w + 1, (size_t)p->n_wires - 1, p->w + 1, p->own_stream);
  if (rc != DVP_OK) {
    multi_close(p, restore, true);
    return rc;
  }
  return multi_run(p, slots, n_slots, p->w, proofs, status, p->own_stream, restore);
}
