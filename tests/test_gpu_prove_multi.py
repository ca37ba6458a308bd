"""GPU tests (-m gpu) of the SRS slots and dvp_prove_multi*: one prover, one witness, one proof per verifier.

The reference for bytes is always the single-SRS path -- a fresh Prover given one SRS -- which tests/test_gpu_prove.py pins against the
oracle at this very size (synthetic_dense(8), and the toy circuit with its two public inputs).  Three trapdoors give three SRSs."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as o
import msm_cases as mc
from witness_cases import be32

pytestmark = pytest.mark.gpu
EINVAL, EUNSAT = -1, -3


class Case:
    """a circuit with its witness, three trapdoors, their SRSs, and the 118 bytes a fresh single-SRS prover gives for each"""

    def __init__(self, dvp, inst, pub, prv, seed):
        self.inst, self.pub, self.prv = inst, list(pub), list(prv)
        rnd = random.Random(seed)
        self.tds = [dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P)) for _ in range(3)]
        scratch = dvp.proving.Prover(inst)
        self.srss = [dvp.srs.verifier_runs_setup(scratch, inst, td) for td in self.tds]
        scratch.close()
        self.ref = []
        for srs in self.srss:
            q = self.single(dvp, srs)
            self.ref.append(q.prove(self.pub, self.prv))
            q.close()
        assert len({p.to_bytes() for p in self.ref}) == 3

    def single(self, dvp, srs):
        q = dvp.proving.Prover(self.inst)
        q.set_srs(srs)
        return q

    def multi(self, dvp):
        """a prover with the three SRSs in slots 0, 1, 2 (slot 0 through the plain setters, as before slots existed)"""
        mp = dvp.proving.Prover(self.inst)
        mp.set_srs(self.srss[0])
        assert [mp.add_srs(self.srss[1]), mp.add_srs(self.srss[2])] == [1, 2]
        assert mp.active_srs() == 0 and mp.srs_slots() == [0, 1, 2]
        return mp

    def payload(self, dvp, j):
        """the stream dvp_prover_srs_hash hashes for SRS j: to_bytes() of g_k[0], g_k[1], g_k[2], g_q, g_m"""
        enc = [dvp.curve.to_bytes(xy, inf).tobytes() for xy, inf in self.srss[j].as_list()]
        return enc[2] + enc[3] + enc[4] + enc[1] + enc[0]


@pytest.fixture(scope="module")
def dense8(dvp):
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(8)
    return Case(dvp, inst, pub, prv, 88)


@pytest.fixture(scope="module")
def toy(dvp):
    g = dvp.gnark_r1cs
    return Case(dvp, g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 2), o.TOY_PUBLIC, o.TOY_PRIVATE, 5)


def _prof(dvp, name):
    ms, n = C.c_double(0), C.c_uint64(0)
    dvp.check(dvp.lib.dvp_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return int(n.value)


def _budget_for(dvp, s0, s1, want0, want1):
    """the smallest budget whose plan covers (want0, want1) bases (the planner is monotone in the budget)"""
    lo, hi = 0, sum(dvp.table_plan(s0, s1, None)[1])
    while lo < hi:
        mid = (lo + hi) // 2
        c = dvp.table_plan(s0, s1, mid)[0]
        if c[1] >= want1 and c[0] >= want0:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _all_forms(dvp, c, mp, slots=None):
    """prove_multi, prove_multi_be32 and prove_multi_dev over `slots`: three result lists"""
    import torch

    w = [1] + c.pub + c.prv
    assignment = torch.from_numpy(dvp.fr.vec(w).view(np.int64)).to(torch.device("cuda", 0))
    return [mp.prove_multi(c.pub, c.prv, slots), mp.prove_multi_be32(be32(w), slots), mp.prove_multi_dev(assignment.data_ptr(), slots)]


@pytest.mark.parametrize("config", ["all-tables", "slot1-one-shot", "slot2-mixed"])
def test_same_bytes_as_n_provers(dvp, dense8, config):
    """item 1: every slot's 118 bytes are those of a fresh single-SRS prover, whatever route that slot's MSMs take"""
    c = dense8
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        mp = c.multi(dvp)
        s0, s1 = mp.msm_size(0), mp.msm_size(1)
        if config == "slot1-one-shot":
            mp.select_srs(1)
            mp.set_table_budget(0)
            mp.select_srs(0)
        if config == "slot2-mixed":
            mp.select_srs(2)
            mp.set_table_budget(_budget_for(dvp, s0, s1, 0, s1 * 3 // 8))
            mp.select_srs(0)
        for got in _all_forms(dvp, c, mp):
            assert got == c.ref
        # which route each slot took: what its coverage says, and what it holds
        for j in range(3):
            mp.select_srs(j)
            cov = [mp.msm_coverage(w)[0] for w in (0, 1)]
            held = mp.srs_slot_bytes(j)[1]
            if config == "slot1-one-shot" and j == 1:
                assert cov == [0, 0] and held == 0
            elif config == "slot2-mixed" and j == 2:
                assert cov[0] == 0 and 0 < cov[1] < s1 and held > 0
            else:
                assert cov == [s0, s1] and held > 0
        mp.select_srs(0)
        # order and repetition are the caller's
        got = mp.prove_multi(c.pub, c.prv, [2, 0, 2])
        assert got == [c.ref[2], c.ref[0], c.ref[2]]
        mp.close()


@pytest.mark.parametrize("host_transcript", [0, 1])
def test_toy_with_public_inputs_both_flavours(dvp, toy, host_transcript):
    """item 1 on the toy circuit (two public inputs) under the device and the host transcript"""
    c = toy
    with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=host_transcript):
        q = c.single(dvp, c.srss[1])
        assert q.prove(c.pub, c.prv) == c.ref[1]  # the flavours agree on the single path
        q.close()
        mp = c.multi(dvp)
        for got in _all_forms(dvp, c, mp):
            assert got == c.ref
        assert mp.prove_multi(c.pub, c.prv, [1]) == [c.ref[1]]
        mp.close()


def test_each_proof_belongs_to_its_verifier(dvp, dense8):
    """item 2: proof j is accepted under trapdoor j and fails the equation under the other two"""
    c = dense8
    mp = c.multi(dvp)
    proofs = mp.prove_multi(c.pub, c.prv)
    mp.close()
    for i, td in enumerate(c.tds):
        verdicts = dvp.srs.verify_batch(td, [c.pub] * 3, proofs).tolist()
        assert verdicts == [0 if j == i else dvp.srs.VERIFY_EQUATION for j in range(3)], (i, verdicts)


def test_phase_one_runs_once(dvp, dense8):
    """item 3: against ONE single proof, a prove_multi over three slots launches the R1CS row kernel, the quotient and every extend
    kernel as often, the challenge kernels, the transcript and the MSM tails three times as often, and waits at most three times.

    The waits: an MSM too small for a first pair round waits for its largest-bucket read ON the proof's stream, mid-way (msm.hip:
    PairRounds::begin counts it as a stream wait), so at 2^8 rows with default knobs a SINGLE proof already waits three times (measured:
    3 for one proof, 9 for three slots).  As tests/test_gpu_table_budget.py does for its 2^13 case, the knobs below give the two
    MSMs of 512 and 1024 terms the shape they have at the sizes the path is meant for -- tables with 2^8-bucket windows, pair rounds
    down to 32 additions, so the first round is enqueued ahead of that read and the read waits on the side stream -- and then a
    proof has its one stream wait and three slots have three."""
    with dvp.tune(DVP_MSM_FIXED_MIN=1, DVP_MSM_FIXED_C=8, DVP_MSM_AFF_MIN=32):
        _phase_one_runs_once(dvp, dense8)


def _phase_one_runs_once(dvp, dense8):
    c = dense8
    mp = c.multi(dvp)
    assert mp.prove_multi(c.pub, c.prv) == c.ref  # every slot's tables and the workspaces exist from here on
    assert mp.prove(c.pub, c.prv) == c.ref[0]
    prefixes = ("prove.hip:", "ecfft.hip:", "msm.hip:k_tail", "fr_ops.hip:k_batch_inverse")
    dvp.lib.dvp_profile_reset()
    assert mp.prove(c.pub, c.prv) == c.ref[0]
    one, waits_one = mc.census(dvp, prefixes), _prof(dvp, "host_waits_stream")
    dvp.lib.dvp_profile_reset()
    assert mp.prove_multi(c.pub, c.prv) == c.ref
    three, waits_three = mc.census(dvp, prefixes), _prof(dvp, "host_waits_stream")
    mp.close()
    once = {k for k in one if k.startswith("ecfft.hip:") or k.startswith(("prove.hip:k_r1cs_eval", "prove.hip:k_quotient"))}
    per_slot = {k for k in one if k.startswith(("msm.hip:k_tail", "fr_ops.hip:k_batch_inverse", "prove.hip:k_alpha_denoms", "prove.hip:k_bary3",
                                                "prove.hip:k_kscalars", "prove.hip:k_transcript", "prove.hip:k_zalpha"))}
    assert one["prove.hip:k_r1cs_eval"] == 1 and sum(one[k] for k in once if k.startswith("ecfft.hip:")) > 0
    assert sum(one[k] for k in once if k.startswith("prove.hip:k_quotient")) == 1
    for k in ("prove.hip:k_alpha_denoms", "prove.hip:k_bary3_final", "prove.hip:k_kscalars", "prove.hip:k_transcript", "prove.hip:k_zalpha"):
        assert one[k] == 1, k
    assert sum(one[k] for k in per_slot if k.startswith("msm.hip:k_tail")) >= 2  # two MSMs per proof
    for k in once:
        assert three[k] == one[k], (k, one[k], three[k])
    for k in per_slot:
        assert three[k] == 3 * one[k], (k, one[k], three[k])
    print("host_waits_stream: one proof", waits_one, "three slots", waits_three)
    assert waits_one == 1 and waits_three <= 3, (waits_one, waits_three)


def test_nothing_existing_moves(dvp, dense8):
    """item 4: slot 0 proves the same bytes whatever happens to other slots; a selected slot is what every entry acts on; the trace rule"""
    c = dense8
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        mp = dvp.proving.Prover(c.inst)
        mp.set_srs(c.srss[0])
        assert (mp.active_srs(), mp.srs_slots()) == (0, [0])
        assert mp.prove(c.pub, c.prv) == c.ref[0]
        hash0, cov0 = mp.srs_hash(), [mp.msm_coverage(w) for w in (0, 1)]
        assert hash0 == o.blake3(c.payload(dvp, 0))
        k1, k2 = mp.add_srs(c.srss[1]), mp.add_srs()
        assert (k1, k2) == (1, 2) and mp.active_srs() == 0
        assert mp.prove(c.pub, c.prv) == c.ref[0]
        mp.select_srs(2)
        mp.select_srs(0)
        mp.drop_srs(2)
        assert mp.srs_slots() == [0, 1] and mp.prove(c.pub, c.prv) == c.ref[0]
        assert mp.add_srs(c.srss[2]) == 2  # the dropped index is reused
        assert mp.prove_multi(c.pub, c.prv) == c.ref
        assert mp.active_srs() == 0 and mp.prove(c.pub, c.prv) == c.ref[0]
        # a selected slot is the one every entry acts on
        s0, s1 = mp.msm_size(0), mp.msm_size(1)
        mp.select_srs(1)
        assert mp.active_srs() == 1
        assert mp.prove(c.pub, c.prv) == c.ref[1]
        assert mp.srs_hash() == o.blake3(c.payload(dvp, 1)) != hash0
        assert mp.msm_plan(1) != (0, 0) and mp.msm_coverage(1)[0] == s1
        mp.set_table_budget(0)
        assert [mp.msm_coverage(w)[0] for w in (0, 1)] == [0, 0] and mp.msm_plan(1) == (0, 0)
        assert mp.prove(c.pub, c.prv) == c.ref[1] and mp.srs_slot_bytes(1)[1] == 0
        mp.select_srs(0)
        assert [mp.msm_coverage(w) for w in (0, 1)] == cov0 and mp.srs_hash() == hash0
        assert mp.msm_plan(1) != (0, 0) and mp.srs_slot_bytes(0)[1] > 0
        assert mp.prove(c.pub, c.prv) == c.ref[0]
        # the trace: valid when the last slot proven is the active one, refused otherwise
        rec = mp.trace_last(dvp.proving.TRACE_POINTS)
        assert rec["commit_p"]["enc"] == c.ref[0].commit_p
        mp.select_srs(0)  # already active: nothing changes
        assert mp.trace_last(dvp.proving.TRACE_POINTS) == rec
        assert mp.prove_multi(c.pub, c.prv, [1, 2, 0]) == [c.ref[1], c.ref[2], c.ref[0]]
        assert mp.trace_last(dvp.proving.TRACE_POINTS) == rec
        assert mp.prove_multi(c.pub, c.prv, [0, 1]) == c.ref[:2]
        with pytest.raises(dvp.DvpError) as e:
            mp.trace_last(dvp.proving.TRACE_POINTS)
        assert e.value.status == EINVAL
        assert mp.prove(c.pub, c.prv) == c.ref[0]
        mp.select_srs(1)  # as after an SRS setter
        with pytest.raises(dvp.DvpError) as e:
            mp.trace_last(dvp.proving.TRACE_POINTS)
        assert e.value.status == EINVAL
        mp.select_srs(2)
        assert mp.prove_multi(c.pub, c.prv, [0, 2])[1] == c.ref[2] and mp.active_srs() == 2
        assert mp.trace_last(dvp.proving.TRACE_POINTS)["commit_p"]["enc"] == c.ref[2].commit_p
        mp.close()


def test_binding_is_per_slot(dvp, dense8):
    """item 5: slot 1 bound to its own SRS hash, slot 0 left at the default, both proven by one prove_multi"""
    c, S = dense8, dvp.srs
    mp = c.multi(dvp)
    mp.select_srs(1)
    h1 = mp.srs_hash()
    assert h1 == o.blake3(c.payload(dvp, 1))
    mp.set_transcript_binding(h1, None)
    mp.select_srs(0)
    p0, p1 = mp.prove_multi(c.pub, c.prv, [0, 1])
    mp.close()
    assert p0 == c.ref[0] and p1.commit_p == c.ref[1].commit_p and p1 != c.ref[1]
    assert S.verify_batch(c.tds[0], [c.pub], [p0]).tolist() == [0]
    assert S.verify_batch(c.tds[1], [c.pub], [p1]).tolist() == [S.VERIFY_EQUATION]
    try:
        S.set_verify_binding(h1, None)
        assert S.verify_batch(c.tds[1], [c.pub], [p1]).tolist() == [0]
        assert S.verify_batch(c.tds[0], [c.pub], [p0]).tolist() == [S.VERIFY_EQUATION]
    finally:
        S.set_verify_binding(None, None)


def test_errors(dvp, nat, dense8):
    """item 6"""
    c = dense8
    mp = c.multi(dvp)
    with pytest.raises(dvp.DvpError) as e:
        mp.prove_multi(c.pub, c.prv, [0, 1, 7])
    assert (e.value.status, e.value.index) == (EINVAL, 2)
    with pytest.raises(dvp.DvpError) as e:
        mp.prove_multi(c.pub, c.prv, [])
    assert e.value.status == EINVAL
    with pytest.raises(dvp.DvpError) as e:
        mp.drop_srs(0)  # the active slot
    assert e.value.status == EINVAL
    with pytest.raises(dvp.DvpError) as e:
        mp.drop_srs(9)
    assert e.value.status == EINVAL
    with pytest.raises(dvp.DvpError) as e:
        mp.select_srs(3)
    assert e.value.status == EINVAL
    # an incomplete slot (four of five vectors): its status only
    k = mp.add_srs()
    assert k == 3
    mp.select_srs(k)
    for which, (xy, inf) in enumerate(c.srss[1].as_list()[:4]):
        mp.set_srs_encoded(which, dvp.curve.to_bytes(xy, inf))
    mp.select_srs(0)
    got = mp.prove_multi(c.pub, c.prv, [0, 3, 2])
    assert got[0] == c.ref[0] and got[2] == c.ref[2]
    assert isinstance(got[1], dvp.DvpError) and got[1].status == EINVAL
    got = mp.prove_multi(c.pub, c.prv, [3, 1])  # the incomplete slot first: phase 1 runs with the first complete one
    assert isinstance(got[0], dvp.DvpError) and got[1] == c.ref[1] and mp.active_srs() == 0
    # a dropped slot is as unknown as one never handed out
    mp.drop_srs(3)
    with pytest.raises(dvp.DvpError) as e:
        mp.prove_multi(c.pub, c.prv, [1, 3])
    assert (e.value.status, e.value.index) == (EINVAL, 1)
    # an unsatisfied witness: the row the witness check names, and the proofs untouched
    bad = list(c.prv)
    bad[3] = (bad[3] + 1) % o.P
    row = mp.check_witness(c.pub, bad).first_unsat
    assert row >= 0
    pub, prv = dvp.proving._fr_arg(c.pub), dvp.proving._fr_arg(bad)
    slots = np.array([0, 1, 2], dtype=np.uint32)
    out, st = np.full((3, 118), 0xA5, dtype=np.uint8), np.zeros(3, dtype=np.int32)
    rc = dvp.lib.dvp_prove_multi(mp._h, nat.ptr(slots), 3, nat.ptr(pub) if pub.shape[0] else None, pub.shape[0], nat.ptr(prv), prv.shape[0],
                                 nat.ptr(out), nat.ptr(st))
    assert (rc, dvp.lib.dvp_last_error_index()) == (EUNSAT, row)
    assert (out == 0xA5).all() and mp.active_srs() == 0
    with pytest.raises(dvp.DvpError) as e:
        mp.prove(c.pub, bad)
    assert (e.value.status, e.value.index) == (EUNSAT, row)  # what a single proof says
    assert mp.prove_multi(c.pub, c.prv) == c.ref
    mp.close()


def test_slots_and_device_lists_exclude_each_other(dvp, dense8):
    """item 6, last line: a second slot under a two-entry device list, and a two-entry list while a prover holds a second slot"""
    c = dense8
    mp = dvp.proving.Prover(c.inst)
    mp.set_srs(c.srss[0])
    try:
        dvp.set_devices([0, 0])
        with pytest.raises(dvp.DvpError) as e:
            mp.add_srs()
        assert e.value.status == EINVAL and mp.srs_slots() == [0]
        assert mp.prove(c.pub, c.prv) == c.ref[0]  # the sharded path is what it was
    finally:
        dvp.set_devices([])
    k = mp.add_srs(c.srss[1])
    try:
        with pytest.raises(dvp.DvpError) as e:
            dvp.set_devices([0, 0])
        assert e.value.status == EINVAL
        dvp.set_devices([0])  # a single device is no list
        assert mp.prove_multi(c.pub, c.prv) == c.ref[:2]
        mp.drop_srs(k)
        dvp.set_devices([0, 0])  # one slot again: allowed
        assert mp.prove(c.pub, c.prv) == c.ref[0]
    finally:
        dvp.set_devices([])
    k = mp.add_srs()
    mp.close()  # a prover that goes with two slots no longer stands in the way
    try:
        dvp.set_devices([0, 0])
    finally:
        dvp.set_devices([])


def test_accounting(dvp, dense8):
    """item 7: what a slot holds on the device"""
    c = dense8
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        mp = dvp.proving.Prover(c.inst)
        mp.set_srs(c.srss[0])
        bases = 64 * (c.inst.n_wires + 5 * mp.m) + (c.inst.n_wires + 5 * mp.m)  # the points and their flag bytes
        assert mp.srs_slot_bytes(0) == (bases, 0)
        k = mp.add_srs()
        assert mp.srs_slot_bytes(k) == (0, 0)
        mp.select_srs(k)
        assert mp.srs_slot_bytes(k) == (0, 0)
        mp.set_srs(c.srss[1])
        assert mp.srs_slot_bytes(k) == (bases, 0)
        mp.select_srs(0)
        assert mp.srs_slot_bytes(k) == (bases, 0)
        z = mp.add_srs(c.srss[2])
        mp.select_srs(z)
        mp.set_table_budget(0)
        mp.select_srs(0)
        assert mp.prove_multi(c.pub, c.prv) == c.ref
        for j in (0, k):
            mp.select_srs(j)
            held = mp.msm_table(0)[0] + mp.msm_table(1)[0]
            assert held > 0 and mp.srs_slot_bytes(j) == (bases, held)
        mp.select_srs(0)
        assert mp.srs_slot_bytes(k)[1] == mp.srs_slot_bytes(0)[1]  # parked or active: the same answer
        assert mp.srs_slot_bytes(z) == (bases, 0)  # budget 0: no tables, ever
        assert mp.prove_multi(c.pub, c.prv, [z]) == [c.ref[2]] and mp.srs_slot_bytes(z) == (bases, 0)
        mp.drop_srs(k)
        assert mp.srs_slot_bytes(k) == (0, 0)
        with pytest.raises(dvp.DvpError):
            mp.srs_slot_bytes(9)
        mp.close()
