"""GPU tests (-m gpu) of the transcript binding: the SRS hash of a prover against the oracle's stream, bound proofs against the
oracle's prover run with a bound challenge, the same bound bytes through every path that derives alpha, the verifier under the same,
the default and a swapped binding, and forged batches under the binding."""
import json
import os
import random
import struct

import numpy as np
import pytest

import pyref as o
import c_oracle as co
import binding_cases as bc
import verify_cases as vc
from util import from_limbs

pytestmark = pytest.mark.gpu
VEC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_vectors.json")))
CIRCUIT_HASH = bytes((7 * i + 3) % 256 for i in range(32))  # an arbitrary circuit hash: the caller's to define


def rows_of(inst):
    rows = []
    for i in range(inst.n_rows):
        row = []
        for mt in (inst.l, inst.r, inst.o):
            a, b = int(mt.row_ptr[i]), int(mt.row_ptr[i + 1])
            row.append([(int(mt.wire[k]), int(mt.coeff[k])) for k in range(a, b)])
        rows.append(tuple(row))
    return rows


class Case:
    """a circuit with its oracle setup, a prover holding the SRS, and the oracle's SRS stream"""

    def __init__(self, dvp, inst, pub, prv, trap):
        self.inst, self.pub, self.prv, self.trap = inst, pub, prv, trap
        self.td = dvp.srs.Trapdoor(*trap)
        self.pv = dvp.proving.Prover(inst)
        self.tree = o.FFTree(self.pv.log_m + 1)
        self.st = o.setup_srs_scalars(self.tree, rows_of(inst), from_limbs(inst.coeffs), inst.num_public_inputs, trap)
        self.srs = dvp.srs.verifier_runs_setup(self.pv, inst, self.td)
        self.pv.set_srs(self.srs)
        self.stream = bc.srs_stream(self.st, inst.n_wires)

    def fresh_prover(self, dvp):
        q = dvp.proving.Prover(self.inst)
        q.set_srs(self.srs)
        return q


@pytest.fixture(scope="module")
def dense8(dvp):
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(8)
    rnd = random.Random(8)
    c = Case(dvp, inst, pub, prv, (rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P)))
    yield c
    c.pv.close()


@pytest.fixture(scope="module")
def toy(dvp):
    g = dvp.gnark_r1cs
    inst = g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 2)
    c = Case(dvp, inst, list(o.TOY_PUBLIC), list(o.TOY_PRIVATE), tuple(int(x, 16) for x in VEC["toy"]["trapdoor"]))
    yield c
    c.pv.close()


@pytest.fixture(scope="module")
def bound8(dvp, dense8):
    """the bound proof of dense8 on the default path, with the oracle's prover under the same binding"""
    c = dense8
    srs_hash = c.pv.srs_hash()
    assert srs_hash == o.blake3(c.stream)
    ch = bc.challenge_fn(srs_hash, CIRCUIT_HASH)
    pr = o.prove_scalars(c.tree, c.st, c.pub, c.prv, lambda dl: ch(co.xsk233_encode(co.k233_mulgen(dl)), c.pub))
    c.pv.set_transcript_binding(srs_hash, CIRCUIT_HASH)
    try:
        proof = c.pv.prove(c.pub, c.prv)
        mids = {k: from_limbs(c.pv.debug(k))[0] for k in ("alpha", "a0", "b0", "i0", "r0")}
    finally:
        c.pv.set_transcript_binding(None, None)
    return dict(srs_hash=srs_hash, pr=pr, proof=proof, mids=mids)


def test_srs_hash_vs_oracle_stream(dvp, toy, dense8):
    """BLAKE3 of to_bytes() of g_k[0..2], g_q, g_m in that order: the toy circuit (48 points, two chunks) and 2^8 rows; a second
    codec rule hashes the other encodings; DVP_EINVAL until all five vectors are set"""
    assert len(toy.stream) == 48 * 30
    for c in (toy, dense8):
        assert len(c.stream) == 30 * (5 * c.pv.m + c.inst.n_wires)
        assert c.pv.srs_hash() == o.blake3(c.stream)
        assert c.pv.srs_hash() == dvp.proving.blake3(c.stream)
    rule = 1
    dvp.check(dvp.lib.dvp_codec_set_rule(rule))
    try:
        other = bc.srs_stream(toy.st, toy.inst.n_wires, rule)
        assert other != toy.stream
        assert toy.pv.srs_hash() == o.blake3(other)
    finally:
        dvp.check(dvp.lib.dvp_codec_set_rule(0))
    assert toy.pv.srs_hash() == o.blake3(toy.stream)
    # incomplete SRS
    q = dvp.proving.Prover(toy.inst)
    with pytest.raises(dvp.DvpError) as e:
        q.srs_hash()
    assert e.value.status == -1
    for which, (xy, inf) in enumerate(toy.srs.as_list()[:4]):
        q.set_srs_encoded(which, dvp.curve.to_bytes(xy, inf))
    with pytest.raises(dvp.DvpError) as e:
        q.srs_hash()
    assert e.value.status == -1
    xy, inf = toy.srs.as_list()[4]
    q.set_srs_encoded(4, dvp.curve.to_bytes(xy, inf))
    assert q.srs_hash() == o.blake3(toy.stream)  # and a prover fed the file payloads hashes to the same
    q.close()


def test_bound_proof_vs_oracle_prover(dvp, dense8, bound8):
    c, pr, proof = dense8, bound8["pr"], bound8["proof"]
    assert bound8["mids"] == {k: pr[k] for k in ("alpha", "a0", "b0", "i0", "r0")}
    assert proof.commit_p == co.xsk233_encode(co.k233_mulgen(pr["dl_commit_p"]))
    assert proof.kzg_k == co.xsk233_encode(co.k233_mulgen(pr["dl_kzg"]))
    assert proof.a0_fr() == (pr["a0"], True) and proof.b0_fr() == (pr["b0"], True)
    assert pr["alpha"] == bc.bound_challenge(proof.commit_p, c.pub, bound8["srs_hash"], CIRCUIT_HASH)
    assert pr["alpha"] != o.transcript_challenge(proof.commit_p, c.pub)
    assert o.verify_dl(c.trap, c.pub, pr["dl_commit_p"], pr["dl_kzg"], pr["a0"], pr["b0"], pr["alpha"])
    # clearing the binding returns the prover to the unbound bytes (what test_gpu_prove.py::test_synthetic_2_8_vs_oracle pins)
    unbound = c.pv.prove(c.pub, c.prv)
    pr0 = o.prove_scalars(c.tree, c.st, c.pub, c.prv, lambda dl: o.transcript_challenge(co.xsk233_encode(co.k233_mulgen(dl)), c.pub))
    assert unbound.commit_p == proof.commit_p  # the commitment does not depend on the challenge
    assert unbound.kzg_k == co.xsk233_encode(co.k233_mulgen(pr0["dl_kzg"])) != proof.kzg_k
    assert unbound.a0_fr() == (pr0["a0"], True) and unbound.b0_fr() == (pr0["b0"], True)
    assert from_limbs(c.pv.debug("alpha"))[0] == pr0["alpha"]


def test_verifier_follows_the_binding(dvp, dense8, bound8):
    """accepted by all three verify flavours under the same pair; exactly DVP_VERIFY_EQUATION under the default and under the swapped
    pair; an unbound proof is rejected the same way by the bound verifier"""
    S, c, proof = dvp.srs, dense8, bound8["proof"]
    s = bound8["srs_hash"]
    unbound = c.pv.prove(c.pub, c.prv)

    def verdicts(p):
        v1 = S.verify_batch(c.td, [c.pub], [p])
        v2, _ = S.verify_batch_rlc(c.td, [c.pub], [p])
        return S.verify(c.td, c.pub, p), int(v1[0]), int(v2[0])

    assert verdicts(proof) == (False, S.VERIFY_EQUATION, S.VERIFY_EQUATION)  # default binding
    assert verdicts(unbound) == (True, 0, 0)
    try:
        S.set_verify_binding(s, CIRCUIT_HASH)
        assert verdicts(proof) == (True, 0, 0)
        assert S.verify_device(c.td, c.pub, proof)
        assert verdicts(unbound) == (False, S.VERIFY_EQUATION, S.VERIFY_EQUATION)
        S.set_verify_binding(CIRCUIT_HASH, s)
        assert verdicts(proof) == (False, S.VERIFY_EQUATION, S.VERIFY_EQUATION)
    finally:
        S.set_verify_binding(None, None)
    assert verdicts(unbound) == (True, 0, 0)


def test_same_bound_bytes_on_every_path(dvp, dense8, bound8):
    """the host transcript (tune knob), a device list, the phased entries and the index-sharded challenge all read the binding"""
    import torch

    c, ref, s = dense8, bound8["proof"], bound8["srs_hash"]
    dev = torch.device("cuda", 0)
    assignment = torch.from_numpy(dvp.fr.vec([1] + c.pub + c.prv).view(np.int64)).to(dev)
    c.pv.set_transcript_binding(s, CIRCUIT_HASH)
    try:
        assert c.pv.prove(c.pub, c.prv) == ref
        assert c.pv.prove_dev(assignment.data_ptr(), 0) == ref
        with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=1):
            assert c.pv.prove(c.pub, c.prv) == ref
            assert c.pv.prove_dev(assignment.data_ptr(), 0) == ref
        try:
            dvp.set_devices([0, 0])
            assert c.pv.prove(c.pub, c.prv) == ref
            assert c.pv.srs_hash() == s  # hashed from the home copies, whatever the device list
        finally:
            dvp.set_devices([])
        # the debug flavour of the device transcript
        assert c.pv.transcript_dev(ref.commit_p, c.pub)[0] == bound8["pr"]["alpha"]
        # phased: begin -> msm_partial -> challenge -> msm_partial -> finish
        be = dvp.distributed.GpuBackend(c.pv, dev)
        be.begin(assignment, True)
        commit = be.msm_partial(0, 0, be.msm_size(0)).clone()
        be.challenge(commit)
        assert be.finish(be.msm_partial(1, 0, be.msm_size(1)).clone()) == ref
    finally:
        c.pv.set_transcript_binding(None, None)
    # challenge_partial / challenge_finish with two simulated ranks, each on a prover of its own
    world, m = 2, c.pv.m
    plan = dvp.distributed.shard_plan(world, c.inst.n_wires, m)
    ranks = []
    for r in range(world):
        q = c.fresh_prover(dvp)
        q.set_transcript_binding(s, CIRCUIT_HASH)
        ranks.append(dvp.distributed.GpuBackend(q, dev))
    parts = []
    for r, be in enumerate(ranks):
        (lo, hi), _, need = plan[r]
        be.begin(assignment, need)
        parts.append(be.msm_partial(0, lo, hi).clone())
    commit = ranks[0].combine(torch.stack(parts))
    recs = [be.challenge_partial(commit, dvp.distributed.shard_range(m, r, world), plan[r][1]).clone() for r, be in enumerate(ranks)]
    gathered = torch.stack(recs)
    parts = []
    for r, be in enumerate(ranks):
        be.challenge_finish(gathered, plan[r][1])
        parts.append(be.msm_partial(1, *plan[r][1]).clone())
    proof = ranks[0].finish(ranks[0].combine(torch.stack(parts)))
    for be in ranks:
        be.prover.close()
    assert proof == ref


def test_bound_proof_with_36_public_inputs(dvp):
    """n_public = 36 is past the device transcript's one chunk: dvp_prove takes the host transcript, which must read the binding too"""
    S = dvp.srs
    inst0, pub0, prv0 = dvp.gnark_r1cs.synthetic_dense(8)
    extra = 34
    inst = type(inst0)(inst0.num_constraints, 2 + extra, inst0.n_rows, inst0.n_wires, inst0.l, inst0.r, inst0.o, inst0.coeffs)
    pub, prv = pub0 + prv0[:extra], prv0[extra:]
    td = S.Trapdoor(11, 13, 17)
    pv = dvp.proving.Prover(inst)
    pv.set_srs(S.verifier_runs_setup(pv, inst, td))
    unbound = pv.prove(pub, prv)
    assert S.verify(td, pub, unbound)
    s = pv.srs_hash()
    pv.set_transcript_binding(s, CIRCUIT_HASH)
    proof = pv.prove(pub, prv)
    assert from_limbs(pv.debug("alpha"))[0] == bc.bound_challenge(proof.commit_p, pub, s, CIRCUIT_HASH)
    assert proof.commit_p == unbound.commit_p and proof != unbound
    try:
        S.set_verify_binding(s, CIRCUIT_HASH)
        assert S.verify(td, pub, proof) and S.verify_device(td, pub, proof)
        assert int(S.verify_batch(td, [pub], [unbound])[0]) == S.VERIFY_EQUATION
    finally:
        S.set_verify_binding(None, None)
    assert int(S.verify_batch(td, [pub], [proof])[0]) == S.VERIFY_EQUATION
    pv.set_transcript_binding(None, None)
    assert pv.prove(pub, prv) == unbound
    pv.close()


def py_dump(rows, coeffs):
    out = [struct.pack("<I", len(coeffs))] + [int(c).to_bytes(32, "big") for c in coeffs] + [struct.pack("<I", len(rows))]
    for l, r, oo in rows:
        out.append(struct.pack("<III", len(l), len(r), len(oo)))
        for part in (l, r, oo):
            for w, c in part:
                out.append(struct.pack("<II", w, c))
    return b"".join(out)


def test_cache_dir_binding(dvp, toy, tmp_path):
    """dvp_cache_dir_set_binding(bind_srs = 1) on the toy cache_dir: Proof.prove(cache_dir, ..) gives the bytes of a prover bound to
    its own SRS hash, which is the oracle's; clearing restores the golden toy proof"""
    A, g, P = dvp.artifacts, dvp.gnark_r1cs, dvp.proving
    cache = tmp_path / "cache"
    cache.mkdir()
    (cache / A.R1CS_CONSTRAINTS_FILE).write_bytes(py_dump(g.TOY_ROWS, g.TOY_COEFFS))
    inst, pv = dvp.srs.verifier_runs_setup_cache_dir(toy.td, cache, 2)
    try:
        s = pv.srs_hash()
        assert s == o.blake3(toy.stream)
        golden = P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE)
        assert golden.commit_p.hex() == VEC["toy"]["commit_p"] and golden.kzg_k.hex() == VEC["toy"]["kzg_k"]
        pv.set_transcript_binding(s, CIRCUIT_HASH)
        want = pv.prove(g.TOY_PUBLIC, g.TOY_PRIVATE)
        assert want != golden
        P.set_cache_dir_binding(cache, 2, None, CIRCUIT_HASH, bind_srs=True)
        assert P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE) == want
        assert P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE) == want
        try:
            dvp.srs.set_verify_binding(s, CIRCUIT_HASH)
            assert dvp.srs.verify_device(toy.td, g.TOY_PUBLIC, want)
        finally:
            dvp.srs.set_verify_binding(None, None)
        # an explicit SRS hash, and bind_srs = 0 with no hash: the SRS half stays BLAKE3("")
        P.set_cache_dir_binding(cache, 2, s, CIRCUIT_HASH)
        assert P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE) == want
        P.set_cache_dir_binding(cache, 2, None, CIRCUIT_HASH)
        pv.set_transcript_binding(None, CIRCUIT_HASH)
        assert P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE) == pv.prove(g.TOY_PUBLIC, g.TOY_PRIVATE) != want
        P.set_cache_dir_binding(cache, 2, None, None)
        assert P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE) == golden
    finally:
        P.release_cache_dir(cache)
        pv.close()


def test_forged_batch_under_the_binding(dvp):
    """proofs forged without a prover (tests/verify_cases.py) against a bound challenge, some tampered: verify_batch and
    verify_batch_rlc give the oracle's verdicts under the binding, and reject every forged proof under the default"""
    S = dvp.srs
    td = (0x3D9F1A77 * 104729 % o.P, 0xC0FFEE1234567 % o.P, 0xDEADBEEF987654321 % o.P)
    s = o.blake3(b"some srs stream")
    rng = random.Random(77)
    cases = [c for c in vc.CASES if c != "v0_zero"] + [None] * 30
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in cases]
    built = vc.build(td, pubs, cases, seed=5, challenge=bc.challenge_fn(s, CIRCUIT_HASH))
    proofs, rows = [b["proof"] for b in built], [b["pub"] for b in built]
    kinds = ("flip_commit", "flip_kzg", "a0_plus_1", "b0_ge_p", "bad_kzg", "wrong_public", "swap")
    for k, i in enumerate(rng.sample(range(len(built)), 2 * len(kinds))):
        proofs[i], _, rows[i] = vc.tamper(built[i], kinds[k // 2], rng)
    want = [bc.oracle_verdict_bound(td, pub, p, s, CIRCUIT_HASH) for pub, p in zip(rows, proofs)]
    assert sum(want) == len(built) - 2 * len(kinds)
    tdo = S.Trapdoor(*td)
    try:
        S.set_verify_binding(s, CIRCUIT_HASH)
        v = S.verify_batch(tdo, rows, proofs)
        v2, rep = S.verify_batch_rlc(tdo, rows, proofs)
    finally:
        S.set_verify_binding(None, None)
    assert [x == 0 for x in v] == want
    assert (v2 == v).all() and rep == S.VERIFY_RLC_FALLBACK
    # under the default binding only chance could accept one of them
    v = S.verify_batch(tdo, rows, proofs)
    assert v.all()
    assert all(x == S.VERIFY_EQUATION for x, w in zip(v, want) if w)
