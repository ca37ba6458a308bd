"""GPU tests (-m gpu): Proof::prove on degenerate circuits and on challenges that collide with a domain, bit-exact against the oracle.

  * every case of prove_edge_cases.py (what each is for: that file; what the oracle says of it: test_prove_edge_cases_cpu.py) through
    the comparison of test_gpu_prove.py -- setup scalars, tables, every stage vector, alpha a0 b0 i0 r0, both commitments, the verdict
    -- and then the same 118 bytes and the same stage vectors through every flavour of a proof: host witness, device witness under
    the device and the host transcript, both routes for i(X) on D', fixed-base tables at these tiny sizes.
  * the sharded challenge (dvp_prove_challenge_partial / _finish) at cuts chosen here: an empty rank, cuts inside k_b and between a
    D_i entry of k_r and its D'_i entry.
  * Prover.force_alpha (dvp_prover_debug_force_alpha): the hook changes nothing but alpha; alpha in D u D' is DVP_ECHALLENGE with the
    index from every entry that derives a challenge; the setup refuses tau in D u D'.
No test provokes a fault: a challenge or a tau inside a domain is an input the library is specified to refuse with a status, and the
batch inversion maps the zero denominator to zero."""
import functools
import os
import random

import numpy as np
import pytest

import pyref as o
import c_oracle as co
import msm_cases as mc
import prove_edge_cases as ec
from prove_parity import check_against_oracle, rows_of, STAGE_VECTORS, STAGE_SCALARS
from util import from_limbs

pytestmark = pytest.mark.gpu
P = o.P
EINVAL, EUNSAT, ECHALLENGE = -1, -3, -8
TRANSCRIPT_DEV_MAX_PUB = 35


def stages(pv, names=STAGE_VECTORS + STAGE_SCALARS):
    return {k: from_limbs(pv.debug(k)) for k in names}


def want_stages(pr, names=STAGE_VECTORS + STAGE_SCALARS):
    return {k: (pr[k] if k in STAGE_VECTORS else [pr[k]]) for k in names}


def on_device(dvp, w):
    import torch

    return torch.from_numpy(dvp.fr.vec(w).view(np.int64)).cuda()


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def enc(dl):
    return co.xsk233_encode(co.k233_mulgen(dl))


# ---- 2: every case, every flavour ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_case_against_oracle_in_every_flavour(dvp, case):
    inst = case.inst()
    tree, st, pr = ec.oracle(case)
    pv, td, proof = check_against_oracle(dvp, inst, case.public, case.private, case.trapdoor, verifies=case.verifies, oracle=(tree, st, pr))
    want = want_stages(pr)
    assert stages(pv) == want
    assert (proof.commit_p == bytes(30), proof.kzg_k == bytes(30)) == (case.commit_neutral, case.kzg_neutral)
    horner = case.n_public <= case.m and case.n_public <= 48
    assert pv.extend_count() == (3 if horner else 4)
    if case.name in ("pub-48", "pub-49"):
        assert pv.extend_count() == {"pub-48": 3, "pub-49": 4}[case.name]
    if case.name == "all-neutral":
        assert proof.to_bytes()[:60] == bytes(60) and proof.to_bytes() == bytes(118) and dvp.srs.verify(td, case.public, proof)
    srs = dvp.srs.verifier_runs_setup(pv, inst, td)
    w = on_device(dvp, case.witness)

    def same(label, run, n_ext=None, **knobs):
        """a fresh prover under the knobs gives the same bytes and stage vectors -- and took the path the flavour is named for"""
        with dvp.tune(**knobs):
            q = dvp.proving.Prover(inst)
            q.set_srs(srs)
            assert n_ext is None or q.extend_count() == n_ext, label
            dvp.lib.dvp_profile_reset()
            got = run(q)
            ran = {k: mc.launches(dvp, k) for k in ("prove.hip:k_transcript", "prove.hip:k_quotient<true>", "prove.hip:k_quotient<false>", "msm.hip:k_dbl_table")}
            assert got == proof, label
            assert stages(q) == want, label
            on_dev = case.n_public <= TRANSCRIPT_DEV_MAX_PUB and not knobs.get("DVP_PROVE_HOST_TRANSCRIPT")
            by_horner = q.extend_count() == 3
            tables = 2 if knobs.get("DVP_MSM_FIXED_MIN") == 1 else 0  # one per MSM, built by the first proof; none at these sizes otherwise
            assert ran == {"prove.hip:k_transcript": int(on_dev), "prove.hip:k_quotient<true>": int(by_horner),
                           "prove.hip:k_quotient<false>": int(not by_horner), "msm.hip:k_dbl_table": tables}, label
            q.close()

    dev = lambda q: q.prove_dev(w.data_ptr(), stream())
    host = lambda q: q.prove(case.public, case.private)
    same("prove_dev", dev)  # the device transcript up to TRANSCRIPT_DEV_MAX_PUB public inputs, the host's beyond
    same("prove_dev, host transcript", dev, DVP_PROVE_HOST_TRANSCRIPT=1)
    for run, name in ((host, "prove"), (dev, "prove_dev")):
        same(name + ", i extended", run, n_ext=4 if case.n_public else 3, DVP_HORNER_MAX_PUB=0)  # no public input: i = 0 either way
        if case.n_public <= case.m:
            same(name + ", i by Horner", run, n_ext=3, DVP_HORNER_MAX_PUB=1000)
        else:  # no knob may take the Horner route where i(X) on D' is not what the reference extends
            same(name + ", Horner asked for beyond m", run, n_ext=4, DVP_HORNER_MAX_PUB=1000)
        same(name + ", fixed-base tables", run, DVP_MSM_FIXED_MIN=1)
    # the same prover again, after all of the above on its siblings
    assert pv.prove(case.public, case.private) == proof and dev(pv) == proof
    pv.close()


@pytest.mark.parametrize("name", ["m2", "m4-padded"])
def test_unsatisfied_rows_at_the_smallest_sizes(dvp, name):
    """the row reported is the FIRST unsatisfied one, also when it is the last real row (m4-padded: the row before the padding)"""
    case = ec.BY_NAME[name]
    inst = case.inst()
    pv = dvp.proving.Prover(inst)
    pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, dvp.srs.Trapdoor(*case.trapdoor)))
    ref = pv.prove(case.public, case.private)
    assert ref.commit_p == enc(ec.oracle(case)[2]["dl_commit_p"])
    last = len(case.rows) - 1
    w = case.witness
    if name == "m2":  # x x = y, y 1 = z
        only_last = w[:3] + [w[3] + 1]
        first_and_last = w[:2] + [w[2] + 1, w[3]]
    else:             # x x = y, y x = z, (z + x) 1 = out
        only_last = [1, w[1] + 1] + w[2:]
        first_and_last = [1, w[1] + 1, w[2], w[3] + 1, w[4]]
    for bad, row in ((only_last, last), (first_and_last, 0)):
        failing = [r for r, sides in enumerate(case.rows)
                   if o.eval_row(sides[0], case.coeffs, bad) * o.eval_row(sides[1], case.coeffs, bad) % P != o.eval_row(sides[2], case.coeffs, bad)]
        assert failing[0] == row and failing[-1] == last
        d_bad = on_device(dvp, bad)
        for host in (0, 1):
            with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=host):
                for run in (lambda: pv.prove(bad[1:1 + case.n_public], bad[1 + case.n_public:]), lambda: pv.prove_dev(d_bad.data_ptr(), stream())):
                    with pytest.raises(dvp.DvpError) as ei:
                        run()
                    assert (ei.value.status, ei.value.index) == (EUNSAT, row)
    assert pv.prove(case.public, case.private) == ref  # the prover is usable afterwards
    pv.close()


# ---- the sharded challenge at cuts chosen here --------------------------------------------------------------------------------------------
CUTS = {
    # 4m = 8: S = [k_a 0..2 | k_b 2..4 | k_r 4..8].  The second rank is empty on both counts; the first cut falls inside k_b; the third
    # rank's K range starts inside k_b and covers all of k_r
    "m2": [((0, 1), (0, 3)), ((1, 1), (3, 3)), ((1, 2), (3, 8))],
    # 4m = 16: k_r = 8..16, interleaved [D_i, D'_i].  The cuts at 9 and 13 are odd: between a D_i entry and its D'_i entry, so the ranks
    # on both sides need index i (of D on one side, of D' on the other); the cut at 10 lies between D'_0 and D_1.  The last rank has no
    # barycentric slice
    "m4-padded": [((0, 1), (0, 9)), ((1, 2), (9, 10)), ((2, 4), (10, 13)), ((4, 4), (13, 16))],
}


def sharded(dvp, inst, srs, w, cuts, forced=None):
    """one fresh prover per rank (its den, den2 and S hold nothing outside the rank's share): begin, the commitment, part 1 with the
    rank's (barycentric, K) ranges, the records stacked as the all-gather would, part 2.  Returns the backends and the stacked partial
    K points."""
    import torch

    dev = torch.device("cuda", 0)
    ranks = []
    for _ in cuts:
        q = dvp.proving.Prover(inst)
        q.set_srs(srs)
        if forced is not None:
            q.force_alpha(forced)
        ranks.append(dvp.distributed.GpuBackend(q, dev))
    for be in ranks:
        be.begin(w, True)
    commit = ranks[0].msm_partial(0, 0, ranks[0].msm_size(0)).clone()
    recs = [be.challenge_partial(commit, d_rng, k_rng).clone() for be, (d_rng, k_rng) in zip(ranks, cuts)]
    gathered = torch.stack(recs)
    parts = []
    for r, (be, (_, k_rng)) in enumerate(zip(ranks, cuts)):
        be.challenge_finish(gathered[list(range(r, len(cuts))) + list(range(r))], k_rng)  # the order of the records does not matter
        parts.append(be.msm_partial(1, *k_rng).clone())
    return ranks, torch.stack(parts)


@pytest.mark.parametrize("name", sorted(CUTS))
def test_sharded_challenge_at_chosen_cuts(dvp, name):
    case = ec.BY_NAME[name]
    inst = case.inst()
    pr = ec.oracle(case)[2]
    m, cuts = case.m, CUTS[name]
    assert [c[1] for c in cuts][0][0] == 0 and cuts[-1][1][1] == 4 * m and all(a[1][1] == b[1][0] and a[0][1] == b[0][0] for a, b in zip(cuts, cuts[1:]))
    assert cuts[0][0][0] == 0 and cuts[-1][0][1] == m
    pv = dvp.proving.Prover(inst)
    srs = dvp.srs.verifier_runs_setup(pv, inst, dvp.srs.Trapdoor(*case.trapdoor))
    pv.set_srs(srs)
    ref = pv.prove(case.public, case.private)
    assert ref.commit_p == enc(pr["dl_commit_p"]) and ref.kzg_k == enc(pr["dl_kzg"])
    w = on_device(dvp, case.witness)
    ranks, parts = sharded(dvp, inst, srs, w, cuts)
    for r, (be, (_, (k_lo, k_hi))) in enumerate(zip(ranks, cuts)):
        got = stages(be.prover, ("a0", "b0", "i0", "r0", "ka", "kb", "kr"))
        assert [got[n][0] for n in ("a0", "b0", "i0", "r0")] == [pr[n] for n in ("a0", "b0", "i0", "r0")], r
        assert (got["ka"] + got["kb"] + got["kr"])[k_lo:k_hi] == pr["s_k"][k_lo:k_hi], r
    kzg = ranks[0].combine(parts)
    for be in ranks:  # every rank holds a0, b0 and the commitment: each assembles the same bytes
        assert be.finish(kzg) == ref
        be.prover.close()
    pv.close()


# ---- 3: the forced challenge ------------------------------------------------------------------------------------------------------------------
class Forced:
    """a circuit, its oracle setup, a prover with the SRS and the proof it gives unforced; oracle(alpha) = pyref.prove_scalars under
    alpha_fn = lambda _: alpha, the four extends (they do not depend on alpha) computed once"""

    def __init__(self, dvp, inst, pub, prv, trap):
        self.dvp, self.inst, self.pub, self.prv, self.trap = dvp, inst, list(pub), list(prv), trap
        self.td = dvp.srs.Trapdoor(*trap)
        self.m = inst.num_constraints
        self.tree = o.FFTree(self.m.bit_length())
        self.st = o.setup_srs_scalars(self.tree, rows_of(inst), from_limbs(inst.coeffs), inst.num_public_inputs, trap)
        self.D, self.D2 = self.st["tables"]["D"], self.st["tables"]["D2"]
        extend, memo = self.tree.extend, {}

        def extend_once(v):
            key = tuple(v)
            if key not in memo:
                memo[key] = extend(v)
            return memo[key]

        self.tree.extend = extend_once
        self.pv = self.prover()
        self.w = on_device(dvp, [1] + self.pub + self.prv)
        self.ref = self.pv.prove(self.pub, self.prv)
        assert dvp.srs.verify(self.td, self.pub, self.ref)

    @functools.lru_cache(maxsize=None)
    def srs(self):
        q = self.dvp.proving.Prover(self.inst)
        s = self.dvp.srs.verifier_runs_setup(q, self.inst, self.td)
        q.close()
        return s

    def prover(self, forced=None):
        q = self.dvp.proving.Prover(self.inst)
        q.set_srs(self.srs())
        if forced is not None:
            q.force_alpha(forced)
        return q

    @functools.lru_cache(maxsize=None)
    def oracle(self, alpha):
        return o.prove_scalars(self.tree, self.st, self.pub, self.prv, lambda _: alpha)

    def collisions(self):
        """(alpha, index): D[i] and D'[i] at both ends, and across the seam of the two 256-lane blocks where there are two"""
        idx = [0, self.m - 1] + ([255, 256] if self.m == 512 else [])
        return [(dom[i], i) for i in idx for dom in (self.D, self.D2)]


@pytest.fixture(scope="module", params=["m4-padded", "dense9"])
def forced(request, dvp):
    if request.param == "dense9":
        inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(9)
        rnd = random.Random(909)
        f = Forced(dvp, inst, pub, prv, tuple(rnd.randrange(1, P) for _ in range(3)))
        assert f.m == 512
    else:
        case = ec.BY_NAME[request.param]
        f = Forced(dvp, case.inst(), case.public, case.private, case.trapdoor)
    yield f
    f.pv.close()


def test_forced_alpha_changes_nothing_else(dvp, forced):
    f = forced
    names = ("alpha", "a0", "b0", "i0", "r0", "ka", "kb", "kr")
    with pytest.raises(dvp.DvpError) as ei:
        f.pv.force_alpha(P)
    assert ei.value.status == EINVAL
    assert f.pv.prove(f.pub, f.prv) == f.ref  # a refused value forces nothing
    for alpha in (5, f.D[0] + 1):
        assert alpha not in f.D and alpha not in f.D2
        pr = f.oracle(alpha)
        f.pv.force_alpha(alpha)
        runs = [("prove", {}, lambda: f.pv.prove(f.pub, f.prv)), ("prove_dev", {}, lambda: f.pv.prove_dev(f.w.data_ptr(), stream())),
                ("prove_dev, host transcript", {"DVP_PROVE_HOST_TRANSCRIPT": 1}, lambda: f.pv.prove_dev(f.w.data_ptr(), stream()))]
        for label, knobs, run in runs:
            with dvp.tune(**knobs):
                dvp.lib.dvp_profile_reset()
                proof = run()
            assert mc.launches(dvp, "prove.hip:k_transcript") == 0, (alpha, label)  # the device flavour copies the pair in instead
            assert stages(f.pv, names) == want_stages(pr, names), (alpha, label)
            assert proof.commit_p == f.ref.commit_p == enc(pr["dl_commit_p"]) and proof.kzg_k == enc(pr["dl_kzg"]), (alpha, label)
            assert proof.a0_fr() == (pr["a0"], True) and proof.b0_fr() == (pr["b0"], True), (alpha, label)
        f.pv.force_alpha(None)
        dvp.lib.dvp_profile_reset()
        assert f.pv.prove(f.pub, f.prv) == f.ref and f.pv.prove_dev(f.w.data_ptr(), stream()) == f.ref
        assert mc.launches(dvp, "prove.hip:k_transcript") == 2  # unset, the hook leaves the launches of a proof as they were


def phased(f, q):
    import torch

    be = f.dvp.distributed.GpuBackend(q, torch.device("cuda", 0))
    be.begin(f.w, True)
    commit = be.msm_partial(0, 0, be.msm_size(0)).clone()
    be.challenge(commit)
    return be.finish(be.msm_partial(1, 0, be.msm_size(1)).clone())


def test_challenge_in_a_domain_is_refused_with_its_index(dvp, forced):
    """DVP_ECHALLENGE (src/proving.rs:548-556) from dvp_prove, both transcript flavours of dvp_prove_dev and dvp_prove_finish after the
    phased entries; then the same prover, unforced, gives the bytes it gave before"""
    f = forced
    assert f.inst.num_public_inputs <= TRANSCRIPT_DEV_MAX_PUB  # so the default flavour of prove_dev is the device transcript
    q = f.prover()
    runs = [("prove", {}, lambda: q.prove(f.pub, f.prv)), ("prove_dev", {}, lambda: q.prove_dev(f.w.data_ptr(), stream())),
            ("prove_dev, host transcript", {"DVP_PROVE_HOST_TRANSCRIPT": 1}, lambda: q.prove_dev(f.w.data_ptr(), stream())),
            ("begin / challenge / finish", {}, lambda: phased(f, q))]
    for alpha, i in f.collisions():
        q.force_alpha(alpha)
        for label, knobs, run in runs:
            with dvp.tune(**knobs):
                with pytest.raises(dvp.DvpError) as ei:
                    run()
            assert (ei.value.status, ei.value.index) == (ECHALLENGE, i), (label, i)
    q.force_alpha(None)
    for label, knobs, run in runs:
        with dvp.tune(**knobs):
            assert run() == f.ref, label
    q.close()


def test_unsatisfied_row_comes_before_the_challenge(dvp, forced):
    """the deferred flavour reports from one block, in the reference's order: the unsatisfied row (src/proving.rs:389-395) before
    alpha in D u D' (:548-556)"""
    f = forced
    q = f.prover(f.D[f.m - 1])
    bad = [1] + f.pub + f.prv
    bad[-1] = (bad[-1] + 1) % P
    d_bad = on_device(dvp, bad)
    for host in (0, 1):
        with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=host):
            with pytest.raises(dvp.DvpError) as ei:
                q.prove_dev(d_bad.data_ptr(), stream())
            assert ei.value.status == EUNSAT and 0 <= ei.value.index < f.inst.n_rows
            with pytest.raises(dvp.DvpError) as ei:
                q.prove_dev(f.w.data_ptr(), stream())
            assert (ei.value.status, ei.value.index) == (ECHALLENGE, f.m - 1)
    q.close()


def test_sharded_challenge_in_a_domain(dvp, forced):
    """the hit flag through k_alpha_denoms_range, k_bary3_record and k_bary3_from_records: whichever rank's share holds the hit, after
    _finish every rank answers DVP_ECHALLENGE with the index (the minimum over the records)"""
    f = forced
    m = f.m
    if m == 4:
        cuts = CUTS["m4-padded"]
        # D[0]: the first rank's barycentric slice.  D[3]: the last rank's K range (k_r entries 13..15 = D'_2, D_3, D'_3).  D'[1]: k_r
        # entry 11, an odd position, inside the third rank's K range alone -- the ranks beside it stop at D'_0 and start at D'_2
        placements = [(f.D[0], 0), (f.D[3], 3), (f.D2[1], 1)]
    else:
        # k_r = 1024..2048.  Rank 1 reads k_r entries 3, 4, 5 = D'_1, D_2, D'_2; rank 0 stops at D_1, rank 2 starts at D_3
        cuts = [((0, 256), (0, 1027)), ((256, 300), (1027, 1030)), ((300, 512), (1030, 2048))]
        placements = [(f.D[255], 255), (f.D[511], 511), (f.D2[2], 2)]
    for alpha, i in placements:
        ranks, parts = sharded(dvp, f.inst, f.srs(), f.w, cuts, forced=alpha)
        kzg = ranks[0].combine(parts)
        for r, be in enumerate(ranks):
            with pytest.raises(dvp.DvpError) as ei:
                be.finish(kzg)
            assert (ei.value.status, ei.value.index) == (ECHALLENGE, i), (i, r)
            be.prover.close()


def test_prove_multi_reports_the_challenge_per_slot(dvp, forced):
    """dvp_prove_multi_dev with two SRS slots: alpha in D u D' is each slot's own outcome (status[j]), not the witness's -- the call
    itself succeeds and goes on to the next slot"""
    f = forced
    rnd = random.Random(31)
    td2 = dvp.srs.Trapdoor(*(rnd.randrange(1, P) for _ in range(3)))
    q = f.prover()
    ref2_prover = dvp.proving.Prover(f.inst)
    srs2 = dvp.srs.verifier_runs_setup(ref2_prover, f.inst, td2)
    ref2_prover.set_srs(srs2)
    ref2 = ref2_prover.prove(f.pub, f.prv)
    ref2_prover.close()
    assert q.add_srs(srs2) == 1
    for host in (0, 1):
        with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=host):
            assert q.prove_multi_dev(f.w.data_ptr(), [0, 1], stream()) == [f.ref, ref2]
            q.force_alpha(f.D2[0])
            for got in (q.prove_multi_dev(f.w.data_ptr(), [0, 1], stream()), q.prove_multi(f.pub, f.prv, [1, 0])):
                assert [type(x) for x in got] == [dvp.DvpError] * 2 and [x.status for x in got] == [ECHALLENGE] * 2
            q.force_alpha(None)
            assert q.prove_multi_dev(f.w.data_ptr(), [1, 0], stream()) == [ref2, f.ref]
    q.close()


# ---- tau in a domain ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m2", "pub-48"])
def test_setup_refuses_tau_in_a_domain(dvp, name, tmp_path):
    """src/ec_fft.rs:350: tau in D u D' has no Lagrange basis at tau; dvp_setup_scalars, verifier_runs_setup and dvp_setup_cache_dir
    answer DVP_EINVAL, and the neighbour D[0] + 1 is an ordinary tau"""
    case = ec.BY_NAME[name]
    assert case.log_m == {"m2": 1, "pub-48": 6}[name]
    inst = case.inst()
    tree = ec.oracle(case)[0]
    D, D2 = tree.both_domains()
    m = case.m
    _, delta, eps = case.trapdoor
    pv = dvp.proving.Prover(inst)
    for tau in (D[0], D[m - 1], D2[0], D2[m - 1]):
        td = dvp.srs.Trapdoor(tau, delta, eps)
        for setup in (dvp.srs.srs_scalars, dvp.srs.verifier_runs_setup):
            with pytest.raises(dvp.DvpError) as ei:
                setup(pv, inst, td)
            assert ei.value.status == EINVAL
    from importlib import import_module
    A = import_module("dv-pari_amd.artifacts")
    inst.write_dump_file(os.path.join(tmp_path, A.R1CS_CONSTRAINTS_FILE))
    with pytest.raises(dvp.DvpError) as ei:
        dvp.srs.verifier_runs_setup_cache_dir(dvp.srs.Trapdoor(D2[m - 1], delta, eps), tmp_path, case.n_public)
    assert ei.value.status == EINVAL
    assert not [n for n in A.SRS_FILES if os.path.exists(os.path.join(tmp_path, n))]
    tau = D[0] + 1
    assert tau not in D and tau not in D2
    st = o.setup_srs_scalars(tree, case.rows, case.coeffs, case.n_public, (tau, delta, eps))
    g_m, g_q, g_k = dvp.srs.srs_scalars(pv, inst, dvp.srs.Trapdoor(tau, delta, eps))
    assert from_limbs(g_m) == ec.gm_padded(case, st) and from_limbs(g_q) == st["g_q"]
    assert [from_limbs(v) for v in g_k] == st["g_k"]
    pv.close()
