"""GPU tests (-m gpu) of dvp_prover_trace_last: the record of a proof against the oracle's restatement of Proof::prove
(pyref.prove_scalars; tests/prove_trace_cases.py) on the toy R1CS and the 2^8 synthetic circuit of test_gpu_prove.py -- every scalar,
every vector digest, every point as (its discrete log) G by the C oracle --, under both Horner routes, both transcript routes and every
table budget; that a trace changes nothing (same bytes afterwards, two traces identical, the launch census of a plain proof); when there
is no trace; and what the record localises."""
import random

import numpy as np
import pytest

import pyref as o
import c_oracle as co
import msm_cases as mc
import prove_trace_cases as tc
from test_gpu_prove import rows_of
from util import from_limbs

pytestmark = pytest.mark.gpu
EINVAL, EUNSAT = -1, -3
HORNER = {"horner": 1 << 20, "extend": 0}  # DVP_HORNER_MAX_PUB: i(X) on D' by Horner / by a fourth extend
TRANSCRIPT = {"device": 0, "host": 1}      # DVP_PROVE_HOST_TRANSCRIPT


class Circuit:
    """a circuit with its SRS, one proof of it and the oracle's restatement of that proof"""

    def __init__(self, dvp, inst, pub, prv, trap):
        self.inst, self.pub, self.prv, self.trap = inst, list(pub), list(prv), trap
        self.td = dvp.srs.Trapdoor(*trap)
        self.pv = dvp.proving.Prover(inst)
        self.tree = o.FFTree(self.pv.log_m + 1)
        self.setup = o.setup_srs_scalars(self.tree, rows_of(inst), from_limbs(inst.coeffs), inst.num_public_inputs, trap)
        self.srs = dvp.srs.verifier_runs_setup(self.pv, inst, self.td)
        self.pv.set_srs(self.srs)
        self.pr = o.prove_scalars(self.tree, self.setup, self.pub, self.prv,
                                  lambda dl: o.transcript_challenge(co.xsk233_encode(co.k233_mulgen(dl)), self.pub))
        self.want_digests = {k: tc.digest(v) for k, v in tc.expected_vectors(self.pr, self.setup["tables"], inst.n_wires).items()}
        self.want_points = {k: tc.expected_point(dl) for k, dl in tc.expected_dlogs(self.pr, self.setup).items()}

    def fresh_prover(self, dvp):
        q = dvp.proving.Prover(self.inst)
        q.set_srs(self.srs)
        return q


@pytest.fixture(scope="module")
def toy(dvp):
    inst = dvp.gnark_r1cs.R1CSInstance.from_rows(dvp.gnark_r1cs.TOY_ROWS, dvp.gnark_r1cs.TOY_COEFFS, 2)
    rnd = random.Random(31)
    c = Circuit(dvp, inst, o.TOY_PUBLIC, o.TOY_PRIVATE, tuple(rnd.randrange(1, o.P) for _ in range(3)))
    yield c
    c.pv.close()


@pytest.fixture(scope="module")
def syn8(dvp):
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(8)
    rnd = random.Random(8)
    c = Circuit(dvp, inst, pub, prv, (rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P)))
    yield c
    c.pv.close()


@pytest.fixture(params=["toy", "syn8"])
def circuit(request):
    return request.getfixturevalue(request.param)


def check_record(dvp, c, proof, rec):
    assert (rec["log2_m"], rec["n_wires"], rec["n_public"]) == (c.pv.log_m, c.inst.n_wires, c.inst.num_public_inputs)
    assert rec["codec_rule"] == dvp.lib.dvp_codec_get_rule() and rec["parts"] == dvp.proving.TRACE_ALL
    for k, v in tc.expected_scalars(c.pr).items():
        assert rec[k] == v, k
    for k in tc.DIGEST_NAMES:
        assert rec[k] == c.want_digests[k], k
    for k in tc.POINT_NAMES:
        assert rec[k] == c.want_points[k], k
    assert rec["commit_p"]["enc"] == proof.commit_p and rec["kzg_k"]["enc"] == proof.kzg_k
    assert rec["mismatch"] == 0
    assert proof.a0_fr() == (rec["a0"], True) and proof.b0_fr() == (rec["b0"], True)


def test_record_vs_oracle_on_every_route(dvp, circuit):
    """every scalar, digest and point against the oracle, under both Horner routes and both transcript routes: one record"""
    c = circuit
    seen = []
    for hname, hmax in HORNER.items():
        for tname, host in TRANSCRIPT.items():
            with dvp.tune(DVP_HORNER_MAX_PUB=hmax, DVP_PROVE_HOST_TRANSCRIPT=host):
                assert c.pv.extend_count() == (3 if hname == "horner" else 4)
                proof, rec = c.pv.prove_trace(c.pub, c.prv)
            check_record(dvp, c, proof, rec)
            assert dvp.srs.verify(c.td, c.pub, proof)
            seen.append((proof, rec))
    assert all(x == seen[0] for x in seen)


def test_parts_select_and_the_rest_is_zero(dvp, syn8):
    c, P = syn8, dvp.proving
    c.pv.prove(c.pub, c.prv)
    full = c.pv.trace_last()
    zero_pt = {"x": 0, "y": 0, "inf": 0, "enc": bytes(30)}
    for parts in (P.TRACE_SCALARS, P.TRACE_DIGESTS, P.TRACE_POINTS, P.TRACE_SCALARS | P.TRACE_POINTS):
        rec = c.pv.trace_last(parts)
        assert rec["parts"] == parts
        for k in tc.SCALAR_NAMES:
            assert rec[k] == (full[k] if parts & P.TRACE_SCALARS else 0), (parts, k)
        for k in tc.DIGEST_NAMES:
            assert rec[k] == (full[k] if parts & P.TRACE_DIGESTS else bytes(32)), (parts, k)
        for k in tc.POINT_NAMES:
            assert rec[k] == (full[k] if parts & P.TRACE_POINTS else zero_pt), (parts, k)
        assert rec["mismatch"] == 0
    for bad in (0, 8, 0x17):
        with pytest.raises(dvp.DvpError) as ei:
            c.pv.trace_last(bad)
        assert ei.value.status == EINVAL


def test_trace_changes_nothing(dvp, circuit):
    """trace, then prove again: the same 118 bytes; trace twice: the same record; the launch census of a plain proof is what it was
    before any trace, and holds none of the trace's kernels"""
    c = circuit
    first = c.pv.prove(c.pub, c.prv)
    dvp.lib.dvp_profile_reset()
    assert c.pv.prove(c.pub, c.prv) == first
    before = mc.census(dvp, prefixes=("",))
    r1 = c.pv.trace_last()
    r2 = c.pv.trace_last()
    assert r1 == r2
    dvp.lib.dvp_profile_reset()
    assert c.pv.prove(c.pub, c.prv) == first
    after = mc.census(dvp, prefixes=("",))
    assert after == before
    assert sum(n for nm, n in before.items() if nm.startswith(("fr_digest.hip:", "blake3_tree.hip:"))) == 0
    assert c.pv.trace_last() == r1
    dvp.lib.dvp_profile_reset()
    c.pv.trace_last(dvp.proving.TRACE_DIGESTS)
    assert mc.launches(dvp, "fr_digest.hip:k_frd_pack<false>") == 16 and mc.launches(dvp, "fr_digest.hip:k_frd_pack<true>") == 0
    assert sum(n for nm, n in mc.census(dvp, prefixes=("msm.hip:", "prove.hip:", "ecfft.hip:")).items()) == 0


def _budget_for(dvp, s0, s1, want0, want1):
    """the smallest budget whose plan covers (want0, want1) bases (the planner is monotone in the budget)"""
    lo, hi = 0, sum(dvp.table_plan(s0, s1, None)[1])
    while lo < hi:
        mid = (lo + hi) // 2
        cov = dvp.table_plan(s0, s1, mid)[0]
        if cov[1] >= want1 and cov[0] >= want0:
            hi = mid
        else:
            lo = mid + 1
    return lo


def test_every_table_budget_one_record(dvp):
    """2^13 rows with the tables in use (DVP_MSM_FIXED_MIN = 1): no limit, a budget that ends inside MSM 0 (a mixed MSM) and no tables
    at all, each under both Horner and both transcript routes -- the same proof and the same record, whose partial commitments come
    from the one-shot MSM every time; a trace builds no table and releases none.  And against the oracle: every point of that record is
    (its discrete log) G by the C oracle, the logarithm summed exactly (numpy integers, no MSM) from the setup's base scalars and the
    scalar vectors -- the witness itself for msm_gm, the prover's resident q2 / k_a / k_b / k_r for the others (their digests are held
    against the oracle at 2^8): so the table path, the mixed path and the one-shot path are each right, not only equal to each other"""
    from util import np_dot_mod_fast
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(13)
    rnd = random.Random(1313)
    td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        pv = dvp.proving.Prover(inst)
        g_m, g_q, g_k = dvp.srs.srs_scalars(pv, inst, td)  # the bases are these multiples of G (verifier_runs_setup's own two steps)
        mg = dvp.curve.point_scalar_mul_gen_batch
        pv.set_srs(dvp.srs.SRS(mg(g_m), mg(g_q), tuple(mg(v) for v in g_k)))
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        inside0 = _budget_for(dvp, s0, s1, s0 * 5 // 8, s1)
        plan = dvp.table_plan(s0, s1, inside0)[0]
        assert 0 < plan[0] < s0 and plan[1] == s1
        seen = []
        for budget in (None, inside0, 0):
            pv.set_table_budget(budget)
            for hmax in HORNER.values():
                for host in TRANSCRIPT.values():
                    with dvp.tune(DVP_HORNER_MAX_PUB=hmax, DVP_PROVE_HOST_TRANSCRIPT=host):
                        proof, rec = pv.prove_trace(pub, prv)
                        held = [pv.msm_table(w)[0] for w in (0, 1)]
                        assert pv.trace_last(dvp.proving.TRACE_POINTS)["msm_gm"] == rec["msm_gm"]
                        assert [pv.msm_table(w)[0] for w in (0, 1)] == held
                    assert (held[0] > 0, held[1] > 0) == ((True, True) if budget != 0 else (False, False)), budget
                    assert rec["mismatch"] == 0 and rec["commit_p"]["enc"] == proof.commit_p and rec["kzg_k"]["enc"] == proof.kzg_k
                    seen.append((proof, rec))
        assert all(x == seen[0] for x in seen)
        assert dvp.srs.verify(td, pub, seen[0][0])
        rec = seen[0][1]
        dl = {"msm_gm": np_dot_mod_fast(dvp.fr.vec([1] + list(pub) + list(prv)), g_m), "msm_q": np_dot_mod_fast(pv.debug("q2"), g_q),
              "kzg_a": np_dot_mod_fast(pv.debug("ka"), g_k[0]), "kzg_b": np_dot_mod_fast(pv.debug("kb"), g_k[1]),
              "kzg_r": np_dot_mod_fast(pv.debug("kr"), g_k[2])}
        dl["commit_p"] = (dl["msm_gm"] + dl["msm_q"]) % o.P
        dl["kzg_k"] = (dl["kzg_a"] + dl["kzg_b"] + dl["kzg_r"]) % o.P
        for k in tc.POINT_NAMES:
            assert rec[k] == tc.expected_point(dl[k]), k
        pv.close()


def test_no_trace_without_a_complete_proof(dvp, syn8):
    """DVP_EINVAL before the first proof, after an unsatisfied witness (also when a good proof came before it), and again a record
    after the next good proof"""
    c = syn8
    q = c.fresh_prover(dvp)
    try:
        def refused():
            with pytest.raises(dvp.DvpError) as ei:
                q.trace_last()
            return ei.value.status == EINVAL

        assert refused()
        bad = list(c.prv)
        bad[0] = (bad[0] + 1) % o.P  # one flipped private wire: some row fails
        for host in TRANSCRIPT.values():
            with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=host):
                with pytest.raises(dvp.DvpError) as ei:
                    q.prove(c.pub, bad)
                assert ei.value.status == EUNSAT
                assert refused()
                good = q.prove(c.pub, c.prv)
                assert q.trace_last()["commit_p"]["enc"] == good.commit_p
                with pytest.raises(dvp.DvpError) as ei:
                    q.prove(c.pub, bad)
                assert ei.value.status == EUNSAT
                assert refused()
    finally:
        q.close()


def test_a_wrong_g_m_base_is_localised(dvp, syn8):
    """one g_m base replaced by another valid point: the verifier rejects the proof; the record shows where the provers part --
    msm_gm and commit_p differ from the honest prover's, msm_q does not, mismatch stays 0 (the table path and the one-shot path
    agree on the wrong SRS), and every vector computed before the challenge has its honest digest.  The challenge is derived from
    commit_p, so alpha and the vectors behind it (denom_invs, denom_invs2, the K scalars) differ as well: a host compares in the
    order of INTEGRATION.md and stops at msm_gm."""
    c = syn8
    c.pv.prove(c.pub, c.prv)
    honest = c.pv.trace_last()
    j = 3  # the first private wire: its value is not zero
    assert c.pr["w"][j] != 0
    (gm_xy, gm_inf), *rest = c.srs.as_list()
    gm_xy, gm_inf = np.array(gm_xy, copy=True), np.array(gm_inf, copy=True)
    assert not gm_inf[j] and not gm_inf[j + 1] and (gm_xy[j] != gm_xy[j + 1]).any()
    gm_xy[j] = gm_xy[j + 1]
    q = dvp.proving.Prover(c.inst)
    try:
        for which, (xy, inf) in enumerate([(gm_xy, gm_inf)] + rest):
            xy, inf = np.ascontiguousarray(xy, dtype=np.uint64), np.ascontiguousarray(inf, dtype=np.uint8)
            dvp.check(dvp.lib.dvp_prover_set_srs_affine(q._h, which, dvp._native.ptr(xy), dvp._native.ptr(inf), xy.shape[0]), "set_srs")
        proof, rec = q.prove_trace(c.pub, c.prv)
    finally:
        q.close()
    assert not dvp.srs.verify(c.td, c.pub, proof)
    assert rec["mismatch"] == 0
    assert rec["msm_gm"] != honest["msm_gm"] and rec["commit_p"] != honest["commit_p"] and rec["msm_q"] == honest["msm_q"]
    before_challenge = ("assignment", "evals.a", "evals.b", "evals.c", "evals.i", "evals2.a", "evals2.b", "evals2.c", "evals2.i", "r_vals2",
                        "q_vals2")
    for k in before_challenge:
        assert rec[k] == honest[k], k
    assert rec["alpha"] != honest["alpha"]
    for k in set(tc.DIGEST_NAMES) - set(before_challenge):
        assert rec[k] != honest[k], k
    # the wrong commitment is the honest one plus w_j (g_m[j+1] - g_m[j])
    g = c.setup["g_m"]
    dl = (tc.expected_dlogs(c.pr, c.setup)["msm_gm"] + c.pr["w"][j] * (g[j + 1] - g[j])) % o.P
    assert rec["msm_gm"] == tc.expected_point(dl)


CHILD = r"""
import importlib, sys
dvp = importlib.import_module("dv-pari_amd")
cache, n_public = sys.argv[1], int(sys.argv[2])
proof, _ = dvp.proving.Proof.prove_witness_file(cache, n_public)
print(proof.to_bytes().hex())
print(dvp.proving.format_prove_trace(dvp.proving.trace_cache_dir(cache, n_public)))
dvp.proving.release_cache_dir()
"""


def test_cache_dir_and_cli_traces_in_fresh_processes(dvp, tmp_path):
    """proving.trace_cache_dir and examples/dvp_prove_cli --trace, each in a fresh child process on a cache_dir written by the setup:
    the text they print parses back to the record the Python prover of the same files delivers"""
    import os
    import shutil
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "the compiled host needs g++"
    exe = tmp_path / "dvp_prove_cli"
    libdir = os.path.join(root, "dv-pari_amd")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "dvp_prove_cli.cpp"),
                           "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-pthread", "-o", str(exe)])
    A, g = dvp.artifacts, dvp.gnark_r1cs
    inst0, pub, prv = g.synthetic_sparse(10)
    cache = tmp_path / "cache"
    cache.mkdir()
    inst0.write_dump_file(cache / A.R1CS_CONSTRAINTS_FILE)
    g.write_witness_to_file(cache / A.R1CS_WITNESS_FILE, [1] + pub + prv)
    rnd = random.Random(31)
    td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
    _, pv = dvp.srs.verifier_runs_setup_cache_dir(td, cache, len(pub), write_precomputes=False)
    ref, rec = pv.prove_trace(pub, prv)
    pv.close()
    assert rec["mismatch"] == 0 and rec["commit_p"]["enc"] == ref.commit_p and dvp.srs.verify(td, pub, ref)
    runs = {"python": ([sys.executable, "-c", CHILD, str(cache), str(len(pub))], dict(os.environ)),
            "cli": ([str(exe), str(cache), str(len(pub)), "--trace"], dict(os.environ, DVP_NO_TORCH_PRELOAD="1")),
            "cli, host witness": ([str(exe), str(cache), str(len(pub)), "--trace", "--host-witness"], dict(os.environ, DVP_NO_TORCH_PRELOAD="1"))}
    for name, (cmd, env) in runs.items():
        out = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root, timeout=300)
        assert out.returncode == 0, (name, out.stderr)
        lines = out.stdout.strip().splitlines()
        assert bytes.fromhex(lines[0]) == ref.to_bytes(), name
        assert dvp.proving.parse_prove_trace("\n".join(lines[1:])) == rec, name
    # the sharded prover has no trace: the compiled host says so instead of printing one
    out = subprocess.run([str(exe), str(cache), str(len(pub)), "--trace", "--devices", "0,0"], capture_output=True, text=True,
                         env=dict(os.environ, DVP_NO_TORCH_PRELOAD="1"), timeout=300)
    assert out.returncode == 1 and "--trace" in out.stderr


def test_staged_proof_traces_only_when_whole(dvp, syn8):
    """the phased entries: begin -> MSM -> challenge -> MSM -> finish over everything leaves the record of the one-call proof; a
    challenge phase run by index slices (dvp_prove_challenge_partial / _finish) gives the same bytes but vectors that are valid only
    where the slices needed them, and an extend-free begin has no q_vals2: neither has a trace"""
    import torch

    c = syn8
    ref, honest = c.pv.prove_trace(c.pub, c.prv)
    dev = torch.device("cuda", 0)
    assignment = torch.from_numpy(dvp.fr.vec([1] + c.pub + c.prv).view(np.int64)).to(dev)
    m = c.pv.m
    for sliced in (False, True):
        q = c.fresh_prover(dvp)
        try:
            be = dvp.distributed.GpuBackend(q, dev)
            be.begin(assignment, True)
            commit = be.msm_partial(0, 0, be.msm_size(0)).clone()
            with pytest.raises(dvp.DvpError):
                q.trace_last()  # a proof in the making is none
            if sliced:
                rec = be.challenge_partial(commit, (0, m), (0, 4 * m)).clone()
                be.challenge_finish(rec.reshape(1, 16), (0, 4 * m))
            else:
                be.challenge(commit)
            assert be.finish(be.msm_partial(1, 0, be.msm_size(1)).clone()) == ref
            if sliced:
                with pytest.raises(dvp.DvpError) as ei:
                    q.trace_last()
                assert ei.value.status == EINVAL
            else:
                assert q.trace_last() == honest
                be.begin(assignment, False)  # extend-free: every begin clears the mark
                with pytest.raises(dvp.DvpError) as ei:
                    q.trace_last()
                assert ei.value.status == EINVAL
        finally:
            q.close()


def test_a_trace_goes_stale_with_what_it_reads(dvp, syn8):
    """entries outside a proof that overwrite what the trace reads take the trace away instead of leaving a silently wrong record: the
    witness check reduces its argument into the assignment's buffer, an SRS setter replaces bases the commitments were summed over,
    and another codec rule would put the proof's two encodings and the five made by the trace under different rules.  The next proof
    brings the record back."""
    c = syn8
    q = c.fresh_prover(dvp)
    try:
        def refused():
            with pytest.raises(dvp.DvpError) as ei:
                q.trace_last()
            return ei.value.status == EINVAL

        proof, rec = q.prove_trace(c.pub, c.prv)
        other = list(c.prv)
        other[0] = (other[0] + 1) % o.P
        assert q.check_witness(c.pub, other).n_unsat > 0
        assert refused()
        assert q.prove_trace(c.pub, c.prv) == (proof, rec)
        assert q.check_witness(c.pub, c.prv).ok  # the very same witness: the buffer was rewritten all the same
        assert refused()
        assert q.prove_trace(c.pub, c.prv) == (proof, rec)
        q.set_srs(c.srs)  # the same bases: the setter cannot know
        assert refused()
        assert q.prove_trace(c.pub, c.prv) == (proof, rec)
        xy, inf = c.srs.as_list()[4]
        q.set_srs_encoded(4, dvp.curve.to_bytes(xy, inf))  # one vector, through the encoded setter
        assert refused()
        assert q.prove_trace(c.pub, c.prv) == (proof, rec)
        rule = dvp.lib.dvp_codec_get_rule()
        try:
            dvp.check(dvp.lib.dvp_codec_set_rule((rule + 1) % 12), "dvp_codec_set_rule")
            assert refused()
        finally:
            dvp.check(dvp.lib.dvp_codec_set_rule(rule), "dvp_codec_set_rule")
        assert q.trace_last() == rec  # nothing was overwritten: under the proof's rule the record is there again
    finally:
        q.close()
