"""GPU tests (-m gpu) of the table budget: dvp_prover_set_table_budget / dvp_prover_msm_coverage, the mixed MSM (a fixed-base MSM over
the covered prefix, a one-shot MSM over the rest, k_join_points), and the fail-soft path of a refused table (DVP_ENOMEM).

Group elements have ONE affine representation and one encoding, so every proof made under a budget is compared byte for byte with
the default prover's and accepted by the designated verifier.  No test fills device memory: a refused table is simulated with
DVP_MSM_TABLE_REFUSE, and the one real refusal is a single request larger than the whole device, which hipMalloc turns down
without touching memory."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as o
import c_oracle as co
from util import to_limbs, from_limbs

pytestmark = pytest.mark.gpu
UNLIMITED = None


def _setup(dvp, log_m=13, seed=1313):
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(log_m)
    rnd = random.Random(seed)
    td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
    pv = dvp.proving.Prover(inst)
    srs = dvp.srs.verifier_runs_setup(pv, inst, td)
    pv.set_srs(srs)
    return inst, pub, prv, td, pv, srs


def _prof_count(dvp, name):
    ms, n = C.c_double(0), C.c_uint64(0)
    dvp.check(dvp.lib.dvp_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return int(n.value)


def _budget_for(dvp, s0, s1, want0, want1):
    """the smallest budget whose plan covers (want0, want1) bases: the bytes of that very plan"""
    lo, hi = 0, sum(dvp.table_plan(s0, s1, None)[1])
    while lo < hi:  # the planner is monotone in the budget (tests/test_table_budget_cpu.py)
        mid = (lo + hi) // 2
        c = dvp.table_plan(s0, s1, mid)[0]
        if c[1] >= want1 and c[0] >= want0:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _check_agrees(dvp, pv, budget):
    """msm_coverage, msm_table (what is held) and the planner say the same, and the tables are within the budget"""
    s0, s1 = pv.msm_size(0), pv.msm_size(1)
    cov, nbytes = dvp.table_plan(s0, s1, budget)
    full = dvp.table_plan(s0, s1, None)[0]
    held = 0
    for which in (0, 1):
        c, total, why = pv.msm_coverage(which)
        assert (c, total) == (cov[which], pv.msm_size(which)), (which, budget)
        assert why == (0 if c == full[which] else 1), (which, budget, why)
        tb, _ = pv.msm_table(which)
        assert tb == nbytes[which], (which, budget, tb, nbytes)
        if c:
            assert tb == pv.msm_plan(which)[1] * c * 64   # rows x covered x 64
        else:
            assert pv.msm_plan(which) == (0, 0)
        held += tb
    assert budget is None or held <= budget
    return cov


def test_same_bytes_at_every_boundary(dvp):
    """budget 0, the boundary inside MSM 1, exactly at the end of MSM 1, inside MSM 0, and no limit: the same 118 bytes"""
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        inst, pub, prv, td, pv, srs = _setup(dvp)
        ref = pv.prove(pub, prv)
        assert dvp.srs.verify(td, pub, ref)
        _check_agrees(dvp, pv, UNLIMITED)
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        (_, _), (fb0, fb1) = dvp.table_plan(s0, s1, None)
        cases = {
            "none": (0, (0, 0)),
            "inside MSM 1": (_budget_for(dvp, s0, s1, 0, s1 * 3 // 8), None),
            "end of MSM 1": (fb1, (0, s1)),
            "inside MSM 0": (_budget_for(dvp, s0, s1, s0 * 5 // 8, s1), None),
            "all": (fb0 + fb1, (s0, s1)),
        }
        for name, (budget, want) in cases.items():
            q = dvp.proving.Prover(inst)
            q.set_srs(srs)
            q.set_table_budget(budget)
            plan = dvp.table_plan(s0, s1, budget)[0]
            if want is not None:
                assert plan == want, name
            elif name == "inside MSM 1":
                assert plan[0] == 0 and 0 < plan[1] < s1, (name, plan)
            else:
                assert 0 < plan[0] < s0 and plan[1] == s1, (name, plan)
            # before the first proof: the plan, not zeros -- and nothing held yet
            assert tuple(q.msm_coverage(w)[0] for w in (0, 1)) == plan, name
            assert q.msm_table(0)[0] == 0 and q.msm_table(1)[0] == 0
            proof = q.prove(pub, prv)
            assert proof == ref, name
            assert dvp.srs.verify(td, pub, proof), name
            assert _check_agrees(dvp, q, budget) == plan
            assert q.prove(pub, prv) == ref, name   # tables are reused
            q.close()
        # no limit set explicitly is the default prover
        q = dvp.proving.Prover(inst)
        q.set_srs(srs)
        q.set_table_budget(UNLIMITED)
        assert q.prove(pub, prv) == ref
        _check_agrees(dvp, q, UNLIMITED)
        q.close()
        pv.close()


def test_budget_changes_between_proofs(dvp):
    """down and up on ONE prover: the bytes stay, the coverage moves, a table that no longer fits is released at once"""
    import torch
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        inst, pub, prv, td, pv, srs = _setup(dvp, seed=77)
        w = torch.from_numpy(dvp.fr.vec([1] + pub + prv).view(np.int64)).cuda()
        st = torch.cuda.current_stream().cuda_stream
        ref = pv.prove(pub, prv)
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        (_, _), (fb0, fb1) = dvp.table_plan(s0, s1, None)
        seen = []
        for budget in (UNLIMITED, fb1 + fb0 // 2, fb1 // 2, 0, fb1 // 3, fb1, fb1 + fb0 // 3, fb1 + fb0, 64 * 30 * 600, UNLIMITED):
            pv.set_table_budget(budget)
            # released at once: what is still held fits the new budget before any proof runs
            assert budget is None or pv.msm_table(0)[0] + pv.msm_table(1)[0] <= budget, budget
            assert pv.prove(pub, prv) == ref, budget
            assert pv.prove_dev(w.data_ptr(), st) == ref, budget
            with dvp.tune(DVP_PROVE_HOST_TRANSCRIPT=1):
                assert pv.prove_dev(w.data_ptr(), st) == ref, budget
            seen.append(_check_agrees(dvp, pv, budget))
        assert len(set(seen)) >= 7, seen   # the coverage did move
        assert seen[0] == seen[-1] == (s0, s1) and seen[3] == (0, 0)
        assert dvp.srs.verify(td, pub, ref)
        pv.close()


def test_budget_from_the_environment_knob(dvp):
    """new provers start from DVP_TABLE_BUDGET_BYTES (here through the run-time flavour of the knob)"""
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        inst, pub, prv, td, pv, srs = _setup(dvp, seed=5)
        ref = pv.prove(pub, prv)
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        fb1 = dvp.table_plan(s0, s1, None)[1][1]
        with dvp.tune(DVP_TABLE_BUDGET_BYTES=fb1 // 2):
            q = dvp.proving.Prover(inst)
        q.set_srs(srs)
        assert q.prove(pub, prv) == ref
        cov = _check_agrees(dvp, q, fb1 // 2)
        assert cov[0] == 0 and 0 < cov[1] < s1
        q.close()
        pv.close()


def _free_wire_prover(dvp, n_wires, rnd):
    """a circuit whose eight rows read wire 0 only (1 * 1 = 1): every other wire is free, so dvp_prover_msm_partial(0, ..) sums
    CHOSEN scalars; the bases are k_i G with known k_i, so the oracle's answer is one generator multiplication"""
    rows = [([(0, 0)], [(0, 0)], [(0, 0)])] * 8
    inst = dvp.gnark_r1cs.R1CSInstance.from_rows(rows, [1], 2, n_wires=n_wires)
    pv = dvp.proving.Prover(inst)
    m = pv.m
    ks = [rnd.randrange(1, o.P) for _ in range(n_wires + 5 * m)]
    mg = dvp.curve.point_scalar_mul_gen_batch
    cut = [0, n_wires, n_wires + m, n_wires + 2 * m, n_wires + 3 * m, n_wires + 5 * m]
    vecs = [mg(to_limbs(ks[cut[i]:cut[i + 1]])) for i in range(5)]
    pv.set_srs(dvp.srs.SRS(vecs[0], vecs[1], (vecs[2], vecs[3], vecs[4])))
    return pv, ks


def _partial(dvp, pv, scalars, lo, hi, raw=None):
    """dvp_prover_msm_partial(0, lo, hi) over the assignment `scalars` -> affine point as ints, or None for the neutral element"""
    import torch
    arr = dvp.fr.vec(scalars)
    if raw:
        for idx, v in raw.items():  # values >= p, limbs as given
            arr[idx] = np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8")
    w = torch.from_numpy(arr.view(np.int64)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    pv.begin(w.data_ptr(), st, need_extend=False)
    out = torch.zeros(10, dtype=torch.int64, device="cuda")
    pv.msm_partial(0, lo, hi, out.data_ptr(), out.data_ptr() + 64, st)
    torch.cuda.synchronize()
    h = out.cpu().numpy().view(np.uint64)
    return None if (int(h[8]) & 0xFFFFFFFF) else tuple(from_limbs(h[:8].reshape(2, 4)))


def test_mixed_join_edge_cases_vs_oracle(dvp):
    """the join of the two halves is a COMPLETE addition: neutral prefix (every covered scalar zero), prefix == suffix (doubling),
    prefix == -suffix (neutral sum), neutral suffix, both neutral -- each against the CPU oracle; and a scalar >= p in the suffix
    is reported with its index in the whole vector"""
    rnd = random.Random(4242)
    n_wires = 4096
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        pv, ks = _free_wire_prover(dvp, n_wires, rnd)
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        budget = _budget_for(dvp, s0, s1, 2000, s1)
        pv.set_table_budget(budget)
        B = pv.msm_coverage(0)[0]   # the boundary: [0, B) from the table, [B, ..) one-shot
        assert 2000 <= B < n_wires - 8 and pv.msm_coverage(1)[0] == s1

        def expect(scalars, lo, hi):
            return co.k233_mulgen(sum(scalars[i] * ks[i] for i in range(lo, hi)) % o.P)

        base = [1] + [rnd.randrange(o.P) for _ in range(n_wires - 1)]
        # a plain mixed range first (and the table now exists: [0, B))
        assert _partial(dvp, pv, base, 0, n_wires) == expect(base, 0, n_wires)
        assert pv.msm_table(0)[0] == pv.msm_plan(0)[1] * B * 64 <= budget
        # prefix neutral: all covered scalars of the range are zero
        s = list(base)
        for i in range(B - 3, B):
            s[i] = 0
        assert _partial(dvp, pv, s, B - 3, B + 2) == expect(s, B - 3, B + 2) != None  # noqa: E711
        # suffix neutral
        s = list(base)
        s[B] = s[B + 1] = 0
        assert _partial(dvp, pv, s, B - 2, B + 2) == expect(s, B - 2, B + 2) != None  # noqa: E711
        # both neutral
        s = list(base)
        s[B - 1] = s[B] = 0
        assert _partial(dvp, pv, s, B - 1, B + 1) is None
        # two bases, prefix sum == suffix sum: s[B-1] k[B-1] == s[B] k[B]
        s = list(base)
        s[B - 1], s[B] = ks[B], ks[B - 1]
        got = _partial(dvp, pv, s, B - 1, B + 1)
        assert got == co.k233_mulgen(2 * ks[B] * ks[B - 1] % o.P) == expect(s, B - 1, B + 1)
        # two bases, opposite sums
        s[B] = o.P - ks[B - 1]
        assert expect(s, B - 1, B + 1) is None
        assert _partial(dvp, pv, s, B - 1, B + 1) is None
        # a scalar >= p in the suffix: DVP_EINVAL with the index in the whole vector; the same in the prefix
        for j in (B + 5, B, B - 1, 3):
            with pytest.raises(dvp.DvpError) as e:
                _partial(dvp, pv, base, 0, n_wires, raw={j: base[j] + o.P})
            assert (e.value.status, e.value.index) == (-1, j), j
        # the first bad index wins, wherever the two lie
        with pytest.raises(dvp.DvpError) as e:
            _partial(dvp, pv, base, 0, n_wires, raw={B + 9: base[B + 9] + o.P, B + 700: base[B + 700] + o.P})
        assert (e.value.status, e.value.index) == (-1, B + 9)
        with pytest.raises(dvp.DvpError) as e:
            _partial(dvp, pv, base, 0, n_wires, raw={B - 9: base[B - 9] + o.P, B + 1: base[B + 1] + o.P})
        assert (e.value.status, e.value.index) == (-1, B - 9)
        # and the prover still sums correctly afterwards
        assert _partial(dvp, pv, base, 0, n_wires) == expect(base, 0, n_wires)
        pv.close()


@pytest.mark.parametrize("log_m,knobs", [(13, {"DVP_MSM_AFF_MIN": 256}), (17, {})])
def test_mixed_prover_waits_as_often_as_the_default(dvp, log_m, knobs):
    """host_waits_stream per proof (synchronisations of the proof's own stream) of a mixed prover == that of a default prover,
    both measured here.  An MSM too small for a first pair round waits for its largest-bucket read ON the stream, mid-way
    (tests/test_gpu_prove.py: test_host_and_device_transcript_same_bytes_and_waits), and a mixed MSM is two MSMs; so the 2^13
    case lowers DVP_MSM_AFF_MIN until every half runs pair rounds -- as the default prover's MSMs do at the sizes this path is
    for -- and the 2^17 case runs with no knob at all."""
    import torch
    with dvp.tune(DVP_MSM_FIXED_MIN=1, **knobs):
        inst, pub, prv, td, pv, srs = _setup(dvp, log_m=log_m, seed=log_m)
        w = torch.from_numpy(dvp.fr.vec([1] + pub + prv).view(np.int64)).cuda()
        st = torch.cuda.current_stream().cuda_stream
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        (_, _), (fb0, fb1) = dvp.table_plan(s0, s1, None)
        counts = {}
        ref = None
        for name, budget in (("default", UNLIMITED), ("inside MSM 1", fb1 // 2), ("inside MSM 0", fb1 + fb0 // 2), ("default again", UNLIMITED)):
            pv.set_table_budget(budget)
            for _ in range(2):
                proof = pv.prove_dev(w.data_ptr(), st)   # tables, workspaces
            dvp.lib.dvp_profile_reset()
            assert pv.prove_dev(w.data_ptr(), st) == proof
            counts[name] = _prof_count(dvp, "host_waits_stream")
            print(name, "host_waits_stream", counts[name], "host_waits_side", _prof_count(dvp, "host_waits_side"))
            ref = ref or proof
            assert proof == ref, name
        assert dvp.srs.verify(td, pub, ref)
        cov1 = dvp.table_plan(s0, s1, fb1 // 2)[0]
        assert 0 < cov1[1] < s1
        assert counts["inside MSM 1"] == counts["default"], counts
        assert counts["inside MSM 0"] == counts["default"], counts
        assert counts["default again"] == counts["default"], counts
        pv.close()


def test_refused_table_fails_soft(dvp):
    """DVP_MSM_TABLE_REFUSE = 1: msm_fixed_build behaves as if hipMalloc had said hipErrorOutOfMemory.  The proof succeeds with the
    same bytes through the one-shot path, the coverage says why (reason 2), a second proof does not ask again, a new budget does;
    dvp_msm_ctx_create -- where the context IS the table -- returns DVP_ENOMEM"""
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        inst, pub, prv, td, pv, srs = _setup(dvp, seed=909)
        ref = pv.prove(pub, prv)
        s0, s1 = pv.msm_size(0), pv.msm_size(1)
        fb1 = dvp.table_plan(s0, s1, None)[1][1]
        for budget in (UNLIMITED, fb1 // 2):
            q = dvp.proving.Prover(inst)
            q.set_srs(srs)
            q.set_table_budget(budget)
            with dvp.tune(DVP_MSM_TABLE_REFUSE=1):
                assert q.prove(pub, prv) == ref
                planned = dvp.table_plan(s0, s1, budget)[0]
                for which in (0, 1):
                    want = (0, pv.msm_size(which), 2) if planned[which] else (0, pv.msm_size(which), 1)
                    assert q.msm_coverage(which) == want, (budget, which)
                    assert q.msm_table(which)[0] == 0
            # the knob is off again, but the refusal is remembered: no retry at every proof
            assert q.prove(pub, prv) == ref
            assert q.msm_table(0)[0] == 0 and q.msm_table(1)[0] == 0
            assert q.msm_coverage(1)[2] == 2
            # a new budget is the occasion to ask again
            q.set_table_budget(budget)
            assert q.prove(pub, prv) == ref
            _check_agrees(dvp, q, budget)
            q.close()
        assert dvp.srs.verify(td, pub, ref)
        # the public fixed-base context has nothing to fall back to
        n = 600
        rnd = random.Random(3)
        k = to_limbs([rnd.randrange(o.P) for _ in range(n)])
        bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        h = C.c_void_p()
        with dvp.tune(DVP_MSM_TABLE_REFUSE=1):
            assert dvp.lib.dvp_msm_ctx_create(dvp._native.ptr(bases), None, n, 0, C.byref(h)) == -7
        assert not h.value
        assert dvp.lib.dvp_msm_ctx_create(dvp._native.ptr(bases), None, n, 0, C.byref(h)) == 0
        dvp.lib.dvp_msm_ctx_destroy(h)
        # and the device is fine: the refusal left no sticky error behind
        assert pv.prove(pub, prv) == ref
        pv.close()


def test_shards_share_the_device_budget(dvp):
    """dvp_set_devices([0, 0]) with a budget that fits ONE shard's tables but not both: the device's budget is split evenly among
    the shards that name it, a shard that does not fit runs one-shot; same bytes, tables within the budget"""
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        inst, pub, prv, td, pv, srs = _setup(dvp, seed=2020)
        ref = pv.prove(pub, prv)
        try:
            dvp.set_devices([0, 0])
            assert pv.prove(pub, prv) == ref
            per_shard = [pv.msm_table(w)[0] // 2 for w in (0, 1)]   # two equal shards with a table each
            assert all(per_shard)
            one = sum(per_shard)
            for budget in (one, one + one // 2, 2 * one - 64, per_shard[1], 0):
                pv.set_table_budget(budget)
                assert pv.prove(pub, prv) == ref, budget
                held = pv.msm_table(0)[0] + pv.msm_table(1)[0]
                assert held <= budget, (budget, held)
                assert held < 2 * one
                assert pv.prove(pub, prv) == ref, budget
            pv.set_table_budget(2 * one)
            assert pv.prove(pub, prv) == ref
            assert pv.msm_table(0)[0] + pv.msm_table(1)[0] == 2 * one
            assert [pv.msm_coverage(w)[2] for w in (0, 1)] == [0, 0]
            # a refused shard table: one-shot, reason 2, same bytes
            pv.set_table_budget(UNLIMITED)
            with dvp.tune(DVP_MSM_TABLE_REFUSE=1):
                assert pv.prove(pub, prv) == ref
            assert pv.msm_coverage(1) == (0, pv.msm_size(1), 2) and pv.msm_table(1)[0] == 0
        finally:
            dvp.set_devices([])
        pv.set_table_budget(UNLIMITED)
        assert pv.prove(pub, prv) == ref
        assert dvp.srs.verify(td, pub, ref)
        pv.close()


def test_one_real_refusal_is_enomem(dvp):
    """ONE request for twice the device's total memory: hipMalloc itself turns it down (nothing is launched, no memory is touched),
    the status is DVP_ENOMEM and not DVP_EHIP, and the next proof in this process succeeds"""
    import torch
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        inst, pub, prv, td, pv, srs = _setup(dvp, seed=31)
        ref = pv.prove(pub, prv)
        _, total = torch.cuda.mem_get_info()
        rate = C.c_double(0)
        rc = dvp.lib.dvp_ubench_gather(None, 2 * total, 1, C.byref(rate))
        assert rc == -7, rc
        assert b"memory" in dvp.lib.dvp_strerror(rc)
        assert pv.prove(pub, prv) == ref
        assert dvp.srs.verify(td, pub, ref)
        pv.close()
