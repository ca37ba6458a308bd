"""GPU tests (-m gpu) of dvp_simulate_batch / _dev (csrc/simulate.hip: k_simulate, srs.simulate_batch): the bytes, status and discrete
logs equal the plain-Python restatement (tests/simulate_cases.py) at every lane position and public-input count, every proof is
accepted by the per-lane verifier, the combined check and the oracle, under another binding and codec rule as well; the stream is
deterministic and splits by index_base; special inputs and input faults behave as include/dvpari.h states; one call is one launch."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as o
import simulate_cases as sc
import verify_cases as vc
from msm_cases import census, launches

pytestmark = pytest.mark.gpu
TD = (0x3D9F1A77 * 104729 % o.P, 0xC0FFEE1234567 % o.P, 0xDEADBEEF987654321 % o.P)
SEED = bytes(range(7, 39))
EDGE_LANES = (0, 63, 64, 255, 256)  # first and last lane of a wave, of a workgroup, and the first of the next workgroup


def gpu_encode_many(dvp):
    def enc(dlogs):
        out = dvp.curve.point_scalar_mul_gen_batch_bytes(dvp.fr.vec(dlogs)) if dlogs else np.zeros((0, 30), dtype=np.uint8)
        return [out[i].tobytes() for i in range(len(dlogs))]
    return enc


def restate(dvp, td, pubs, binding=(None, None), **kw):
    ch = lambda e, pub: dvp.proving.transcript_challenge(e, pub, *binding)  # noqa: E731
    return sc.simulate(td, pubs, encode_many=gpu_encode_many(dvp), challenge=ch, **kw)


def rand_pubs(rng, n, n_public):
    return [[rng.randrange(o.P) for _ in range(n_public)] for _ in range(n)]


def assert_equals_restatement(dvp, got, want):
    proofs, status, dlogs = got
    assert proofs.shape == (len(want), 118) and status.shape == (len(want),) and dlogs.shape == (len(want), 2, 4)
    for j, w in enumerate(want):
        assert status[j] == w["status"], (j, w["case"], int(status[j]))
        assert proofs[j].tobytes() == w["proof"], (j, w["case"])
        assert dvp.fr.to_ints(dlogs[j]) == [w["p"], w["k"]], (j, w["case"])


def assert_accepted(dvp, td, pubs, proofs, status):
    S = dvp.srs
    assert not status.any()
    v = S.verify_batch(S.Trapdoor(*td), pubs, proofs)
    assert not v.any(), np.nonzero(v)[0][:10]
    v, report = S.verify_batch_rlc(S.Trapdoor(*td), pubs, proofs)
    assert not v.any() and report == S.VERIFY_RLC_COMBINED


@pytest.mark.parametrize("n_public", [0, 2, 36])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_bytes_equal_the_restatement_and_are_accepted(dvp, n, n_public):
    """the cases rotate over the lanes; at 257 proofs every case also sits at lanes 0, 63, 64, 255 and 256 (one call per case)"""
    rng = random.Random(1000 * n + n_public)
    S = dvp.srs
    for r in (range(7) if n == 257 else [n % 7]):
        cases = [(j + r) % 7 for j in range(n)]
        for lane in EDGE_LANES:
            if lane < n:
                cases[lane] = r
        pubs = rand_pubs(rng, n, n_public)
        got = S.simulate_batch(S.Trapdoor(*TD), pubs, seed=SEED, index_base=r << 40, cases=cases, return_dlogs=True)
        assert_equals_restatement(dvp, got, restate(dvp, TD, pubs, seed=SEED, index_base=r << 40, cases=cases))
        assert_accepted(dvp, TD, pubs, got[0], got[1])


def test_a_sample_passes_the_oracle(dvp):
    rng = random.Random(6)
    S = dvp.srs
    cases = [sc.GENERIC, sc.T_HALF, sc.P_ZERO, sc.K_PLUS_G, sc.K_MINUS_G, sc.K_ZERO]
    pubs = rand_pubs(rng, 6, 3)
    proofs, status = S.simulate_batch(S.Trapdoor(*TD), pubs, cases=cases)
    assert not status.any()
    for j in range(6):
        assert vc.oracle_verdict(TD, pubs[j], proofs[j].tobytes()), cases[j]


def test_other_binding_and_codec_rule(dvp):
    """the simulator follows dvp_verify_set_binding and dvp_codec_set_rule as the verifier does; a batch made under one binding is
    rejected with VERIFY_EQUATION under another"""
    S = dvp.srs
    td = S.Trapdoor(*TD)
    rng = random.Random(12)
    n = 65
    pubs = rand_pubs(rng, n, 2)
    cases = [j % 7 for j in range(n)]
    binding = (o.blake3(b"an srs"), o.blake3(b"a circuit"))
    S.set_verify_binding(*binding)
    try:
        bound = S.simulate_batch(td, pubs, seed=SEED, cases=cases, return_dlogs=True)
        assert_equals_restatement(dvp, bound, restate(dvp, TD, pubs, binding=binding, seed=SEED, cases=cases))
        assert_accepted(dvp, TD, pubs, bound[0], bound[1])
    finally:
        S.set_verify_binding(None, None)
    assert (S.verify_batch(td, pubs, bound[0]) == S.VERIFY_EQUATION).all()
    plain = S.simulate_batch(td, pubs, seed=SEED, cases=cases)
    S.set_verify_binding(*binding)
    try:
        assert (S.verify_batch(td, pubs, plain[0]) == S.VERIFY_EQUATION).all()
    finally:
        S.set_verify_binding(None, None)
    assert_accepted(dvp, TD, pubs, plain[0], plain[1])
    rule = 1
    dvp.check(dvp.lib.dvp_codec_set_rule(rule))
    try:
        got = S.simulate_batch(td, pubs[:20], seed=SEED, cases=cases[:20], return_dlogs=True)
        want = sc.simulate(TD, pubs[:20], seed=SEED, cases=cases[:20], encode_many=lambda dl: vc.oracle_encode_many(dl, rule=rule),
                           challenge=dvp.proving.transcript_challenge)
        assert_equals_restatement(dvp, got, want)
        assert_accepted(dvp, TD, pubs[:20], got[0], got[1])
    finally:
        dvp.check(dvp.lib.dvp_codec_set_rule(0))


def test_deterministic_per_trapdoor_and_split_by_index_base(dvp):
    S = dvp.srs
    rng = random.Random(3)
    n = 130
    pubs = rand_pubs(rng, n, 1)
    cases = [j % 7 for j in range(n)]
    td = S.Trapdoor(*TD)
    a = S.simulate_batch(td, pubs, cases=cases, return_dlogs=True)  # seed=None: the key comes from the trapdoor
    b = S.simulate_batch(td, pubs, cases=cases, return_dlogs=True)
    assert all((x == y).all() for x, y in zip(a, b))
    assert_equals_restatement(dvp, (a[0][:9], a[1][:9], a[2][:9]), restate(dvp, TD, pubs[:9], cases=cases[:9]))
    other = S.simulate_batch(S.Trapdoor(TD[0], TD[1], TD[2] + 1), pubs, cases=cases, return_dlogs=True)
    assert not other[1].any() and (other[0][:, 89:] != a[0][:, 89:]).any(axis=1).all()  # every drawn b0 differs
    h = n // 2
    lo = S.simulate_batch(td, pubs[:h], cases=cases[:h], index_base=0, return_dlogs=True)
    hi = S.simulate_batch(td, pubs[h:], cases=cases[h:], index_base=h, return_dlogs=True)
    for whole, x, y in zip(a, lo, hi):
        assert (np.concatenate([x, y]) == whole).all()


def test_b0_override_bump_and_v0_zero(dvp):
    """each in a call of one proof"""
    S = dvp.srs
    td = S.Trapdoor(*TD)
    pub = [[5, 6, 7]]
    proofs, status = S.simulate_batch(td, pub, seed=SEED, b0=[0xB0B0])
    assert status[0] == 0 and int.from_bytes(proofs[0, 89:].tobytes(), "little") == 0xB0B0
    assert_accepted(dvp, TD, pub, proofs, status)
    pole = (-vc.inv(TD[1] * TD[1])) % o.P  # 1 + delta^2 b0 = 0
    got = S.simulate_batch(td, pub, seed=SEED, b0=[pole], return_dlogs=True)
    assert int.from_bytes(got[0][0, 89:].tobytes(), "little") == (pole + 1) % o.P
    assert_equals_restatement(dvp, got, restate(dvp, TD, pub, seed=SEED, b0=[pole]))
    assert_accepted(dvp, TD, pub, got[0], got[1])
    # v0 = 0: tau = the alpha of this very proof (alpha depends on p, the public inputs and the binding, not on tau)
    alpha = dvp.fr.to_int(S.verify_trace(td, pub, proofs)["alpha"][0])
    assert alpha == dvp.proving.transcript_challenge(proofs[0, :30].tobytes(), pub[0])
    z = S.simulate_batch(S.Trapdoor(alpha, TD[1], TD[2]), pub, seed=SEED, b0=[0xB0B0], return_dlogs=True)
    assert z[1][0] == S.SIM_V0_ZERO and not z[0].any() and not z[2].any()


def test_host_flavour_input_faults(dvp, nat):
    S = dvp.srs
    td = S.Trapdoor(*TD)
    pubs = [[1, 2], [3, 4], [5, 6]]

    def fails(index=None, **kw):
        args = dict(td=td, public_inputs=pubs)
        args.update(kw)
        with pytest.raises(nat.DvpError) as e:
            S.simulate_batch(args.pop("td"), args.pop("public_inputs"), **args)
        assert e.value.name == "DVP_EINVAL"
        if index is not None:
            assert e.value.index == index

    fails(index=3, public_inputs=[[1, 2], [3, o.P], [5, 6]])  # the flat index
    fails(index=1, cases=[0, 7, 0])
    fails(index=2, b0=[1, 2, o.P])
    fails(td=S.Trapdoor(TD[0], TD[1], 0))  # epsilon = 0
    for k in range(3):
        bad = list(TD)
        bad[k] = o.P
        fails(td=S.Trapdoor(*bad))
    fails(public_inputs=[[0] * 8193])  # n_public > DVP_VERIFY_MAX_PUBLIC
    t, d, e = (S._raw_limbs(x) for x in TD)
    st = np.zeros(3, dtype=np.uint8)
    pa = np.zeros((3, 118), dtype=np.uint8)
    pub = S._public_array(pubs, 3)
    p = nat.ptr
    assert dvp.lib.dvp_simulate_batch(p(t), p(d), p(e), p(pub), 2, 3, None, 0, None, None, None, p(st), None) == -1  # no proofs
    assert dvp.lib.dvp_simulate_batch(p(t), p(d), p(e), p(pub), 2, 3, None, 0, None, None, p(pa), None, None) == -1  # no status
    assert dvp.lib.dvp_simulate_batch(p(t), p(d), p(e), None, 2, 3, None, 0, None, None, p(pa), p(st), None) == -1   # no public inputs
    assert dvp.lib.dvp_simulate_batch(p(t), p(d), p(e), None, 2, 0, None, 0, None, None, None, None, None) == 0      # n = 0
    proofs, status = S.simulate_batch(td, [])
    assert proofs.shape == (0, 118) and status.shape == (0,)


def test_dev_flavour_on_a_stream(dvp):
    """dvp_simulate_batch_dev on torch tensors and a non-default stream: the host flavour's bytes; each of the three input faults is a
    status bit of its own proof, which is zero bytes, and the neighbours are untouched"""
    import torch

    S = dvp.srs
    rng = random.Random(21)
    n, n_public = 300, 2
    pubs = rand_pubs(rng, n, n_public)
    cases = np.array([j % 7 for j in range(n)], dtype=np.uint8)
    b0 = dvp.fr.vec([rng.randrange(o.P) for _ in range(n)])
    host = S.simulate_batch(S.Trapdoor(*TD), pubs, seed=SEED, index_base=11, cases=cases, b0=b0, return_dlogs=True)
    pub = S._public_array(pubs, n)
    faults = {7: S.SIM_BAD_PUBLIC, 64: S.SIM_BAD_CASE, 255: S.SIM_BAD_B0, 256: S.SIM_BAD_PUBLIC | S.SIM_BAD_CASE | S.SIM_BAD_B0}
    over = np.frombuffer(o.P.to_bytes(32, "little"), dtype="<u8")
    for j, bits in faults.items():
        if bits & S.SIM_BAD_PUBLIC:
            pub[j, 1] = over
        if bits & S.SIM_BAD_CASE:
            cases[j] = 7
        if bits & S.SIM_BAD_B0:
            b0[j] = over
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    tpub, tcases, tb0 = up(pub), up(cases), up(b0)
    tp = torch.full((n, 118), 0xEE, dtype=torch.uint8, device=dev)
    ts = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    tl = torch.full((n, 64), 0xEE, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    keep, (t, d, e) = S._trapdoor_args(S.Trapdoor(*TD))
    sd = np.frombuffer(SEED, dtype=np.uint8).copy()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with torch.cuda.stream(s):
        rc = dvp.lib.dvp_simulate_batch_dev(t, d, e, vp(tpub), n_public, n, dvp._native.ptr(sd), 11, vp(tcases), vp(tb0), vp(tp), vp(ts), vp(tl),
                                            C.c_void_p(s.cuda_stream))
    assert rc == 0
    s.synchronize()
    gp, gs, gl = tp.cpu().numpy(), ts.cpu().numpy(), tl.cpu().numpy().view("<u8").reshape(n, 2, 4)
    ep, es, el = (x.copy() for x in host)
    for j, bits in faults.items():
        ep[j], es[j], el[j] = 0, bits, 0
    assert (gs == es).all(), np.nonzero(gs != es)[0][:10]
    assert (gp == ep).all(), np.nonzero((gp != ep).any(axis=1))[0][:10]
    assert (gl == el).all()


def test_one_call_is_one_launch(dvp):
    S = dvp.srs
    td = S.Trapdoor(*TD)
    pubs = [[j] for j in range(300)]
    S.simulate_batch(td, pubs[:1])  # the generator table and the squaring tables exist after this
    dvp.lib.dvp_profile_reset()
    proofs, status = S.simulate_batch(td, pubs)
    assert launches(dvp, "simulate.hip:k_simulate") == 1
    assert not any(census(dvp, prefixes=("msm.hip:", "codec.hip:", "verify.hip:")).values())
    assert not status.any()
