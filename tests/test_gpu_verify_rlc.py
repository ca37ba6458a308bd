"""GPU tests (-m gpu) of batch verification by one random linear combination (csrc/verify.hip: dvp_verify_batch_rlc,
dvp_verify_batch_rlc_dev, srs.verify_batch_rlc): valid batches are accepted through the combined MSM check alone (report
COMBINED), batches with a bad proof get dvp_verify_batch's verdicts index for index, the coefficient rule is pinned byte for byte,
and the device flavour is right on a stream and from two host threads at once.  Proofs are built without a prover
(tests/verify_cases.py)."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import pyref as o
import verify_cases as vc

pytestmark = pytest.mark.gpu
TD = (0x3D9F1A77 * 104729 % o.P, 0xC0FFEE1234567 % o.P, 0xDEADBEEF987654321 % o.P)
EXC = [c for c in vc.CASES if c != "v0_zero"]  # v0 = 0 needs a trapdoor of its own per proof
MALFORMED = ("a0_ge_p", "b0_ge_p", "bad_commit", "bad_kzg", "spare_commit", "spare_kzg")


def gpu_encode_many(dvp):
    def enc(dlogs):
        s = np.zeros((len(dlogs), 4), dtype=np.uint64)
        if dlogs:
            s[:] = np.frombuffer(b"".join(int(k % o.P).to_bytes(32, "little") for k in dlogs), dtype="<u8").reshape(-1, 4)
        out = np.zeros((len(dlogs), 30), dtype=np.uint8)
        dvp.check(dvp.lib.dvp_mulgen_batch(dvp._native.ptr(s), len(dlogs), dvp._native.ptr(out)), "dvp_mulgen_batch")
        return [out[i].tobytes() for i in range(len(dlogs))]
    return enc


def bulk(dvp, pubs, cases, seed, td=TD):
    return vc.build(td, pubs, cases, seed=seed, encode_many=gpu_encode_many(dvp), challenge=dvp.proving.transcript_challenge)


def rows_of(built):
    return [c["proof"] for c in built], [c["pub"] for c in built]


def expected_report(S, v):
    """what the combined check must report for per-lane verdicts v (exact up to the 2^-127 bound)"""
    if (v == S.VERIFY_EQUATION).any():
        return S.VERIFY_RLC_FALLBACK
    return S.VERIFY_RLC_COMBINED if (v == 0).any() else 0


def tampered_batch(dvp, built, kinds, rng, per_kind=3):
    """the valid batch with each kind of vc.TAMPER at `per_kind` random indices -> (proofs, pubs, {index: kind})"""
    proofs, pubs = rows_of(built)
    pos = rng.sample(range(len(built)), per_kind * len(kinds))
    where = {}
    for k, i in enumerate(pos):
        kind = kinds[k // per_kind]
        b, td, pub = vc.tamper(built[i], kind, rng)
        if kind == "wrong_trapdoor":  # one trapdoor per batch: break the equation the same way through a0
            b = built[i]["proof"][:60] + ((built[i]["a0"] + 7) % o.P).to_bytes(29, "little") + b[89:]
        proofs[i], pubs[i] = b, pub
        where[i] = kind
    return proofs, pubs, where


@pytest.mark.parametrize("n_public", [0, 2, 36])
def test_valid_batches_report_combined(dvp, n_public):
    """n = 1, 2, 37, 1500 valid proofs, the exceptional shapes first: all verdicts 0 through the combined check alone -- a
    fallback to the per-lane check fails the test"""
    S = dvp.srs
    rng = random.Random(500 + n_public)
    cases = EXC + [None] * (1500 - len(EXC))
    pubs = [[rng.randrange(o.P) for _ in range(n_public)] for _ in cases]
    built = bulk(dvp, pubs, cases, seed=600 + n_public)
    proofs, pubs = rows_of(built)
    for n in (1, 2, 37, 1500):
        v, rep = S.verify_batch_rlc(S.Trapdoor(*TD), pubs[:n], proofs[:n])
        assert not v.any(), (n, np.nonzero(v)[0][:10])
        assert rep == S.VERIFY_RLC_COMBINED, (n, rep)


def test_repeated_and_exceptional_bases(dvp):
    """one proof 1000 times (the MSM sees K and P 1000 times over), K = +-G, K = O, P = O: all accepted through COMBINED"""
    S, td = dvp.srs, dvp.srs.Trapdoor(*TD)
    rng = random.Random(11)
    one = bulk(dvp, [[rng.randrange(o.P), rng.randrange(o.P)]], [None], seed=12)[0]
    v, rep = S.verify_batch_rlc(td, [one["pub"]] * 1000, [one["proof"]] * 1000)
    assert not v.any() and rep == S.VERIFY_RLC_COMBINED, rep
    for cases in (["k_plus_g", "k_minus_g"] * 20, ["k_zero"] * 30, ["p_zero"] * 30, ["k_zero", "p_zero", None] * 10):
        pubs = [[rng.randrange(o.P)] for _ in cases]
        built = bulk(dvp, pubs, cases, seed=13 + len(cases))
        proofs, pubs = rows_of(built)
        v, rep = S.verify_batch_rlc(td, pubs, proofs)
        assert not v.any(), (cases[0], np.nonzero(v)[0])
        assert rep == S.VERIFY_RLC_COMBINED, (cases[0], rep)


def test_tampered_proofs_match_verify_batch(dvp):
    """every vc.TAMPER kind at random indices of a 257-proof batch (one kind per batch, then all together): verdicts equal
    dvp_verify_batch's index for index; FALLBACK exactly when a well-formed proof fails its equation, else COMBINED with the
    malformed proofs carrying their flag bits"""
    S, td = dvp.srs, dvp.srs.Trapdoor(*TD)
    rng = random.Random(2025)
    n = 257
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in range(n)]
    built = bulk(dvp, pubs, [None] * n, seed=88)
    for kinds in [(k,) for k in vc.TAMPER] + [vc.TAMPER]:
        proofs, pubs_t, where = tampered_batch(dvp, built, list(kinds), rng)
        ref = S.verify_batch(td, pubs_t, proofs)
        v, rep = S.verify_batch_rlc(td, pubs_t, proofs)
        assert (v == ref).all(), (kinds, np.nonzero(v != ref)[0][:10])
        assert rep == expected_report(S, ref), (kinds, rep, ref[list(where)])
        assert all(ref[i] for i in where), kinds  # every tampering is rejected by the per-lane check
        if all(k in MALFORMED for k in kinds):
            assert rep == S.VERIFY_RLC_COMBINED, kinds
            assert all(ref[i] and not ref[i] & S.VERIFY_EQUATION for i in where), kinds
        untouched = np.ones(n, dtype=bool)
        untouched[list(where)] = False
        assert not v[untouched].any(), kinds


def test_cancelling_pair_is_rejected(dvp):
    """two proofs with errors e G and -e G (a0 shifted in opposite directions, du0/da0 = eps (1 + delta^2 b0)): a plain sum of the
    equations cancels, the random linear combination does not -- both are EQUATION"""
    S, td = dvp.srs, dvp.srs.Trapdoor(*TD)
    tau, delta, eps = TD
    rng = random.Random(21)
    pubs = [[rng.randrange(o.P)] for _ in range(6)]
    built = bulk(dvp, pubs, [None] * 6, seed=22)
    proofs, pubs = rows_of(built)
    e = 0x1234567890ABCDEF
    for i, sign in ((1, 1), (4, -1)):
        c = built[i]
        da = sign * e * vc.inv(eps * (1 + delta * delta * c["b0"])) % o.P
        proofs[i] = c["proof"][:60] + ((c["a0"] + da) % o.P).to_bytes(29, "little") + c["proof"][89:]
    # the two errors cancel in a plain sum: u0 moves by +e and -e with the same transcript
    ref = S.verify_batch(td, pubs, proofs)
    assert list(ref) == [0, S.VERIFY_EQUATION, 0, 0, S.VERIFY_EQUATION, 0], ref
    v, rep = S.verify_batch_rlc(td, pubs, proofs)
    assert (v == ref).all(), v
    assert rep == S.VERIFY_RLC_FALLBACK


def coeff(seed, j, proof, pub):
    """r_j of the header, in Python"""
    h_pub = o.blake3(b"".join((x % o.P).to_bytes(29, "little") for x in pub))
    d = o.blake3(bytes(seed) + j.to_bytes(8, "little") + proof + h_pub)
    return int.from_bytes(d[:16], "little") | (1 << 127)


def test_coefficient_pin(dvp):
    """with a fixed seed the coefficients are known before the trapdoor: choose delta' so that sum r_j e_j(tau, delta', eps) = 0
    for five proofs valid under TD (e_j = the discrete log of v0_j K_j + u0_j G - P_j).  With that seed the call must accept all five
    through COMBINED -- a false accept that pins r_j byte for byte -- while each proof fails on its own and the trapdoor-derived key
    (seed=None) falls back.  (Solving for tau' instead is degenerate here: every e_j(tau') is eps (tau' - tau) k_j.)"""
    S = dvp.srs
    tau, delta, eps = TD
    rng = random.Random(31)
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in range(5)]
    built = bulk(dvp, pubs, [None] * 5, seed=32)
    proofs, pubs = rows_of(built)
    seed = bytes(range(7, 39))
    r = [coeff(seed, j, proofs[j], pubs[j]) for j in range(5)]
    # e_j(delta') = eps [(delta' - delta) b0_j + (delta'^2 - delta^2) r0_j] = eps (delta' - delta) [b0_j + (delta' + delta) r0_j]
    r0 = [(c["a0"] * c["b0"] - o.evaluate_monomial_basis_poly(c["pub"], c["alpha"])) % o.P for c in built]
    sb = sum(rj * c["b0"] for rj, c in zip(r, built)) % o.P
    sr = sum(rj * x for rj, x in zip(r, r0)) % o.P
    delta2 = (-delta - sb * vc.inv(sr)) % o.P
    assert delta2 != delta
    tdx = S.Trapdoor(tau, delta2, eps)

    def err(j):
        c = built[j]
        u0 = (c["a0"] + delta2 * c["b0"] + delta2 * delta2 * r0[j]) * eps % o.P
        v0 = (tau - c["alpha"]) * eps % o.P
        return (v0 * c["k"] + u0 - c["p"]) % o.P

    assert all(err(j) for j in range(5)) and sum(rj * err(j) for j, rj in enumerate(r)) % o.P == 0
    v, rep = S.verify_batch_rlc(tdx, pubs, proofs, seed=seed)
    assert rep == S.VERIFY_RLC_COMBINED and not v.any(), (rep, v)
    ref = S.verify_batch(tdx, pubs, proofs)
    assert (ref == S.VERIFY_EQUATION).all(), ref
    v, rep = S.verify_batch_rlc(tdx, pubs, proofs)
    assert rep == S.VERIFY_RLC_FALLBACK and (v == S.VERIFY_EQUATION).all(), (rep, v)
    # and under TD itself the five are valid with either key
    for sd in (seed, None):
        v, rep = S.verify_batch_rlc(S.Trapdoor(*TD), pubs, proofs, seed=sd)
        assert rep == S.VERIFY_RLC_COMBINED and not v.any()


def test_trapdoor_key_is_deterministic(dvp):
    """seed=None: the same batch twice gives the same verdicts and report, on the combined and on the fallback path"""
    S, td = dvp.srs, dvp.srs.Trapdoor(*TD)
    rng = random.Random(41)
    pubs = [[rng.randrange(o.P)] for _ in range(100)]
    built = bulk(dvp, pubs, [None] * 100, seed=42)
    proofs, pubs = rows_of(built)
    bad, bad_pubs, _ = tampered_batch(dvp, built, ["a0_plus_1", "bad_kzg"], rng, per_kind=2)
    for p, q in ((proofs, pubs), (bad, bad_pubs)):
        v1, r1 = S.verify_batch_rlc(td, q, p)
        v2, r2 = S.verify_batch_rlc(td, q, p)
        assert r1 == r2 and (v1 == v2).all()
        assert r1 == expected_report(S, S.verify_batch(td, q, p))


def _dev_call(dvp, td, tpub, npub, tp, n, tv, trep, stream, seed=None):
    keep, (t, d, e) = dvp.srs._trapdoor_args(dvp.srs.Trapdoor(*td))
    sd = None if seed is None else np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    return dvp.lib.dvp_verify_batch_rlc_dev(t, d, e, C.c_void_p(tpub.data_ptr()), npub, C.c_void_p(tp.data_ptr()), n,
                                            None if sd is None else dvp._native.ptr(sd), C.c_void_p(tv.data_ptr()),
                                            None if trep is None else C.c_void_p(trep.data_ptr()), C.c_void_p(stream.cuda_stream))


def _to_dev(dvp, proofs, pubs, n):
    import torch

    dev = torch.device("cuda:0")
    pa = np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(n, 118)
    pub = dvp.srs._public_array(pubs, n)
    return pub, torch.from_numpy(pa.copy()).to(dev), torch.from_numpy(pub.view(np.int64).copy()).to(dev)


def test_dev_flavour_on_a_stream_matches_host(dvp):
    """dvp_verify_batch_rlc_dev on torch tensors and a non-default stream: the host flavour's verdicts and report (d_report); a
    non-canonical device public input is the BAD_PUBLIC verdict of its proof"""
    import torch

    S = dvp.srs
    rng = random.Random(3)
    n = 3000
    pubs = [[rng.randrange(o.P) for _ in range(3)] for _ in range(n)]
    built = bulk(dvp, pubs, [None] * n, seed=5)
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    for tamper in (False, True):
        proofs, pubs_t = rows_of(built)
        if tamper:
            for i in range(0, n, 97):
                proofs[i] = vc.tamper(built[i], vc.TAMPER[i % 11], rng)[0]
        host, host_rep = S.verify_batch_rlc(S.Trapdoor(*TD), pubs_t, proofs)
        pub, tp, tpub = _to_dev(dvp, proofs, pubs_t, n)
        tv = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        trep = torch.full((1,), 0x7777, dtype=torch.int32, device=dev)
        with torch.cuda.stream(s):
            assert _dev_call(dvp, TD, tpub, 3, tp, n, tv, trep, s) == 0
        s.synchronize()
        assert (tv.cpu().numpy() == host).all()
        assert int(trep.item()) == host_rep == (S.VERIFY_RLC_FALLBACK if tamper else S.VERIFY_RLC_COMBINED), (tamper, host_rep)
        # a non-canonical public input on the device
        pub[5, 1] = np.frombuffer(o.P.to_bytes(32, "little"), dtype="<u8")
        tpub = torch.from_numpy(pub.view(np.int64).copy()).to(dev)
        tv.fill_(0xEE)
        with torch.cuda.stream(s):
            assert _dev_call(dvp, TD, tpub, 3, tp, n, tv, trep, s) == 0
        s.synchronize()
        exp = host.copy()
        exp[5] = S.VERIFY_BAD_PUBLIC | (host[5] & ~np.uint8(S.VERIFY_EQUATION))
        got = tv.cpu().numpy()
        assert (got == exp).all(), np.nonzero(got != exp)[0][:10]
        assert int(trep.item()) == expected_report(S, exp)
        # without d_report
        tv.fill_(0xEE)
        with torch.cuda.stream(s):
            assert _dev_call(dvp, TD, tpub, 3, tp, n, tv, None, s) == 0
        s.synchronize()
        assert (tv.cpu().numpy() == exp).all()


def test_two_host_threads_on_one_device(dvp):
    """two threads, two streams, one device: a valid batch and one with a tampered proof, verified over and over at the same time --
    each gets its own right answer every time"""
    import torch

    S = dvp.srs
    rng = random.Random(61)
    n = 2000
    pubs = [[rng.randrange(o.P)] for _ in range(n)]
    built = bulk(dvp, pubs, [None] * n, seed=62)
    good_p, good_q = rows_of(built)
    bad_p, bad_q, where = tampered_batch(dvp, built, ["a0_plus_1"], rng, per_kind=1)
    (i_bad,) = where
    dev = torch.device("cuda:0")
    jobs = []
    for proofs, pq, exp_rep in ((good_p, good_q, S.VERIFY_RLC_COMBINED), (bad_p, bad_q, S.VERIFY_RLC_FALLBACK)):
        _, tp, tpub = _to_dev(dvp, proofs, pq, n)
        exp = np.zeros(n, dtype=np.uint8)
        if exp_rep == S.VERIFY_RLC_FALLBACK:
            exp[i_bad] = S.VERIFY_EQUATION
        jobs.append(dict(tp=tp, tpub=tpub, exp=exp, rep=exp_rep, s=torch.cuda.Stream(device=dev),
                         tv=torch.full((n,), 0xEE, dtype=torch.uint8, device=dev), trep=torch.zeros(1, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    errors = []
    barrier = threading.Barrier(2)

    def run(job):
        try:
            torch.cuda.set_device(0)
            barrier.wait()
            for _ in range(8):
                with torch.cuda.stream(job["s"]):
                    job["tv"].fill_(0xEE)
                    job["trep"].fill_(0x7777)
                    rc = _dev_call(dvp, TD, job["tpub"], 1, job["tp"], n, job["tv"], job["trep"], job["s"])
                job["s"].synchronize()
                got, rep = job["tv"].cpu().numpy(), int(job["trep"].item())
                if rc != 0 or rep != job["rep"] or not (got == job["exp"]).all():
                    errors.append((rc, rep, np.nonzero(got != job["exp"])[0][:5]))
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))

    th = [threading.Thread(target=run, args=(j,)) for j in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th)
    assert not errors, errors[:4]


def test_batch_of_2_16(dvp):
    """2^16 valid proofs (a 4096-proof pool tiled: every index has its own coefficient) report COMBINED; the same batch with one
    invalid proof at index 40000 gives dvp_verify_batch's verdicts"""
    S, td = dvp.srs, dvp.srs.Trapdoor(*TD)
    rng = random.Random(71)
    pool = 4096
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in range(pool)]
    built = bulk(dvp, pubs, [None] * pool, seed=72)
    pa = np.frombuffer(b"".join(c["proof"] for c in built), dtype=np.uint8).reshape(pool, 118)
    pub = S._public_array(pubs, pool)
    n = 1 << 16
    proofs = np.tile(pa, (n // pool, 1))
    pubs_n = np.tile(pub, (n // pool, 1, 1))
    v, rep = S.verify_batch_rlc(td, pubs_n, proofs)
    assert rep == S.VERIFY_RLC_COMBINED and not v.any(), (rep, np.nonzero(v)[0][:10])
    c = built[40000 % pool]
    proofs[40000, 60:89] = np.frombuffer(((c["a0"] + 1) % o.P).to_bytes(29, "little"), dtype=np.uint8)
    v, rep = S.verify_batch_rlc(td, pubs_n, proofs)
    ref = S.verify_batch(td, pubs_n, proofs)
    assert rep == S.VERIFY_RLC_FALLBACK
    assert (v == ref).all() and list(np.nonzero(v)[0]) == [40000] and v[40000] == S.VERIFY_EQUATION


def test_second_codec_rule(dvp):
    """under codec rule 1 a rule-1 batch is accepted through COMBINED; read back under rule 0 the verdicts are dvp_verify_batch's
    and the combined check falls back"""
    S, td = dvp.srs, dvp.srs.Trapdoor(*TD)
    rule = 1
    enc = lambda dl: vc.oracle_encode_many(dl, rule=rule)  # noqa: E731
    rng = random.Random(8)
    pubs = [[rng.randrange(o.P)] for _ in range(20)]
    cases = [None] * 13 + EXC
    dvp.check(dvp.lib.dvp_codec_set_rule(rule))
    try:
        built = vc.build(TD, pubs, cases, seed=9, encode_many=enc)
        proofs, pubs = rows_of(built)
        v, rep = S.verify_batch_rlc(td, pubs, proofs)
        assert not v.any() and rep == S.VERIFY_RLC_COMBINED, (v, rep)
    finally:
        dvp.check(dvp.lib.dvp_codec_set_rule(0))
    ref = S.verify_batch(td, pubs, proofs)
    v, rep = S.verify_batch_rlc(td, pubs, proofs)
    assert (v == ref).all(), (v, ref)
    assert ref.any() and rep == S.VERIFY_RLC_FALLBACK


def test_argument_errors(dvp):
    """DVP_EINVAL for a non-canonical trapdoor value, n_public above DVP_VERIFY_MAX_PUBLIC, a non-canonical host public input (its
    flat index in dvp_last_error_index), null buffers and n above DVP_VERIFY_RLC_MAX_PROOFS; n = 0 is DVP_OK"""
    S = dvp.srs
    rng = random.Random(91)
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in range(3)]
    built = bulk(dvp, pubs, [None] * 3, seed=92)
    proofs, pubs = rows_of(built)
    for bad_td in ((o.P, TD[1], TD[2]), (TD[0], o.P + 5, TD[2]), (TD[0], TD[1], (1 << 256) - 1)):
        with pytest.raises(dvp.DvpError) as ex:
            _raw_call(dvp, bad_td, pubs, proofs)
        assert ex.value.status == -1
    q = [list(r) for r in pubs]
    q[2][1] = o.P
    with pytest.raises(dvp.DvpError) as ex:
        S.verify_batch_rlc(S.Trapdoor(*TD), q, proofs)
    assert ex.value.status == -1 and ex.value.index == 5
    keep, (t, d, e) = S._trapdoor_args(S.Trapdoor(*TD))
    pa = S._proofs_array(proofs)
    pub = S._public_array(pubs, 3)
    out = np.zeros(3, dtype=np.uint8)
    ptr = dvp._native.ptr
    big = np.zeros(4, dtype=np.uint64)
    assert dvp.lib.dvp_verify_batch_rlc(t, d, e, ptr(big), 8193, ptr(pa), 3, None, ptr(out), None) == -1
    assert dvp.lib.dvp_verify_batch_rlc(t, d, e, ptr(pub), 2, None, 3, None, ptr(out), None) == -1
    assert dvp.lib.dvp_verify_batch_rlc(t, d, e, ptr(pub), 2, ptr(pa), 3, None, None, None) == -1
    assert dvp.lib.dvp_verify_batch_rlc(t, d, e, None, 2, ptr(pa), 3, None, ptr(out), None) == -1
    assert dvp.lib.dvp_verify_batch_rlc(t, d, e, ptr(pub), 2, ptr(pa), 1 << 26, None, ptr(out), None) == -1
    assert dvp.lib.dvp_verify_batch_rlc_dev(t, d, e, None, 0, C.c_void_p(16), 1 << 26, None, C.c_void_p(16), None, None) == -1
    assert dvp.lib.dvp_verify_batch_rlc_dev(t, d, e, None, 8193, None, 0, None, None, None, None) == -1
    rep = C.c_uint32(0x55)
    assert dvp.lib.dvp_verify_batch_rlc(t, d, e, None, 2, None, 0, None, None, C.byref(rep)) == 0 and rep.value == 0
    assert dvp.lib.dvp_verify_batch_rlc_dev(t, d, e, None, 2, None, 0, None, None, None, None) == 0
    v, r = S.verify_batch_rlc(S.Trapdoor(*TD), [], [])
    assert v.shape == (0,) and r == 0
    with pytest.raises(ValueError):
        S.verify_batch_rlc(S.Trapdoor(*TD), pubs, proofs, seed=b"short")


def _raw_call(dvp, td, pubs, proofs):
    """the host entry with raw trapdoor limbs (Trapdoor itself may reduce its values)"""
    S = dvp.srs
    raw = [np.frombuffer(int(x).to_bytes(32, "little"), dtype="<u8").copy() for x in td]
    pa = S._proofs_array(proofs)
    pub = S._public_array(pubs, len(proofs))
    out = np.zeros(len(proofs), dtype=np.uint8)
    ptr = dvp._native.ptr
    dvp.check(dvp.lib.dvp_verify_batch_rlc(*[ptr(a) for a in raw], ptr(pub), pub.shape[1], ptr(pa), len(proofs), None, ptr(out), None),
              "dvp_verify_batch_rlc")
