"""GPU tests (-m gpu) of the arkworks boundary: k_fr_from_ark / k_fr_to_ark (csrc/fr_ark.hip) against Python integers at the block-edge
sizes, and the entries that take Fr vectors as arkworks holds them in memory -- dvp_prove_ark, dvp_prove_cache_dir_ark,
dvp_msm_xsk233_ark, dvp_msm_ctx_run_ark -- against the canonical entries on the same statement.  The arkworks form of every input is
made from Python integers (tests/ark_cases.py), not by the library."""
import random
import threading

import numpy as np
import pytest

import ark_cases as ac
import msm_cases as mc

pytestmark = pytest.mark.gpu
K_FROM, K_TO = "fr_ark.hip:k_fr_from_ark", "fr_ark.hip:k_fr_to_ark"
EINVAL, EUNSAT = -1, -3
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, len(ac.VALUES)]  # around the wave (64) and the workgroup (256), several workgroups
# the boundary values sit behind witness_cases' 4096 random ones: every size takes its values from the END of the list
TAIL = lambda seq, n: seq[len(seq) - n:]


def u64(ints) -> np.ndarray:
    return np.frombuffer(ac.limbs_bytes(ints), dtype=np.uint64).reshape(-1, 4)


def ark(ints) -> np.ndarray:
    """the memory of a Vec<Fr> holding these values"""
    return u64([ac.to_ark(x) for x in ints])


@pytest.mark.parametrize("direction", ["from_ark", "to_ark"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_python_integers(dvp, n, direction):
    import torch

    host, dev, kernel, other, expected = ((dvp.fr.from_ark, dvp.fr.from_ark_dev, K_FROM, K_TO, ac.FROM_ARK) if direction == "from_ark" else
                                          (dvp.fr.to_ark, dvp.fr.to_ark_dev, K_TO, K_FROM, ac.TO_ARK))
    raw = ac.limbs_bytes(TAIL(ac.VALUES, n))
    want = ac.limbs_bytes(TAIL(expected, n))
    # host-pointer flavour, from an address that is not even 2-byte aligned
    odd = np.frombuffer(b"\x00" * 3 + raw, dtype=np.uint8)[3:]
    assert odd.ctypes.data % 2 == 1
    dvp.lib.dvp_profile_reset()
    assert host(odd.view(np.uint64)).tobytes() == want
    assert mc.launches(dvp, kernel) == 1 and mc.launches(dvp, other) == 0
    st = torch.cuda.current_stream().cuda_stream
    # device flavour, out of place: the input stays, and nothing is written beyond element n - 1
    src = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    dst = torch.full((32 * (n + 2),), 0xAB, dtype=torch.uint8, device="cuda")
    dvp.lib.dvp_profile_reset()
    dev(src.data_ptr(), n, dst.data_ptr(), st)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().tobytes()
    assert got[:32 * n] == want and got[32 * n:] == b"\xab" * 64
    assert src.cpu().numpy().tobytes() == raw
    assert mc.launches(dvp, kernel) == 1 and mc.launches(dvp, other) == 0
    # device flavour, in place: d_out NULL, and d_out == d_in
    for same in (False, True):
        buf = torch.full((32 * (n + 2),), 0xCD, dtype=torch.uint8, device="cuda")
        buf[:32 * n] = src
        dvp.lib.dvp_profile_reset()
        dev(buf.data_ptr(), n, buf.data_ptr() if same else None, st)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().tobytes()
        assert got[:32 * n] == want and got[32 * n:] == b"\xcd" * 64
        assert mc.launches(dvp, kernel) == 1 and mc.launches(dvp, other) == 0


# ---- proofs ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def statements(dvp):
    """name -> (prover, trapdoor, public, private): the toy circuit and synthetic_sparse(10), with two public inputs and with none"""
    import pyref as o

    g = dvp.gnark_r1cs
    made = {}
    rnd = random.Random(0xA4C)
    toy_w = list(g.TOY_PUBLIC) + list(g.TOY_PRIVATE)
    sp2 = g.synthetic_sparse(10)
    sp0 = g.synthetic_sparse(10, n_public=0)
    for name, inst, pub, prv in (("toy", g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 2), toy_w[:2], toy_w[2:]),
                                 ("toy-nopub", g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 0), [], toy_w),
                                 ("sparse10", *sp2), ("sparse10-nopub", *sp0)):
        td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
        pv = dvp.proving.Prover(inst)
        pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, td))
        made[name] = (pv, td, [int(x) for x in pub], [int(x) for x in prv])
    yield made
    for pv, *_ in made.values():
        pv.close()


@pytest.mark.parametrize("devices", [[], [0, 0]], ids=["one-device", "devices-0-0"])
@pytest.mark.parametrize("name", ["toy", "toy-nopub", "sparse10", "sparse10-nopub"])
def test_prove_ark_same_bytes_as_prove(dvp, statements, name, devices):
    pv, td, pub, prv = statements[name]
    try:
        dvp.set_devices(devices)
        ref = pv.prove(pub, prv)
        dvp.lib.dvp_profile_reset()
        got = pv.prove_ark(ark(pub), ark(prv))
        assert mc.launches(dvp, K_FROM) == 1 and mc.launches(dvp, K_TO) == 0
        # negative control: the CANONICAL limbs through the same entry are taken as arkworks form, i.e. as another witness
        try:
            wrong = pv.prove_ark(u64(pub), u64(prv))
        except dvp.DvpError as e:
            assert e.status == EUNSAT
        else:
            assert wrong.to_bytes() != ref.to_bytes() and not dvp.srs.verify(td, pub, wrong)
    finally:
        dvp.set_devices([])
    assert got.to_bytes() == ref.to_bytes() and len(got.to_bytes()) == 118
    assert dvp.srs.verify(td, pub, got)


def test_prove_ark_errors(dvp, statements):
    import pyref as o

    pv, _, pub, prv = statements["sparse10"]
    ref = pv.prove(pub, prv)
    # an unsatisfied witness: the status and the row dvp_prove reports
    bad = list(prv)
    bad[100] = (bad[100] + 1) % o.P
    with pytest.raises(dvp.DvpError) as e1:
        pv.prove(pub, bad)
    with pytest.raises(dvp.DvpError) as e2:
        pv.prove_ark(ark(pub), ark(bad))
    assert e1.value.status == e2.value.status == EUNSAT and e1.value.index == e2.value.index >= 0
    # a private vector one element short, one too long, a public vector of the wrong length: refused, and the kernel never ran
    dvp.lib.dvp_profile_reset()
    for a, b in ((pub, prv[:-1]), (pub, prv + [5]), (pub[:-1], prv), (pub[:-1], prv + [5])):
        with pytest.raises(dvp.DvpError) as e:
            pv.prove_ark(ark(a), ark(b))
        assert e.value.status == EINVAL
    assert mc.launches(dvp, K_FROM) == 0
    # and the prover is fine afterwards
    assert pv.prove_ark(ark(pub), ark(prv)).to_bytes() == ref.to_bytes()


# ---- the cache_dir entry ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cache(dvp, tmp_path_factory):
    """a cache_dir for synthetic_sparse(10); (path, trapdoor, public, private, Proof.prove's proof from canonical limbs)"""
    A, g = dvp.artifacts, dvp.gnark_r1cs
    inst0, pub, prv = g.synthetic_sparse(10)
    pub, prv = [int(x) for x in pub], [int(x) for x in prv]
    path = tmp_path_factory.mktemp("fr_ark") / "cache"
    path.mkdir()
    inst0.write_dump_file(path / A.R1CS_CONSTRAINTS_FILE)
    td = dvp.srs.Trapdoor(31, 41, 59)
    _, pv = dvp.srs.verifier_runs_setup_cache_dir(td, path, len(pub), write_precomputes=False)
    pv.close()
    ref = dvp.proving.Proof.prove(path, pub, prv)
    assert dvp.srs.verify(td, pub, ref)
    yield path, td, pub, prv, ref
    dvp.proving.release_cache_dir()


def test_cache_dir_entry_same_bytes_as_proof_prove(dvp, cache):
    path, td, pub, prv, ref = cache
    a_pub, a_prv = ark(pub), ark(prv)
    dvp.lib.dvp_profile_reset()
    got = dvp.proving.Proof.prove_ark(path, a_pub, a_prv)
    assert mc.launches(dvp, K_FROM) == 1
    assert got.to_bytes() == ref.to_bytes() and dvp.srs.verify(td, pub, got)
    with pytest.raises(dvp.DvpError) as e:
        dvp.proving.Proof.prove_ark(path, a_pub, a_prv[:-1])
    assert e.value.status == EINVAL
    # two host threads on one cache_dir at once
    bad = []

    def loop():
        try:
            for _ in range(4):
                if dvp.proving.Proof.prove_ark(path, a_pub, a_prv).to_bytes() != ref.to_bytes():
                    bad.append("bytes")
        except Exception as ex:  # noqa: BLE001 -- report from the main thread
            bad.append(repr(ex))

    th = [threading.Thread(target=loop) for _ in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, bad


# ---- MSM -------------------------------------------------------------------------------------------------------------------------
def rand_scalars(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(ac.P) for _ in range(n)]


@pytest.mark.parametrize("n,special", [(1, [0]), (1, [1]), (1, [ac.P - 1]), (2, [0, 1]), (2, [ac.P - 1, 1]), (257, [0, 1, ac.P - 1])],
                         ids=["1-zero", "1-one", "1-pm1", "2-zero-one", "2-pm1-one", "257"])
def test_msm_xsk233_ark_same_point_as_canonical(dvp, n, special):
    s = (special + rand_scalars(n, 0x51 + n))[:n]
    enc = dvp.curve.point_scalar_mul_gen_batch_bytes(u64(rand_scalars(n, 0x52 + n)))
    want = dvp.curve.multi_scalar_mul_bytes(u64(s).view(np.uint8).reshape(n, 32), enc)
    dvp.lib.dvp_profile_reset()
    assert dvp.curve.multi_scalar_mul_bytes_ark(ark(s), enc) == want
    assert mc.launches(dvp, K_FROM) == 1 and mc.launches(dvp, K_TO) == 0
    if n > 1:  # the canonical limbs through the _ark entry are other scalars
        assert dvp.curve.multi_scalar_mul_bytes_ark(u64(s), enc) != want


def test_msm_ctx_run_ark_same_point_as_canonical(dvp):
    n = 300
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(u64(rand_scalars(n, 0x61)))
    assert not inf.any()
    s = [0, 1, ac.P - 1] + rand_scalars(n - 3, 0x62)
    fb = dvp.curve.FixedBaseMsm(bases)
    try:
        for lo, hi in ((0, n), (37, 291), (1, 3), (299, 300)):
            want_xy, want_inf = fb.run(u64(s[lo:hi]), lo, hi)
            dvp.lib.dvp_profile_reset()
            xy, is_inf = fb.run_ark(ark(s[lo:hi]), lo, hi)
            assert mc.launches(dvp, K_FROM) == 1
            assert is_inf == want_inf and xy.tobytes() == want_xy.tobytes(), (lo, hi)
        with pytest.raises(dvp.DvpError) as e:  # a range beyond the context
            fb.run_ark(ark(s[:2]), n - 1, n + 1)
        assert e.value.status == EINVAL
    finally:
        fb.close()
