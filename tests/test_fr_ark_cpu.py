"""The arkworks boundary without a GPU: the per-element functions of k_fr_from_ark / k_fr_to_ark (csrc/fr_ark.cuh) in their host build,
byte for byte against Python integers on tests/ark_cases.py; fr_ark_is_one; and every answer the new entries give before they touch a
device."""
import numpy as np
import pytest

import ark_cases as ac

EINVAL = -1


def u64(raw: bytes) -> np.ndarray:
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4)


def test_host_build_matches_python_integers(dvp):
    fr = dvp.fr
    src = u64(ac.limbs_bytes(ac.VALUES))
    got = fr.from_ark_host(src)
    assert got.dtype == np.uint64 and got.shape == (len(ac.VALUES), 4)
    assert got.tobytes() == ac.limbs_bytes(ac.FROM_ARK)
    assert fr.to_ark_host(src).tobytes() == ac.limbs_bytes(ac.TO_ARK)
    assert src.tobytes() == ac.limbs_bytes(ac.VALUES)  # the input is not written


def test_round_trips(dvp):
    fr = dvp.fr
    src = u64(ac.limbs_bytes(ac.VALUES))
    reduced = ac.limbs_bytes([x % ac.P for x in ac.VALUES])
    assert fr.to_ark_host(fr.from_ark_host(src)).tobytes() == reduced
    assert fr.from_ark_host(fr.to_ark_host(src)).tobytes() == reduced


def test_one_element_at_a_time_and_from_an_odd_address(dvp):
    """no dependence on the neighbours or on alignment"""
    fr = dvp.fr
    for fn, want in ((fr.from_ark_host, ac.FROM_ARK), (fr.to_ark_host, ac.TO_ARK)):
        for off in (1, 3, 5):
            buf = np.frombuffer(b"\xff" * off + ac.limbs_bytes(ac.VALUES[-120:]), dtype=np.uint8)[off:]
            assert buf.ctypes.data % 2 == 1
            assert fn(buf.view(np.uint64)).tobytes() == ac.limbs_bytes(want[-120:])
            assert fn(bytes(buf)).tobytes() == ac.limbs_bytes(want[-120:])  # bytes are taken as well
        for i in list(range(len(ac.VALUES) - 300, len(ac.VALUES) - 256)) + [0, 3, 9, 10]:
            assert dvp.fr.to_ints(fn(u64(ac.limbs_bytes([ac.VALUES[i]])))) == [want[i]], i


def test_ark_is_one_only_for_representatives_of_r(dvp):
    is_one = lambda x: dvp.fr.ark_is_one(int(x).to_bytes(32, "little"))
    assert is_one(ac.R)
    ks = [k for k in (1, 2, 3, 2**10, 2**24, ac.wc.K_MAX - 1, ac.wc.K_MAX) if ac.R + k * ac.P < 2**256]
    assert len(ks) >= 6
    for k in ks:
        assert is_one(ac.R + k * ac.P), k
    for x in (1, 0, ac.P, ac.R - 1, ac.R + 1, ac.R + ac.P - 1, ac.R ^ (1 << 255), 2**256 - 1, ac.R * ac.R % ac.P):
        assert not is_one(x), x
    # from an odd address
    buf = np.frombuffer(b"\x00" + ac.R.to_bytes(32, "little"), dtype=np.uint8)[1:]
    assert dvp.lib.dvp_debug_fr_ark_is_one(buf.ctypes.data) == 1
    assert dvp.lib.dvp_debug_fr_ark_is_one(None) == EINVAL


def test_entries_check_arguments_before_any_device_call(dvp, nat, tmp_path):
    lib = dvp.lib
    src = np.zeros(64 + 16, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    base = src.ctypes.data + (-src.ctypes.data) % 16  # a 16-byte aligned address (a HOST one: a launch on it would be refused or fault)
    for fn in (lib.dvp_fr_from_ark, lib.dvp_fr_to_ark):
        assert fn(None, 0, None) == 0
        assert fn(None, 2, nat.ptr(out)) == EINVAL and fn(base, 2, None) == EINVAL
    for to_ark in (0, 1):
        assert lib.dvp_debug_fr_ark_host(to_ark, None, 0, None) == 0
        assert lib.dvp_debug_fr_ark_host(to_ark, None, 2, nat.ptr(out)) == EINVAL
        assert lib.dvp_debug_fr_ark_host(to_ark, base, 2, None) == EINVAL
    for dev in (lib.dvp_fr_from_ark_dev, lib.dvp_fr_to_ark_dev):
        assert dev(None, 0, None, None) == 0
        assert dev(base + 8, 0, base + 4, None) == 0  # n = 0 touches nothing
        assert dev(None, 2, base, None) == EINVAL
        assert dev(None, 2, None, None) == EINVAL
        for off in (1, 4, 8):
            assert dev(base + off, 2, base, None) == EINVAL
            assert dev(base, 2, base + off, None) == EINVAL
            assert dev(base + off, 2, base + off, None) == EINVAL
            assert dev(base + off, 2, None, None) == EINVAL  # in place on a misaligned address
        # more elements than one launch holds: refused before anything is allocated, copied or launched
        for n in (0xFFFFFF01, 1 << 32, (1 << 59) + 1):
            assert dev(base, n, base, None) == EINVAL
            assert dev(base, n, None, None) == EINVAL
    for n in (0xFFFFFF01, 1 << 32, (1 << 59) + 1):
        assert lib.dvp_fr_from_ark(base, n, nat.ptr(out)) == EINVAL
        assert lib.dvp_fr_to_ark(base, n, nat.ptr(out)) == EINVAL
    proof = np.zeros(118, dtype=np.uint8)
    assert lib.dvp_prove_ark(None, base, 1, base, 1, nat.ptr(proof)) == EINVAL
    # the cache_dir entry: NULL arguments are refused before the directory (which does not exist) is opened
    nowhere = str(tmp_path / "no_such_cache_dir").encode()
    assert lib.dvp_prove_cache_dir_ark(None, base, 1, base, 1, nat.ptr(proof)) == EINVAL
    assert lib.dvp_prove_cache_dir_ark(nowhere, base, 1, base, 1, None) == EINVAL
    assert lib.dvp_prove_cache_dir_ark(nowhere, None, 1, base, 1, nat.ptr(proof)) == EINVAL
    assert lib.dvp_prove_cache_dir_ark(nowhere, base, 1, None, 1, nat.ptr(proof)) == EINVAL
    # the MSM entries
    enc = np.zeros(60, dtype=np.uint8)
    assert lib.dvp_msm_xsk233_ark(None, nat.ptr(enc), 2, nat.ptr(enc)) == EINVAL
    assert lib.dvp_msm_xsk233_ark(base, None, 2, nat.ptr(enc)) == EINVAL
    assert lib.dvp_msm_xsk233_ark(base, nat.ptr(enc), 2, None) == EINVAL
    import ctypes as C

    inf = C.c_int(0)
    assert lib.dvp_msm_ctx_run_ark(None, base, 0, 2, nat.ptr(out), C.byref(inf)) == EINVAL


def test_wrappers_check_shapes(dvp):
    fr = dvp.fr
    for fn in (fr.from_ark, fr.to_ark, fr.from_ark_host, fr.to_ark_host):
        assert fn(b"").shape == (0, 4) and fn(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)  # n = 0: no device
        for bad in (b"\x00" * 33, np.zeros((2, 3), dtype=np.uint64), np.zeros((1, 2, 4), dtype=np.uint64), np.zeros(6, dtype=np.uint64),
                    np.zeros((2, 32), dtype=np.uint8), np.zeros((2, 4), dtype=np.int64)):
            with pytest.raises(ValueError):
                fn(bad)
    assert fr.from_ark_host(np.zeros(8, dtype=np.uint64)).shape == (2, 4)  # a flat buffer of 4 n words is n elements
    good = np.zeros((2, 4), dtype=np.uint64)
    for bad in (b"\x00" * 33, np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 32), dtype=np.uint8)):
        for args in ((bad, good), (good, bad)):
            with pytest.raises(ValueError):
                dvp.proving.Prover.prove_ark(None, *args)  # refused before the handle is looked at
            with pytest.raises(ValueError):
                dvp.proving.Proof.prove_ark("no_such_cache_dir", *args)
        with pytest.raises(ValueError):
            dvp.curve.multi_scalar_mul_bytes_ark(bad, np.zeros((2, 30), dtype=np.uint8))
    with pytest.raises(ValueError):
        dvp.curve.multi_scalar_mul_bytes_ark(good, np.zeros((3, 30), dtype=np.uint8))  # counts differ
    with pytest.raises(ValueError):
        fr.ark_is_one(b"\x00" * 31)
