"""The witness wire without a GPU: the per-element function of k_fr_from_be32 (csrc/fr_wire.cuh: 32 bytes big-endian, any x < 2^256,
-> x mod p) in its host build, byte for byte against Python integers on tests/witness_cases.py; the old host reducer
(dvp_file_witness_read) on the same values; and every answer the new entries give before they touch a device."""
import struct

import numpy as np
import pytest

import witness_cases as wc

EINVAL, EIO = -1, -6


def expected_limbs():
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in wc.EXPECTED), dtype="<u8").reshape(-1, 4)


def test_host_build_matches_python_integers(dvp):
    out = dvp.fr.from_be32_host(wc.be32(wc.VALUES))
    assert out.dtype == np.uint64 and out.shape == (len(wc.VALUES), 4)
    assert out.tobytes() == expected_limbs().tobytes()
    # one element at a time and from an odd address: no dependence on the neighbours or on alignment
    buf = np.frombuffer(b"\xff" * 5 + wc.be32(wc.VALUES[:40]), dtype=np.uint8)[5:]
    assert dvp.fr.from_be32_host(buf).tobytes() == expected_limbs()[:40].tobytes()
    for i in (0, 3, 9, 10):
        assert dvp.fr.to_ints(dvp.fr.from_be32_host(wc.be32([wc.VALUES[i]]))) == [wc.EXPECTED[i]]


def test_old_host_reducer_agrees(dvp, tmp_path):
    """dvp_file_witness_read (25 conditional subtractions per element) on a file of the raw, unreduced values: identical limbs"""
    path = tmp_path / "raw_witness"
    path.write_bytes(wc.witness_file_bytes(wc.VALUES))
    old = dvp.gnark_r1cs.load_witness_from_file(path)
    assert old.tobytes() == expected_limbs().tobytes()
    raw = dvp.gnark_r1cs.read_witness_raw(path)
    assert raw.dtype == np.uint8 and raw.shape == (len(wc.VALUES), 32) and raw.tobytes() == wc.be32(wc.VALUES)  # no reduction
    assert dvp.fr.from_be32_host(raw).tobytes() == old.tobytes()


def test_vector_entries_check_arguments_before_any_device_call(dvp, nat):
    lib = dvp.lib
    src = np.zeros(64 + 16, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    base = src.ctypes.data + (-src.ctypes.data) % 16  # a 16-byte aligned address (a HOST one: a launch on it would be refused or fault)
    for fn in (lib.dvp_fr_from_be32, lib.dvp_debug_fr_from_be32_host):
        assert fn(None, 0, None) == 0
        assert fn(None, 2, nat.ptr(out)) == EINVAL and fn(base, 2, None) == EINVAL
    assert lib.dvp_fr_from_be32_dev(None, 0, None, None) == 0
    assert lib.dvp_fr_from_be32_dev(base + 8, 0, base + 4, None) == 0  # n = 0 touches nothing
    assert lib.dvp_fr_from_be32_dev(None, 2, base, None) == EINVAL
    assert lib.dvp_fr_from_be32_dev(base, 2, None, None) == EINVAL
    for off in (1, 4, 8):
        assert lib.dvp_fr_from_be32_dev(base + off, 2, base, None) == EINVAL
        assert lib.dvp_fr_from_be32_dev(base, 2, base + off, None) == EINVAL
        assert lib.dvp_fr_from_be32_dev(base + off, 2, base + off, None) == EINVAL
    # more elements than one launch holds: refused before anything is allocated or copied (no device here to refuse it otherwise)
    for n in (0xFFFFFF01, 1 << 32, (1 << 59) + 1):
        assert lib.dvp_fr_from_be32(base, n, nat.ptr(out)) == EINVAL
        assert lib.dvp_fr_from_be32_dev(base, n, base, None) == EINVAL
    proof = np.zeros(118, dtype=np.uint8)
    assert lib.dvp_prove_be32(None, base, 2, nat.ptr(proof)) == EINVAL


def test_file_entry_judges_the_file_before_it_opens_cache_dir(dvp, nat, tmp_path):
    """a missing file and a count the bytes cannot hold are DVP_EIO, element 0 == 0 (mod p) is DVP_EINVAL with index 0 -- with a cache_dir
    that does not even exist, so nothing was opened and no device was asked"""
    lib = dvp.lib
    nowhere = str(tmp_path / "no_such_cache_dir").encode()
    proof = np.zeros(118, dtype=np.uint8)
    pub = np.zeros((2, 4), dtype=np.uint64)
    call = lambda cd, path, pr=proof: lib.dvp_prove_cache_dir_witness_file(cd, 2, path, None if pr is None else nat.ptr(pr), nat.ptr(pub))
    assert call(None, b"x") == EINVAL and call(nowhere, b"x", None) == EINVAL
    assert call(nowhere, str(tmp_path / "missing").encode()) == EIO
    assert call(nowhere, None) == EIO  # <cache_dir>/witness_to_dvsnark
    f = tmp_path / "w"
    good = [1, 5, 6, 7, 8]
    for blob in (b"", b"\x00\x00", struct.pack(">I", 5) + wc.be32(good)[:-1], struct.pack(">I", 6) + wc.be32(good), struct.pack(">I", 0xFFFFFFFF) + wc.be32(good)):
        f.write_bytes(blob)
        assert call(nowhere, str(f).encode()) == EIO, len(blob)
    f.write_bytes(wc.witness_file_bytes([1, 5]))  # fewer than 1 + n_public elements
    assert call(nowhere, str(f).encode()) == EINVAL
    for e0 in (0, wc.P, 2, wc.P + 2, 2**256 - 1):
        with pytest.raises(dvp.DvpError) as err:  # moves the thread's error index away from 0 (a host-only precondition failure)
            dvp.fr.debug_op("add", [b"\x00" * 32 + b"\xff" * 32, b"\x00" * 64], False)
        assert err.value.index == 1 and lib.dvp_last_error_index() == 1
        f.write_bytes(wc.witness_file_bytes([e0] + good[1:]))
        assert call(nowhere, str(f).encode()) == EINVAL and lib.dvp_last_error_index() == 0, e0
    # element 0 == 1 in either representative passes the host's checks: the call then fails at the cache_dir that is not there
    for e0 in (1, 1 + wc.P, 1 + wc.K_MAX * wc.P):
        f.write_bytes(wc.witness_file_bytes([e0] + good[1:]))
        assert call(nowhere, str(f).encode()) == EIO, e0
    with pytest.raises(dvp.DvpError) as e:
        dvp.proving.Proof.prove_witness_file(tmp_path / "no_such_cache_dir", 2)
    assert e.value.status == EIO


def test_wrappers_check_shapes(dvp, tmp_path):
    fr, g = dvp.fr, dvp.gnark_r1cs
    assert fr.from_be32(b"").shape == (0, 4) and fr.from_be32(np.zeros((0, 32), dtype=np.uint8)).shape == (0, 4)  # n = 0: no device
    for bad in (b"\x00" * 33, np.zeros((2, 31), dtype=np.uint8), np.zeros((1, 2, 16), dtype=np.uint8), np.zeros(8, dtype=np.uint64)):
        for fn in (fr.from_be32, fr.from_be32_host):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError):
            dvp.proving.Prover.prove_be32(None, bad)  # refused before the handle is looked at
    assert fr.from_be32_host(np.zeros(64, dtype=np.uint8)).shape == (2, 4)  # a flat buffer of 32 n bytes is n elements
    short = tmp_path / "short"
    for blob in (b"\x00", struct.pack(">I", 2) + b"\x00" * 63):
        short.write_bytes(blob)
        with pytest.raises(ValueError):
            g.read_witness_raw(short)
    short.write_bytes(struct.pack(">I", 1) + b"\x00" * 40)  # trailing bytes beyond the count are not part of the payload
    assert g.read_witness_raw(short).shape == (1, 32)
