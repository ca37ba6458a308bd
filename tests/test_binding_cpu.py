"""CPU tests of the transcript binding: the host BLAKE3 on the long vectors (tests/golden/blake3_long.json), the bound host
transcript against the oracle's restatement, the verifier's process-wide binding, and the argument errors of every new entry that
needs no device."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import pyref as o
import binding_cases as bc

VEC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_vectors.json")))
EINVAL = -1


def test_fixture_is_the_oracles(dvp):
    """the fixture agrees with the entries tests/test_oracle.py pins to the published vectors, and with the oracle on a sample"""
    for n, h in VEC["blake3"].items():
        if int(n) in bc.B3_LONG:
            assert bc.B3_LONG[int(n)] == h, n
    assert {0, 1, 1025} <= set(bc.B3_LONG) and len(bc.B3_LONG) == 29
    for n in (65, 2049, 7169):
        assert o.blake3(bc.b3_input(n)).hex() == bc.B3_LONG[n]


def test_host_blake3_long_vectors(dvp):
    for n, h in bc.B3_LONG.items():
        assert dvp.proving.blake3(bc.b3_input(n)).hex() == h, n


def test_bound_challenge_vs_oracle(dvp):
    rnd = random.Random(31)
    tc = dvp.proving.transcript_challenge
    for npub in (0, 2, 36):
        commit = bytes(rnd.randrange(256) for _ in range(30))
        pub = [rnd.randrange(o.P) for _ in range(npub)]
        s, c = bytes(rnd.randrange(256) for _ in range(32)), bytes(rnd.randrange(256) for _ in range(32))
        unbound = o.transcript_challenge(commit, pub)
        assert tc(commit, pub) == unbound == bc.bound_challenge(commit, pub)
        assert tc(commit, pub, None, None) == unbound
        assert tc(commit, pub, o.blake3(b""), o.blake3(b"")) == unbound  # NULL means BLAKE3("")
        got = tc(commit, pub, s, c)
        assert got == bc.bound_challenge(commit, pub, s, c) and got != unbound
        assert tc(commit, pub, c, s) == bc.bound_challenge(commit, pub, c, s) != got  # the order of the two hashes matters
        assert tc(commit, pub, s, None) == bc.bound_challenge(commit, pub, s, None) != got
        assert tc(commit, pub, None, c) == bc.bound_challenge(commit, pub, None, c) != got
    # the raw entry with NULL, NULL is dvp_transcript_challenge
    cp = np.frombuffer(bytes(range(30)), dtype=np.uint8).copy()
    pub = dvp.fr.vec(o.TOY_PUBLIC)
    a, b = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ptr = dvp._native.ptr
    assert dvp.lib.dvp_transcript_challenge(ptr(cp), ptr(pub), 2, ptr(a)) == 0
    assert dvp.lib.dvp_transcript_challenge_bound(ptr(cp), ptr(pub), 2, None, None, ptr(b)) == 0
    assert a.tobytes() == b.tobytes() and hex(dvp.fr.to_int(a)) == VEC["challenge_toy"]


def test_verify_binding_round_trip(dvp):
    S = dvp.srs
    empty = o.blake3(b"")
    assert S.get_verify_binding() == (empty, empty)
    s, c = bytes(range(32)), bytes(range(100, 132))
    try:
        S.set_verify_binding(s, c)
        assert S.get_verify_binding() == (s, c)
        S.set_verify_binding(None, c)
        assert S.get_verify_binding() == (empty, c)
        S.set_verify_binding(s, None)
        assert S.get_verify_binding() == (s, empty)
    finally:
        S.set_verify_binding(None, None)
    assert S.get_verify_binding() == (empty, empty)
    with pytest.raises(ValueError):
        S.set_verify_binding(b"short", None)


def test_argument_errors_without_a_device(dvp):
    lib, ptr = dvp.lib, dvp._native.ptr
    h = np.zeros(32, dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    cp = np.zeros(30, dtype=np.uint8)
    assert lib.dvp_transcript_challenge_bound(None, None, 0, None, None, ptr(out)) == EINVAL
    assert lib.dvp_transcript_challenge_bound(ptr(cp), None, 1, None, None, ptr(out)) == EINVAL
    assert lib.dvp_transcript_challenge_bound(ptr(cp), None, 0, None, None, None) == EINVAL
    assert lib.dvp_transcript_challenge_bound(ptr(cp), None, 0, ptr(h), None, ptr(out)) == 0
    assert lib.dvp_verify_get_binding(None, ptr(h)) == EINVAL and lib.dvp_verify_get_binding(ptr(h), None) == EINVAL
    assert lib.dvp_prover_srs_hash(None, ptr(h)) == EINVAL
    assert lib.dvp_prover_set_transcript_binding(None, ptr(h), ptr(h)) == EINVAL
    assert lib.dvp_cache_dir_set_binding(None, 2, None, None, 0) == EINVAL
    # dvp_blake3_dev checks its arguments before it touches the device (the pointers are never followed)
    fake = C.c_void_p(0x1000)
    assert lib.dvp_blake3_dev(fake, 16, None, None) == EINVAL
    assert lib.dvp_blake3_dev(None, 16, fake, None) == EINVAL
    assert lib.dvp_blake3_dev(fake, (1 << 40) + 1, fake, None) == EINVAL
    assert lib.dvp_debug_blake3_leaves_dev(None, 1024, 0, fake, None) == EINVAL
    assert lib.dvp_debug_blake3_leaves_dev(fake, 0, 0, fake, None) == EINVAL
    assert lib.dvp_debug_blake3_leaves_dev(fake, 2048, (1 << 32) - 1, fake, None) == EINVAL  # the 32-bit chunk counter
    assert lib.dvp_debug_blake3_reduce_dev(fake, 1, fake, fake, None) == EINVAL
    assert lib.dvp_debug_blake3_tree_run() >= 2
