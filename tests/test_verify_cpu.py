"""CPU tests of the verifier entries (dvp_verify*, dvp_sp1_public_input): the synthetic-proof generator of verify_cases.py
against the discrete-log form of SRS::verify, the argument checks that return before any GPU work, and the SP1 public-input
scalar against the oracle's BLAKE3."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as o
import verify_cases as vc

TD = (0x1234567 * 7919 % o.P, 0xABCDEF12345 % o.P, 0x9E3779B97F4A7C15 % o.P)


def _limbs(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").copy()


@pytest.mark.parametrize("case", (None,) + vc.CASES)
def test_generator_is_sound(case):
    """every valid case satisfies v0 K + u0 G == P on discrete logs; every tampered scalar breaks it"""
    rng = random.Random(hash(case) & 0xFFFF)
    pub = [rng.randrange(o.P) for _ in range(3)]
    (c,) = vc.build(TD, [pub], [case], seed=11)
    assert c["alpha"] == o.transcript_challenge(c["proof"][:30], pub)
    assert o.verify_dl(c["td"], pub, c["p"], c["k"], c["a0"], c["b0"], c["alpha"])
    assert not o.verify_dl(c["td"], pub, c["p"], c["k"], (c["a0"] + 1) % o.P, c["b0"], c["alpha"])
    assert not o.verify_dl(c["td"], pub, c["p"] + 1, c["k"], c["a0"], c["b0"], c["alpha"])
    assert not o.verify_dl(c["td"], pub[:-1] + [pub[-1] + 1], c["p"], c["k"], c["a0"], c["b0"], c["alpha"])
    tau, delta, eps = c["td"]
    v0 = (tau - c["alpha"]) * eps % o.P
    if case == "v0_zero":
        assert v0 == 0
    if case == "k_zero":
        assert c["k"] == 0 and c["proof"][30:60] == bytes(30)
    if case == "p_zero":
        assert c["proof"][:30] == bytes(30)
    if case in ("k_plus_g", "k_minus_g"):
        assert c["k"] == (1 if case == "k_plus_g" else o.P - 1)


def test_oracle_verdict_matches_generator():
    """the reference's boolean on the C oracle accepts the valid cases and rejects a tampered one of each kind"""
    rng = random.Random(5)
    cases = vc.build(TD, [[rng.randrange(o.P)] for _ in vc.CASES], list(vc.CASES), seed=3)
    for c in cases:
        assert vc.oracle_verdict(c["td"], c["pub"], c["proof"]), c["case"]
    for kind in vc.TAMPER:
        b, td, pub = vc.tamper(cases[0], kind, rng)
        assert not vc.oracle_verdict(td, pub, b), kind


def _td_ptrs(td):
    arrs = [_limbs(x) for x in td]
    return arrs, [a.ctypes.data_as(C.c_void_p) for a in arrs]


def test_verify_argument_checks(dvp):
    """DVP_EINVAL for a trapdoor value >= p and for a non-canonical public input (with its flat index); n = 0 is OK -- all before
    any device work, so these run without a GPU"""
    lib = dvp.lib
    proofs = np.zeros((3, 118), dtype=np.uint8)
    verdicts = np.zeros(3, dtype=np.uint8)
    pub = np.zeros((3, 2, 4), dtype=np.uint64)
    pp, vp_, pubp = (a.ctypes.data_as(C.c_void_p) for a in (proofs, verdicts, pub))
    for bad in range(3):
        td = list(TD)
        td[bad] = o.P + bad
        keep, (t, d, e) = _td_ptrs(td)
        assert lib.dvp_verify_batch(t, d, e, pubp, 2, pp, 3, vp_) == -1
        assert lib.dvp_verify_batch_dev(t, d, e, pubp, 2, pp, 3, vp_, None) == -1
        acc = C.c_int(7)
        assert lib.dvp_verify(t, d, e, pubp, 2, pp, C.byref(acc), None) == -1
    keep, (t, d, e) = _td_ptrs(TD)
    assert lib.dvp_verify_batch(t, d, e, None, 0, None, 0, None) == 0
    assert lib.dvp_verify_batch_dev(t, d, e, None, 0, None, 0, None, None) == 0
    assert lib.dvp_verify_batch(t, d, e, pubp, 8193, pp, 1, vp_) == -1  # > DVP_VERIFY_MAX_PUBLIC
    pub[2, 1] = _limbs(o.P)  # flat index 2 * 2 + 1
    assert lib.dvp_verify_batch(t, d, e, pubp, 2, pp, 3, vp_) == -1
    assert lib.dvp_last_error_index() == 5
    pub[2, 1] = _limbs(o.P - 1)
    pub[0, 0] = _limbs(1 << 255)
    assert lib.dvp_verify_batch(t, d, e, pubp, 2, pp, 3, vp_) == -1
    assert lib.dvp_last_error_index() == 0
    # zero trapdoor values are not rejected (the reference does not); n = 0 with them is OK
    keep0, (t0, d0, e0) = _td_ptrs((0, 0, 0))
    assert lib.dvp_verify_batch(t0, d0, e0, None, 0, None, 0, None) == 0
    assert dvp.srs.verify_batch(dvp.srs.Trapdoor(*TD), [], np.zeros((0, 118), dtype=np.uint8)).shape == (0,)


def _sp1_expected(raw):
    h = o.blake3(int(raw).to_bytes(8, "little"))
    return int.from_bytes(bytes(4) + h[4:], "big")


def test_sp1_public_input(dvp):
    """sp1_generate_scalar_from_raw_public_input (src/gnark_r1cs.rs:214-229): BLAKE3 of the LE bytes, bytes 0..3 cleared, big-endian"""
    rng = random.Random(9)
    for raw in [0, 1, 2**64 - 1] + [rng.randrange(2**64) for _ in range(20)]:
        got = dvp.srs.sp1_public_input(raw)
        assert got == _sp1_expected(raw), hex(raw)
        assert got < 2**224 < o.P
    assert dvp.lib.dvp_sp1_public_input(5, None) == -1
