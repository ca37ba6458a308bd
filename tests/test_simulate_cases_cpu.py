"""CPU tests of tests/simulate_cases.py, the plain-Python restatement of dvp_simulate_batch that the GPU tests compare the kernel
with: its proofs are accepted by the reference's check restated on the C oracle (verify_cases.oracle_verdict), and its draws, its
determinism and its special inputs are what include/dvpari.h states.  The oracle's verdict takes about 0.6 s per proof, so the whole file
asks for 15 of them: 14 shared proofs and the one with the bumped b0; every discrete log is encoded once."""
import pytest

import pyref as o
import simulate_cases as sc
import verify_cases as vc

TD = (0x3D9F1A77 * 104729 % o.P, 0xC0FFEE1234567 % o.P, 0xDEADBEEF987654321 % o.P)
SEED = bytes(range(32))
N_PUBLIC = (0, 36)  # 36 x 29 B crosses one BLAKE3 chunk

_enc = {}


def encode_many(dlogs):
    """the oracle's encodings, each discrete log encoded once for the whole file"""
    miss = [k for k in dict.fromkeys(dlogs) if k not in _enc]
    _enc.update(zip(miss, vc.oracle_encode_many(miss)))
    return [_enc[k] for k in dlogs]


def pubs_for(n_public):
    return [[sc.draw(b"pub" + bytes(29), 1000 * n_public + 40 * j + i, 9) for i in range(n_public)] for j in range(len(sc.CASES))]


@pytest.fixture(scope="module")
def shared():
    """every case at 0 and at 36 public inputs, index_base 0: case c is proof c"""
    return {k: sc.simulate(TD, pubs_for(k), seed=SEED, cases=sc.CASES, encode_many=encode_many) for k in N_PUBLIC}


@pytest.mark.parametrize("n_public", N_PUBLIC)
def test_every_case_is_accepted_by_the_oracle(shared, n_public):
    for c in shared[n_public]:
        assert c["status"] == sc.OK and len(c["proof"]) == 118
        assert vc.oracle_verdict(TD, c["pub"], c["proof"]), c["case"]


def test_cases_reach_their_exceptional_points(shared):
    by = {c["case"]: c for c in shared[0]}
    assert by[sc.P_ZERO]["p"] == 0 and by[sc.P_ZERO]["proof"][:30] == bytes(30)
    assert by[sc.K_ZERO]["k"] == 0 and by[sc.K_ZERO]["proof"][30:60] == bytes(30)
    assert by[sc.K_PLUS_G]["k"] == 1 and by[sc.K_MINUS_G]["k"] == o.P - 1
    assert by[sc.U0_ZERO]["t"] == 0
    c = by[sc.T_HALF]
    assert 2 * c["t"] % o.P == c["p"] and c["v0"] * c["k"] % o.P == c["t"]  # v0 K == u0 G


def test_draws_are_below_2_230():
    top = 0
    for j in range(300):
        for tag in (1, 2, 3):
            v = sc.draw(SEED, (1 << 63) + j, tag)
            assert 0 <= v < (1 << 230) < o.P
            top = max(top, v)
    assert top >> 225  # and they use the bits up there
    assert sc.draw(SEED, 7, 1) != sc.draw(SEED, 7, 2) != sc.draw(SEED, 8, 2)
    assert sc.draw(SEED, 1 << 64, 1) == sc.draw(SEED, 0, 1)  # the index is a u64


def test_same_key_and_index_give_the_same_bytes(shared):
    """index_base = 5 with j = 0 is index_base = 0 with j = 5, and another key or index is another proof"""
    want = shared[0][5]
    again = sc.simulate(TD, [want["pub"]], seed=SEED, index_base=5, cases=[want["case"]], encode_many=encode_many)[0]
    assert again["proof"] == want["proof"] and (again["p"], again["k"]) == (want["p"], want["k"])
    for other in (dict(seed=SEED, index_base=4), dict(seed=bytes(32), index_base=5), dict(seed=None, index_base=5)):
        assert sc.draw(other["seed"] or sc.default_key(TD), other["index_base"], 1) != want["p"]
    assert sc.default_key(TD) != sc.default_key((TD[0] + 1, TD[1], TD[2]))


def test_b0_with_a_zero_denominator_is_bumped():
    b0 = (-vc.inv(TD[1] * TD[1])) % o.P
    assert (1 + TD[1] * TD[1] * b0) % o.P == 0
    c = sc.simulate(TD, [[3, 4]], seed=SEED, b0=[b0], encode_many=encode_many)[0]
    assert c["b0"] == (b0 + 1) % o.P and int.from_bytes(c["proof"][89:], "little") == c["b0"]
    assert vc.oracle_verdict(TD, c["pub"], c["proof"])
    kept = sc.simulate(TD, [[3, 4]], seed=SEED, b0=[12345], encode_many=encode_many)[0]  # a given b0 is kept: same P, no new encoding of it
    assert kept["b0"] == 12345 and kept["proof"][:30] == c["proof"][:30]


def test_tau_equal_to_alpha_is_v0_zero(shared):
    c = shared[0][0]
    z = sc.simulate((c["alpha"], TD[1], TD[2]), [c["pub"]], seed=SEED, encode_many=encode_many)[0]
    assert z["status"] == sc.V0_ZERO and z["proof"] == bytes(118) and (z["p"], z["k"]) == (0, 0)
