"""CPU: the coefficient derivation and the combined check of dvp_points_check_dlog on discrete logs (tests/dlog_check_cases.py)."""
import ctypes as C
import random

import pytest

import c_oracle as co
import dlog_check_cases as dc
import pyref as o
from util import pts_to_np


def vector(n, seed):
    rnd = random.Random(seed)
    s = [rnd.randrange(1, o.P) for _ in range(n)]
    return s, pts_to_np([co.k233_mulgen(k) for k in s])


def test_coefficients_follow_the_derivation():
    s, xy = vector(3, 1)
    h = dc.points_hash(xy)
    assert h == o.blake3(xy.tobytes() + bytes(3)) == dc.points_hash(xy, [0, 0, 0])
    assert dc.points_hash(xy, [0, 1, 0]) != h
    r = dc.coefficients(h, 3)
    k = o.blake3(o.blake3(b"dv-pari dlog check v1") + h)
    assert r[2] == int.from_bytes(o.blake3(k + (2).to_bytes(8, "little"))[:16], "little") | (1 << 127)
    assert all((1 << 127) <= x < (1 << 128) for x in r) and len(set(r)) == 3
    seeded = dc.coefficients(h, 3, seed=bytes(range(32)))
    assert seeded != r and seeded == dc.coefficients(h, 3, seed=bytes(range(32)))
    # the coefficients are fixed only after the points are: another point, other coefficients at EVERY index
    xy2 = xy.copy()
    xy2[1] = pts_to_np([co.k233_mulgen(s[1] + 1)])[0]
    assert all(a != b for a, b in zip(r, dc.coefficients(dc.points_hash(xy2), 3)))


def test_srs_keys_differ_by_vector_and_trapdoor():
    td = (5, 6, 7)
    keys = {dc.srs_key(td, v) for v in range(5)} | {dc.srs_key((5, 6, 8), 0), dc.srs_key(td, 0, seed=bytes(32))}
    assert len(keys) == 7
    assert dc.srs_key(td, 3) == o.blake3(b"dv-pari srs check v1" + b"".join(x.to_bytes(32, "little") for x in td) + (3).to_bytes(4, "little"))
    assert dc.srs_key(td, 3, seed=bytes(32)) == o.blake3(bytes(32) + (3).to_bytes(4, "little"))


@pytest.mark.parametrize("n", [1, 2, 5, 257])
def test_combined_sum_separates_right_from_tampered(n):
    s, xy = vector(n, 40 + n)
    r = dc.coefficients(dc.points_hash(xy), n)
    assert dc.combined_sum(r, s, s) == 0
    for name, delta, first in dc.tampers(n, n):
        t = dc.apply_tamper(s, delta)
        assert first == min(i for i in range(n) if t[i] != s[i]), name
        # the coefficients belong to the points under test: re-derived from the tampered points where those are cheap to make
        if n <= 5:
            r_t = dc.coefficients(dc.points_hash(pts_to_np([co.k233_mulgen(k) for k in t])), n)
        else:
            r_t = r
        assert dc.combined_sum(r_t, s, t) != 0, name
        if name == "pair":  # what a plain sum of the points would have passed
            assert sum(ti - si for si, ti in zip(s, t)) % o.P == 0


def test_block_sum_constants_are_readable():
    lanes, blocks = dc.fr_sum_constants()
    assert lanes == 256 and blocks >= 1


def test_report_structs_match_the_header(nat):
    """dvp_dlog_report / dvp_srs_check_report as include/dvpari.h lays them out (x86-64 / LP64 C layout)"""
    assert C.sizeof(nat.DlogReport) == 24 and nat.DlogReport.first_bad.offset == 8 and nat.DlogReport.point_class.offset == 16
    assert C.sizeof(nat.SrsCheckReport) == 8 + 20 + 20 + 40 + 40 and nat.SrsCheckReport.first_bad.offset == 48
    for name in ("dvp_points_check_dlog", "dvp_points_check_dlog_dev", "dvp_points_check_dlog_work_bytes", "dvp_srs_check_cache_dir"):
        assert name in nat.EXPORTED, name
    # host arithmetic only: monotone, zero for nothing
    wb = [nat.lib.dvp_points_check_dlog_work_bytes(n) for n in (0, 1, 2, 256, 257, 1 << 20, (1 << 20) + 1)]
    assert wb[0] == 0 < wb[1] and all(a <= b for a, b in zip(wb, wb[1:])) and wb[-1] >= 97 * (1 << 20)
