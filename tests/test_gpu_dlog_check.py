"""GPU tests (-m gpu) of dvp_points_check_dlog: "are these points the given multiples of G?" by one combined MSM, and the
entry-for-entry comparison that names the first wrong index (csrc/srs_check.hip; the derivation restated in dlog_check_cases.py).

Lengths: 1, 2, 255, 256, 257 (lanes and blocks of the coefficient kernel), one more than a full first level of the block sums (every
lane of every block has one element and lane 0 of block 0 a second; the constants are read from csrc/fr_block.cuh), and 2^20 + 1, which
needs two batches of the comparison (that one only under `exact`, with the wrong entry in the second batch)."""
import numpy as np
import pytest

import dlog_check_cases as dc
import msm_cases as mc
import point_cases as pc
import pyref as o
from util import to_limbs, from_limbs, rand_fr_np

pytestmark = pytest.mark.gpu

LANES, BLOCKS = dc.fr_sum_constants()
LENGTHS = list(dc.BLOCK_LENGTHS) + [LANES * BLOCKS + 1]
SEEDS = [bytes(32), bytes(range(32)), bytes(255 - i for i in range(32))]
PREP, DIFF = "srs_check.hip:k_dlog_rlc_prep", "srs_check.hip:k_points_first_diff"
EINVAL = -1


def modes():
    """(seed, exact) of every way to ask"""
    return [(None, False)] + [(s, False) for s in SEEDS] + [(None, True)]


@pytest.fixture(scope="module")
def vectors(dvp):
    """n -> (scalars [n, 4], points [n, 8]) of random canonical non-zero scalars; made once per length"""
    made = {}

    def get(n):
        if n not in made:
            s = rand_fr_np(n, 7000 + n % 1000)
            s[:, 0] |= np.uint64(1)
            xy, inf = dvp.curve.point_scalar_mul_gen_batch(s)
            assert not inf.any()
            made[n] = (s, xy)
        return made[n]

    return get


@pytest.fixture(scope="module")
def bad_points():
    """one recorded point of every class of dvp_points_check that is not 0: [(class, xy [8])]"""
    out = {}
    for c in pc.load():
        if c["cls"] and not c["inf"] and c["cls"] not in out:
            out[c["cls"]] = pc.arrays([c])[0][0]
    assert sorted(out) == [pc.UNREDUCED, pc.OFF_CURVE, pc.ORDER4, pc.COSET_N]
    return sorted(out.items())


def mulgen(dvp, ints):
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(to_limbs(ints))
    assert not inf.any()
    return xy


def expect(dvp, rep, exact, wrong_at=None):
    """the report of a well-formed vector: right, or wrong with its first index"""
    C = dvp.curve
    if wrong_at is None:
        assert (rep.verdict, rep.first_bad, rep.point_class) == (0, None, 0), rep
        assert rep.path == (C.DLOG_PATH_EXACT if exact else C.DLOG_PATH_COMBINED), rep
    else:
        assert (rep.verdict, rep.first_bad, rep.point_class) == (C.DLOG_WRONG, wrong_at, 0), rep
        assert rep.path == (C.DLOG_PATH_EXACT if exact else C.DLOG_PATH_LOCATED), rep


@pytest.mark.parametrize("n", LENGTHS)
def test_right_vector_and_path(dvp, vectors, n):
    s, xy = vectors(n)
    for seed, exact in modes():
        dvp.lib.dvp_profile_reset()
        expect(dvp, dvp.curve.check_dlogs(s, xy, seed=seed, exact=exact), exact)
        if exact:  # no coefficient is computed, every point is compared
            mc.assert_census(dvp, [DIFF], [PREP, "msm.hip:k_tail*"], n)
        else:  # the combined check alone
            mc.assert_census(dvp, [PREP, "srs_check.hip:k_dlog_rlc_final", "srs_check.hip:k_dlog_key", "msm.hip:k_tail*"], [DIFF, "codec.hip:k_mulgen"], n)
    # an all-zero infinity mask is no mask
    expect(dvp, dvp.curve.check_dlogs(s, xy, np.zeros(n, dtype=np.uint8)), False)


@pytest.mark.parametrize("n", LENGTHS)
def test_zero_scalars_and_points_at_infinity(dvp, vectors, n):
    s0, xy = vectors(n)
    i = n // 2
    s = s0.copy()
    s[i] = 0
    inf = np.zeros(n, dtype=np.uint8)
    inf[i] = 1
    for seed, exact in modes():
        expect(dvp, dvp.curve.check_dlogs(s, xy, inf, seed=seed, exact=exact), exact)              # s_i = 0 and O: right
        expect(dvp, dvp.curve.check_dlogs(s, xy, None, seed=seed, exact=exact), exact, i)          # s_i = 0 and a finite point
        expect(dvp, dvp.curve.check_dlogs(s0, xy, inf, seed=seed, exact=exact), exact, i)          # s_i != 0 and O
    inf[i] = 255  # any non-zero flag means O
    expect(dvp, dvp.curve.check_dlogs(s, xy, inf), False)


@pytest.mark.parametrize("n", LENGTHS)
def test_wrong_entries_are_located(dvp, vectors, n):
    s, xy0 = vectors(n)
    for name, delta, first in dc.tampers(n, n):
        xy = xy0.copy()
        idx = sorted(delta)
        xy[idx] = mulgen(dvp, [(k + delta[i]) % o.P for i, k in zip(idx, from_limbs(s[idx]))])
        for seed, exact in modes():
            dvp.lib.dvp_profile_reset()
            expect(dvp, dvp.curve.check_dlogs(s, xy, seed=seed, exact=exact), exact, first)
            mc.assert_census(dvp, [DIFF, "codec.hip:k_mulgen"] + ([] if exact else [PREP]), [PREP] if exact else [], (n, name))


def test_wrong_entry_in_the_second_locate_batch(dvp, vectors):
    n = (1 << 20) + 1
    s, xy0 = vectors(n)
    expect(dvp, dvp.curve.check_dlogs(s, xy0, exact=True), True)
    xy = xy0.copy()
    xy[n - 1] = mulgen(dvp, [(from_limbs(s[n - 1:])[0] + 1) % o.P])[0]
    dvp.lib.dvp_profile_reset()
    expect(dvp, dvp.curve.check_dlogs(s, xy, exact=True), True, n - 1)
    assert mc.launches(dvp, DIFF) == 2 and mc.launches(dvp, PREP) == 0


@pytest.mark.parametrize("n", LENGTHS)
def test_bad_points_end_the_check_before_any_msm(dvp, vectors, bad_points, n):
    s, xy0 = vectors(n)
    expect(dvp, dvp.curve.check_dlogs(s, xy0), False)  # the process's one-time tables exist from here on
    for j, (cls, pt) in enumerate(bad_points):
        i = (n - 1) * j // 3
        xy = xy0.copy()
        xy[i] = pt
        for seed, exact in modes():
            dvp.lib.dvp_profile_reset()
            rep = dvp.curve.check_dlogs(s, xy, seed=seed, exact=exact)
            assert (rep.verdict, rep.first_bad, rep.point_class) == (dvp.curve.DLOG_BAD_POINT, i, cls), (rep, pc.CLASS_NAMES[cls])
            mc.assert_census(dvp, ["codec.hip:k_points_check"], ["msm.hip:*", "srs_check.hip:*", "codec.hip:k_mulgen"], (n, cls))
        # with its infinity flag set the same coordinates are no point at all: the entry is O, wrong for s_i != 0
        inf = np.zeros(n, dtype=np.uint8)
        inf[i] = 1
        expect(dvp, dvp.curve.check_dlogs(s, xy, inf), False, i)
    if n >= 2:  # two bad points: the smaller index, with its class
        xy = xy0.copy()
        xy[0], xy[n - 1] = bad_points[1][1], bad_points[0][1]
        rep = dvp.curve.check_dlogs(s, xy)
        assert (rep.verdict, rep.first_bad, rep.point_class) == (dvp.curve.DLOG_BAD_POINT, 0, bad_points[1][0])


@pytest.mark.parametrize("n", LENGTHS)
def test_non_canonical_scalar(dvp, vectors, n):
    s0, xy = vectors(n)
    for i in sorted({0, n - 1}):
        for val in (o.P, (1 << 256) - 1):
            s = s0.copy()
            s[i] = to_limbs([val])[0]
            for exact in (False, True):
                with pytest.raises(dvp.DvpError) as e:
                    dvp.curve.check_dlogs(s, xy, exact=exact)
                assert (e.value.status, e.value.index) == (EINVAL, i)


def test_empty_vector_and_bad_arguments(dvp, nat):
    rep = dvp.curve.check_dlogs(np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 8), dtype=np.uint64))
    assert (rep.verdict, rep.first_bad) == (0, None)
    r = nat.DlogReport()
    import ctypes as C

    one = np.zeros(8, dtype=np.uint64)
    assert dvp.lib.dvp_points_check_dlog(nat.ptr(one), nat.ptr(one), None, 1, None, 2, C.byref(r)) == EINVAL  # an unknown flag
    assert dvp.lib.dvp_points_check_dlog(None, nat.ptr(one), None, 1, None, 0, C.byref(r)) == EINVAL
    assert dvp.lib.dvp_points_check_dlog(nat.ptr(one), nat.ptr(one), None, 1, None, 0, None) == EINVAL
    with pytest.raises(ValueError):
        dvp.curve.check_dlogs(one[:4], one, seed=b"short")


@pytest.mark.parametrize("n", [257, LANES * BLOCKS + 1])
def test_device_form_with_the_callers_workspace(dvp, vectors, n):
    import torch

    s, xy0 = vectors(n)
    xy = xy0.copy()
    bad = n - 2
    xy[bad] = mulgen(dvp, [(from_limbs(s[bad:bad + 1])[0] + 1) % o.P])[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()
    d_s, d_good, d_bad = up(s), up(xy0), up(xy)
    inf = np.zeros(n, dtype=np.uint8)
    d_inf = up(inf)
    wb = dvp.curve.check_dlogs_work_bytes(n)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    st = torch.cuda.current_stream().cuda_stream
    run = lambda pts, d_i=0, **kw: dvp.curve.check_dlogs_dev(d_s.data_ptr(), pts.data_ptr(), d_i, n, work.data_ptr(), wb, stream=st, **kw)
    for seed, exact in modes():
        assert run(d_good, seed=seed, exact=exact) == dvp.curve.check_dlogs(s, xy0, seed=seed, exact=exact)
        assert run(d_good, d_inf.data_ptr(), seed=seed, exact=exact) == dvp.curve.check_dlogs(s, xy0, inf, seed=seed, exact=exact)
        rep = run(d_bad, seed=seed, exact=exact)
        assert rep == dvp.curve.check_dlogs(s, xy, seed=seed, exact=exact)
        expect(dvp, rep, exact, bad)
    # what held the coefficients' products is zero again: the first 32 (n + 1) bytes of the workspace are the MSM scalars
    torch.cuda.synchronize()
    assert not work[: 32 * (n + 1)].any().item()
    with pytest.raises(dvp.DvpError) as e:  # one byte less
        dvp.curve.check_dlogs_dev(d_s.data_ptr(), d_good.data_ptr(), 0, n, work.data_ptr(), wb - 1, stream=st)
    assert e.value.status == EINVAL
    # a scalar that is not below p, found on the device by either path
    s_bad = s.copy()
    s_bad[n - 1] = to_limbs([o.P])[0]
    d_sb = up(s_bad)
    for exact in (False, True):
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.check_dlogs_dev(d_sb.data_ptr(), d_good.data_ptr(), 0, n, work.data_ptr(), wb, exact=exact, stream=st)
        assert (e.value.status, e.value.index) == (EINVAL, n - 1)
