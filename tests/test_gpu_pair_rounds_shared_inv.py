"""GPU parity tests (-m gpu) of the pair rounds' two forms of the field inversion (msm_rounds.cuh: k_affine_round, AFF_SHARE_INV):
one per wave (DVP_MSM_AFF_SHARE_INV=0) or one per workgroup, the waves' running products multiplied up a tree in LDS and the
inverse handed back down (1: whenever the workgroup has more than one wave; 2: in rounds of at least DVP_MSM_AFF_SHARE_MIN
planned additions).  The field inverse is exact, so both forms must return the same bytes; every result is also compared with
the oracle (k233_mulgen of the scalar-log dot product).  The library counts its pair-round launches by form
(dvp_profile_read "rounds_inv_shared" / "rounds_inv_private"), so every case proves which form ran.  The inputs are those of
test_gpu_pair_rounds_dense.py (same seeds); DVP_MSM_AFF_MIN=32 makes the rounds run all the way down at these sizes."""
import ctypes as C

import numpy as np
import pytest

import pyref as o
import c_oracle as co
from util import from_limbs, np_to_pt, rand_fr_np, np_dot_mod
from msm_cases import exceptional_pairs_input

pytestmark = pytest.mark.gpu

N = 6000
SUB_HI = (4000, 4100, 4200, 4300, 4400, 4500, 4600, 4700)


def inv_rounds(dvp):
    """(private, shared) pair-round launches since the last dvp_profile_reset"""
    out = []
    for name in (b"rounds_inv_private", b"rounds_inv_shared"):
        ms, n = C.c_double(0), C.c_uint64(0)
        dvp.check(dvp.lib.dvp_profile_read(name, C.byref(ms), C.byref(n)))
        out.append(int(n.value))
    return tuple(out)


def check_forms(dvp, run, exp, expect_shared, where, **knobs):
    """run() under `knobs` with DVP_MSM_AFF_SHARE_INV 0 and 1: both equal the oracle's point and each other's bytes.  With 0 no
    launch is shared; with 1 all are (expect_shared) or none is (a workgroup of one wave)"""
    got = []
    for share in (0, 1):
        dvp.lib.dvp_profile_reset()
        with dvp.tune(DVP_MSM_AFF_SHARE_INV=share, **knobs):
            xy, is_inf = run()
        assert np_to_pt(xy, is_inf) == exp, (share, where, knobs)
        got.append((xy.tobytes(), is_inf))
        n_private, n_shared = inv_rounds(dvp)
        if share == 1 and expect_shared:
            assert n_shared > 0 and n_private == 0, (share, where, knobs, n_private, n_shared)
        else:
            assert n_private > 0 and n_shared == 0, (share, where, knobs, n_private, n_shared)
    assert got[0] == got[1], (where, knobs)


@pytest.fixture(scope="module")
def random_input(dvp):
    k, s = rand_fr_np(N, 9101), rand_fr_np(N, 9102)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    ks, ss = from_limbs(k), from_limbs(s)
    prod = [a * b for a, b in zip(ss, ks)]
    ranges = [(0, N)] + [(7, hi) for hi in SUB_HI]
    exp = {(lo, hi): co.k233_mulgen(sum(prod[lo:hi]) % o.P) for lo, hi in ranges}
    return bases, s, exp


@pytest.fixture(scope="module", params=[8, 11])
def random_fb(dvp, random_input, request):
    with dvp.tune(DVP_MSM_FIXED_C=request.param):
        fb = dvp.curve.FixedBaseMsm(random_input[0])
    yield fb
    fb.close()


@pytest.mark.parametrize("tpb", [64, 128, 256])
def test_random_rounds_to_the_bottom(dvp, random_input, random_fb, tpb):
    """6 000 random scalars and bases, fixed-base, windows of 8 and 11 bits, 1 / 3 / 64 slots per thread at most, workgroups of one,
    two and four waves: one wave keeps its private inversion whatever the knob says, two and four share"""
    _, s, exp = random_input
    for bmax in (1, 3, 64):
        check_forms(dvp, lambda: random_fb.run(s, 0, N), exp[(0, N)], tpb != 64, (0, N),
                    DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1, DVP_MSM_AFF_BMAX=bmax, DVP_MSM_AFF_TPB=tpb)


@pytest.mark.parametrize("tpb", [128, 256])
def test_sub_ranges_partly_filled_last_workgroup(dvp, random_input, random_fb, tpb):
    """the sub-ranges (7, hi): the thread count of a round changes with hi, so the last live workgroup meets partly filled waves and
    whole waves at or beyond the round's last thread -- they stay for the barriers, with a product of one and no slot"""
    _, s, exp = random_input
    for hi in SUB_HI:
        for bmax in (1, 3, 64):
            check_forms(dvp, lambda: random_fb.run(s[7:hi], 7, hi), exp[(7, hi)], True, (7, hi),
                        DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1, DVP_MSM_AFF_BMAX=bmax, DVP_MSM_AFF_TPB=tpb)


def test_dense_order(dvp, random_input, random_fb):
    """DVP_MSM_ROUND_DENSE=1: the waves whose lanes all hold leftovers skip pass 1's product and post a one to the exchange"""
    _, s, exp = random_input
    for bmax in (1, 3, 64):
        check_forms(dvp, lambda: random_fb.run(s, 0, N), exp[(0, N)], True, "dense",
                    DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1, DVP_MSM_AFF_BMAX=bmax, DVP_MSM_ROUND_DENSE=1)


def test_auto_keeps_small_rounds_private(dvp, random_input, random_fb):
    """DVP_MSM_AFF_SHARE_INV=2 at the default workgroup and slot counts: every round of 6 000 points plans far fewer additions than
    one chip-full at DVP_MSM_AFF_BMIN slots per thread, so all stay private; with the threshold at one addition all share"""
    _, s, exp = random_input
    got = []
    for share_min, want_shared in ((0, False), (1, True)):
        dvp.lib.dvp_profile_reset()
        with dvp.tune(DVP_MSM_AFF_SHARE_INV=2, DVP_MSM_AFF_SHARE_MIN=share_min, DVP_MSM_AFF_MIN=32):
            xy, is_inf = random_fb.run(s, 0, N)
        assert np_to_pt(xy, is_inf) == exp[(0, N)], share_min
        got.append((xy.tobytes(), is_inf))
        n_private, n_shared = inv_rounds(dvp)
        assert (n_shared > 0 and n_private == 0) if want_shared else (n_private > 0 and n_shared == 0), (share_min, n_private, n_shared)
    assert got[0] == got[1]


@pytest.fixture(scope="module")
def exceptional_input():
    bases, s, _, _, exp = exceptional_pairs_input()  # the input of test_gpu_msm.test_bucket_reduction_exceptional_pairs
    return bases, s, exp


@pytest.mark.parametrize("c", [8, 11])
def test_exceptional_pairs(dvp, exceptional_input, c):
    """doublings, P - P and the infinity markers earlier rounds made of them, under all three placements of the bookkeeping"""
    bases, s, exp = exceptional_input
    with dvp.tune(DVP_MSM_FIXED_C=c):
        fb = dvp.curve.FixedBaseMsm(bases)
    try:
        for pipeline in (0, 1, 2):
            check_forms(dvp, lambda: fb.run(s), exp, True, "exceptional", DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_PIPELINE=pipeline)
    finally:
        fb.close()


@pytest.mark.parametrize("c", [8, 11])
def test_degenerate_leftover_patterns(dvp, c):
    """three bases with one common scalar, one base alone (its rounds pass single entries through), 5 and 7 equal scalars, 400 triples: rounds of a
    handful of slots, where one workgroup holds three waves of threads beyond the last one"""
    cases = [(rand_fr_np(3, 9201), np.repeat(rand_fr_np(1, 9202), 3, axis=0)), (rand_fr_np(1, 9203), rand_fr_np(1, 9204))]
    for m in (5, 7):
        cases.append((rand_fr_np(m, 9205 + m), np.repeat(rand_fr_np(1, 9215 + m), m, axis=0)))
    cases.append((rand_fr_np(1200, 9230), np.repeat(rand_fr_np(400, 9231), 3, axis=0)))
    for k, s in cases:
        bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
        assert not inf.any()
        exp = co.k233_mulgen(np_dot_mod(s, k))
        with dvp.tune(DVP_MSM_FIXED_C=c):
            fb = dvp.curve.FixedBaseMsm(bases)
        try:
            for bmax in (1, 3, 64):
                check_forms(dvp, lambda: fb.run(s), exp, True, k.shape[0],
                            DVP_MSM_AFF_MIN=1, DVP_MSM_AFF_BMIN=1, DVP_MSM_AFF_BMAX=bmax)
        finally:
            fb.close()


def test_one_shot_path(dvp):
    """a one-shot MSM on device pointers (dvp_msm_affine_dev, 3 000 points), windows of 8 and 11 bits"""
    import torch

    n = 3000
    k, s = rand_fr_np(n, 9301), rand_fr_np(n, 9302)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    exp = co.k233_mulgen(np_dot_mod(s, k))
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(s.view(np.int64)).to(dev)
    d_b = torch.from_numpy(np.ascontiguousarray(bases).view(np.int64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        d_out = torch.zeros(10, dtype=torch.int64, device=dev)
        dvp.curve.multi_scalar_mul_dev(d_s.data_ptr(), d_b.data_ptr(), None, n, d_out.data_ptr(), d_out.data_ptr() + 64, stream)
        torch.cuda.synchronize()
        h = d_out.cpu().numpy().view(np.uint64)
        return h[:8].copy(), bool(h[8] & np.uint64(0xFFFFFFFF))

    for c in (8, 11):
        check_forms(dvp, run, exp, True, ("one-shot", c), DVP_MSM_C=c, DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1)
