"""GPU tests (-m gpu) of the pair rounds' rare slots (msm_rounds.cuh: k_affine_round, "RARE slots"): a pair whose addition is not the
chord formula -- an operand is infinity, a doubling, P - P -- is only detected by the straight-line code of the two slot loops and
handled behind wave-uniform branches.  The inputs here are made of such pairs: all of them (eight points and their negatives), a few
dozen planted among 6 000 random ones, and ranges whose sum is the neutral element.  Every expected point comes from the oracle
(k233_mulgen of the scalar-log dot product), and the returned bytes must be the same under every setting of the knobs that decide
how a round's slots are laid over threads, waves and workgroups: DVP_MSM_AFF_TPB 64 / 128 / 256, DVP_MSM_AFF_BMAX 1 / 3 / 64,
DVP_MSM_AFF_SHARE_INV 0 / 1, DVP_MSM_ROUND_DENSE 0 / 1, windows of 8 and 11 bits.  DVP_MSM_AFF_MIN=32 makes the rounds run to the
bottom; the library's launch counters (dvp_profile_read) say which form of the inversion and of the descriptors ran."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pyref as o
import c_oracle as co
from util import from_limbs, to_limbs, np_to_pt, rand_fr_np
from msm_cases import exceptional_pairs_input

pytestmark = pytest.mark.gpu

N = 6000
GRID = list(itertools.product((1, 3, 64), (0, 1), (0, 1)))  # DVP_MSM_AFF_BMAX, DVP_MSM_AFF_SHARE_INV, DVP_MSM_ROUND_DENSE


def counter(dvp, name):
    ms, n = C.c_double(0), C.c_uint64(0)
    dvp.check(dvp.lib.dvp_profile_read(name, C.byref(ms), C.byref(n)))
    return int(n.value)


def check_grid(dvp, run, exp, tpb, where, dense_runs=True):
    """run() under every (bmax, share, dense) of GRID at workgroups of `tpb` threads: each result is the oracle's point, all have the
    same bytes, and the counters show the form that was asked for (one wave per workgroup keeps its private inversion; dense_runs:
    whether the input gets the all-rounds bookkeeping the dense order needs, None: either)"""
    got = set()
    for bmax, share, dense in GRID:
        dvp.lib.dvp_profile_reset()
        with dvp.tune(DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1, DVP_MSM_AFF_BMAX=bmax, DVP_MSM_AFF_TPB=tpb, DVP_MSM_AFF_SHARE_INV=share,
                      DVP_MSM_ROUND_DENSE=dense):
            xy, is_inf = run()
        at = (where, tpb, bmax, share, dense)
        assert np_to_pt(xy, is_inf) == exp, at
        got.add((b"" if is_inf else np.asarray(xy).tobytes(), bool(is_inf)))  # (the coordinates of an infinite result mean nothing)
        n_private, n_shared = counter(dvp, b"rounds_inv_private"), counter(dvp, b"rounds_inv_shared")
        if share and tpb > 64:
            assert n_shared > 0 and n_private == 0, (at, n_private, n_shared)
        else:
            assert n_private > 0 and n_shared == 0, (at, n_private, n_shared)
        n_word, n_dense = counter(dvp, b"later_rounds_word"), counter(dvp, b"later_rounds_dense")
        if dense and dense_runs:
            assert n_dense > 0 and n_word == 0, (at, n_word, n_dense)
        elif not dense or dense_runs is not None:
            assert n_dense == 0, (at, n_word, n_dense)
    assert len(got) == 1, where


@pytest.fixture(scope="module")
def all_rare_input():
    bases, s, _, _, exp = exceptional_pairs_input(4096)
    return bases, s, exp


def negated(points):
    """-(x, y) = (x, x + y) on [n, 8] uint64 rows"""
    out = points.copy()
    out[:, 4:] ^= out[:, :4]
    return out


@pytest.fixture(scope="module")
def mixed_input(dvp):
    """6 000 random bases and scalars (the seeds of test_gpu_pair_rounds_shared_inv.py) with 48 planted neighbours (i, i + 1): base
    i + 1 is base i again or its negative, scalar i + 1 is scalar i again or its negative.  Equal scalars put the two into the same
    bucket of every window, next to each other in the sorted order, so wherever they fall on one slot the first round meets a
    doubling or P - P, and the infinity P - P leaves is an operand of the round after.  The neighbours sit at the start, in the
    middle and at the very end of the index range: the last two indices close whichever bucket they fall into."""
    k, s = rand_fr_np(N, 9101), rand_fr_np(N, 9102)
    ks, ss = from_limbs(k), from_limbs(s)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    bases = np.ascontiguousarray(bases).copy()
    spots = list(range(0, 32, 2)) + list(range(3001, 3033, 2)) + list(range(N - 32, N, 2))
    for j, i in enumerate(spots):
        neg_base, neg_scalar = bool(j & 1), bool(j & 2)
        bases[i + 1] = negated(bases[i:i + 1])[0] if neg_base else bases[i]
        ks[i + 1] = (o.P - ks[i]) if neg_base else ks[i]
        ss[i + 1] = (o.P - ss[i]) % o.P if neg_scalar else ss[i]
    exp = co.k233_mulgen(sum(a * b for a, b in zip(ss, ks)) % o.P)
    return bases, to_limbs(ss), exp


@pytest.fixture(scope="module")
def neutral_input(dvp):
    """512 bases, every even one followed by its negative under the same scalar: any range [2 i, 2 j) sums to the neutral element"""
    n = 512
    k, s = rand_fr_np(n // 2, 9501), rand_fr_np(n // 2, 9502)
    half, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    half = np.ascontiguousarray(half)
    bases = np.empty((n, 8), dtype=np.uint64)
    bases[0::2] = half
    bases[1::2] = negated(half)
    return bases, np.repeat(s, 2, axis=0)


def fixed_base(dvp, bases, c):
    with dvp.tune(DVP_MSM_FIXED_C=c):
        return dvp.curve.FixedBaseMsm(bases)


@pytest.mark.parametrize("tpb", [64, 128, 256])
@pytest.mark.parametrize("c", [8, 11])
def test_all_rare(dvp, all_rare_input, c, tpb):
    """eight points and their negatives under five scalars: nearly every pair of every round is a doubling, P - P or has an infinity
    for an operand, so whole threads and waves hold nothing but rare slots"""
    bases, s, exp = all_rare_input
    fb = fixed_base(dvp, bases, c)
    try:
        check_grid(dvp, lambda: fb.run(s), exp, tpb, ("all rare", c))
    finally:
        fb.close()


@pytest.mark.parametrize("tpb", [64, 128, 256])
@pytest.mark.parametrize("c", [8, 11])
def test_mixed(dvp, mixed_input, c, tpb):
    """rare slots beside generic pairs and leftovers in one wave"""
    bases, s, exp = mixed_input
    fb = fixed_base(dvp, bases, c)
    try:
        check_grid(dvp, lambda: fb.run(s, 0, N), exp, tpb, ("mixed", c))
    finally:
        fb.close()


@pytest.mark.parametrize("c", [8, 11])
def test_one_shot_path(dvp, all_rare_input, c):
    """dvp_msm_affine_dev (no sign mask: the operands are the bases themselves) on the all-rare input: its single pair round per
    bucket set takes the same kernel"""
    import torch

    bases, s, exp = all_rare_input
    n = s.shape[0]
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(s.view(np.int64)).to(dev)
    d_b = torch.from_numpy(np.ascontiguousarray(bases).view(np.int64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    got = set()
    for share in (0, 1):
        d_out = torch.zeros(10, dtype=torch.int64, device=dev)
        dvp.lib.dvp_profile_reset()
        with dvp.tune(DVP_MSM_C=c, DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1, DVP_MSM_AFF_SHARE_INV=share):
            dvp.curve.multi_scalar_mul_dev(d_s.data_ptr(), d_b.data_ptr(), None, n, d_out.data_ptr(), d_out.data_ptr() + 64, stream)
            torch.cuda.synchronize()
        h = d_out.cpu().numpy().view(np.uint64)
        is_inf = bool(h[8] & np.uint64(0xFFFFFFFF))
        assert np_to_pt(h[:8], is_inf) == exp, (c, share)
        assert counter(dvp, b"rounds_inv_shared" if share else b"rounds_inv_private") > 0, (c, share)
        got.add((h[:8].tobytes(), is_inf))
    assert len(got) == 1, c


@pytest.mark.parametrize("c", [8, 11])
def test_neutral_sub_range(dvp, neutral_input, c):
    """ranges made of (P, -P) neighbours under equal scalars: every bucket empties into infinity markers, which the later rounds add
    to each other; the result is the neutral element"""
    bases, s = neutral_input
    fb = fixed_base(dvp, bases, c)
    try:
        for lo, hi in ((0, 512), (64, 320), (2, 500)):
            for tpb in (64, 256):
                check_grid(dvp, lambda: fb.run(s[lo:hi], lo, hi), None, tpb, ("neutral", c, lo, hi), dense_runs=None)
    finally:
        fb.close()
