"""GPU parity tests (-m gpu) of the pair rounds' two forms (msm_rounds.cuh: k_affine_round, k_round_desc_all):
  * the numerator multiplied into the prefix in pass 1 (AFF_NUM1, compiled in): every result below goes through it;
  * the later rounds in dense order (DVP_MSM_ROUND_DENSE, default 0): a round's additions in slots [0, A), its odd leftovers behind
    them, two descriptor words per slot -- only with the all-rounds bookkeeping (DVP_MSM_ROUND_PIPELINE 1 / 2, and then only when
    the MSM has at least four entries per bucket and two rounds planned); the per-round bookkeeping keeps one word per slot.
Every result is compared with the oracle (k233_mulgen of the scalar-log dot product), and where the knob is switched the returned
xy / inf are compared byte for byte between DVP_MSM_ROUND_DENSE = 0 and 1.  DVP_MSM_AFF_MIN=32 makes the rounds run all the way
down at these sizes, so the bucket counts pass through every parity."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as o
import c_oracle as co
from util import to_limbs, from_limbs, pts_to_np, np_to_pt, rand_fr_np, np_dot_mod
from msm_cases import exceptional_pairs_input

pytestmark = pytest.mark.gpu


def later_rounds(dvp):
    """(one-word, dense) launches of the rounds after the first since the last dvp_profile_reset"""
    out = []
    for name in (b"later_rounds_word", b"later_rounds_dense"):
        ms, n = C.c_double(0), C.c_uint64(0)
        dvp.check(dvp.lib.dvp_profile_read(name, C.byref(ms), C.byref(n)))
        out.append(int(n.value))
    return tuple(out)


def run_both(dvp, fb, s, exp, lo=0, hi=None, expect_dense=None, **knobs):
    """fb.run under `knobs` with the dense order off and on: both equal the oracle's point and each other's bytes.  The library
    counts the later rounds it launches by descriptor form: with the knob off none is dense; with it on all are (expect_dense =
    True: and there is at least one), or none is (expect_dense = False: an input or a setting that keeps the per-round bookkeeping)"""
    got = []
    for dense in (0, 1):
        dvp.lib.dvp_profile_reset()
        with dvp.tune(DVP_MSM_ROUND_DENSE=dense, **knobs):
            xy, is_inf = fb.run(s, lo, hi)
        assert np_to_pt(xy, is_inf) == exp, (dense, knobs, lo, hi)
        got.append((xy.tobytes(), is_inf))
        n_word, n_dense = later_rounds(dvp)
        if dense == 0 or expect_dense is False:
            assert n_dense == 0, (dense, knobs, n_word, n_dense)
        elif expect_dense:
            assert n_dense > 0 and n_word == 0, (dense, knobs, n_word, n_dense)
    assert got[0] == got[1], (knobs, lo, hi)


@pytest.fixture(scope="module")
def random_input(dvp):
    n = 6000
    k, s = rand_fr_np(n, 9101), rand_fr_np(n, 9102)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    ks, ss = from_limbs(k), from_limbs(s)
    exp = {(lo, hi): co.k233_mulgen(sum(a * b for a, b in zip(ss[lo:hi], ks[lo:hi])) % o.P) for lo, hi in ((0, n), (7, 4000))}
    return bases, s, exp


@pytest.mark.parametrize("c", [8, 11])
def test_random_rounds_to_the_bottom(dvp, random_input, c):
    """6 000 random scalars and bases, fixed-base, window 8 (128 buckets of ~1 400 entries: eleven rounds) and 11 (1 024 buckets of
    ~130: eight rounds); 1, 3 and 64 slots per thread at most, so a thread's rows are all additions, mixed, or all leftovers"""
    bases, s, exp = random_input
    with dvp.tune(DVP_MSM_FIXED_C=c):
        fb = dvp.curve.FixedBaseMsm(bases)
    try:
        for bmax in (1, 3, 64):
            for lo, hi in exp:
                run_both(dvp, fb, s[lo:hi], exp[(lo, hi)], lo, hi, expect_dense=True, DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMAX=bmax, DVP_MSM_AFF_BMIN=1)
    finally:
        fb.close()


def _triples(n_groups, seed):
    """n_groups x 3 bases, the three of a group under one common scalar"""
    k = rand_fr_np(3 * n_groups, seed)
    s = np.repeat(rand_fr_np(n_groups, seed + 1), 3, axis=0)
    return k, s


@pytest.mark.parametrize("c", [8, 11])
def test_degenerate_leftover_patterns(dvp, c):
    """three bases with one common scalar (every bucket holds 3, then 2 points: a round of one pair plus one leftover per bucket),
    one base alone (nothing to add anywhere), 5 and 7 equal scalars.  These inputs hold fewer than four entries per bucket, so
    msm_core gives them the per-round bookkeeping whatever the knob says (and the lone base no round at all); 400 such triples at
    once (buckets of 3, 6, .. points: a leftover in every bucket of every other round) take the pattern through the dense order."""
    rounds = dict(DVP_MSM_AFF_MIN=1, DVP_MSM_AFF_BMIN=1)
    cases = []
    k3 = rand_fr_np(3, 9201)
    cases.append((k3, np.repeat(rand_fr_np(1, 9202), 3, axis=0)))
    cases.append((rand_fr_np(1, 9203), rand_fr_np(1, 9204)))
    for m in (5, 7):
        cases.append((rand_fr_np(m, 9205 + m), np.repeat(rand_fr_np(1, 9215 + m), m, axis=0)))
    cases.append(_triples(400, 9230))
    for k, s in cases:
        big = k.shape[0] >= 1200  # only the 400 triples hold four entries per bucket
        bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
        assert not inf.any()
        exp = co.k233_mulgen(np_dot_mod(s, k))
        with dvp.tune(DVP_MSM_FIXED_C=c):
            fb = dvp.curve.FixedBaseMsm(bases)
        try:
            for bmax in (1, 3, 64):
                run_both(dvp, fb, s, exp, expect_dense=big, DVP_MSM_AFF_BMAX=bmax, **rounds)
        finally:
            fb.close()


@pytest.fixture(scope="module")
def exceptional_input():
    bases, s, _, _, exp = exceptional_pairs_input()  # the input of test_gpu_msm.test_bucket_reduction_exceptional_pairs
    return bases, s, exp


@pytest.mark.parametrize("c", [8, 11])
def test_exceptional_pairs(dvp, exceptional_input, c):
    """doublings, P - P and the infinity markers earlier rounds made of them, as pair operands and as leftovers, with the rounds
    stopped early (4 096) and run to the bottom (32), under all three placements of the bookkeeping (0: per round, one-word
    descriptors whatever DVP_MSM_ROUND_DENSE says)"""
    bases, s, exp = exceptional_input
    with dvp.tune(DVP_MSM_FIXED_C=c):
        fb = dvp.curve.FixedBaseMsm(bases)
    try:
        for aff_min in (32, 4096):
            for pipeline in (0, 1, 2):
                run_both(dvp, fb, s, exp, expect_dense=pipeline != 0, DVP_MSM_AFF_MIN=aff_min, DVP_MSM_ROUND_PIPELINE=pipeline)
    finally:
        fb.close()


def test_one_shot_path(dvp):
    """a one-shot MSM on device pointers (dvp_msm_affine_dev, 3 000 points) under the same knobs: per-window bucket sets; with c = 11
    they hold fewer than four entries per bucket and the rounds keep the per-round bookkeeping and its one-word descriptors"""
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
    for c in (8, 11):
        got = []
        for dense in (0, 1):
            d_out = torch.zeros(10, dtype=torch.int64, device=dev)
            dvp.lib.dvp_profile_reset()
            with dvp.tune(DVP_MSM_C=c, DVP_MSM_AFF_MIN=32, DVP_MSM_AFF_BMIN=1, DVP_MSM_ROUND_DENSE=dense):
                dvp.curve.multi_scalar_mul_dev(d_s.data_ptr(), d_b.data_ptr(), None, n, d_out.data_ptr(), d_out.data_ptr() + 64, stream)
                torch.cuda.synchronize()
            h = d_out.cpu().numpy().view(np.uint64)
            is_inf = bool(h[8] & np.uint64(0xFFFFFFFF))
            assert np_to_pt(h[:8], is_inf) == exp, (c, dense)
            n_word, n_dense = later_rounds(dvp)
            assert n_word + n_dense > 0 and (n_dense > 0) == (dense == 1 and c == 8), (c, dense, n_word, n_dense)
            got.append((h[:8].tobytes(), is_inf))
        assert got[0] == got[1], c
