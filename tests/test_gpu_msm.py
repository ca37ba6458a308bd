"""GPU parity tests (-m gpu): sect233k1 MSM / fixed-base mulgen / codec through the C ABI.
Bit-exact (affine group elements) against the OpenSSL-pinned C oracle; BASELINE config #2
(2^16 points) is checked through the discrete-log identity sum s_i (k_i G) = (sum s_i k_i) G,
exactly the shape of the reference's own test_msm (src/curve.rs:218-232)."""
import json
import os
import random

import numpy as np
import pytest

import pyref as o
import c_oracle as co
from util import to_limbs, from_limbs, pts_to_np, np_to_pt, rand_fr_np, np_dot_mod, np_dot_mod_fast, tau_adversarial_scalars
from msm_cases import exceptional_pairs_input, assert_census, rest_len
from msm_stage_cases import signed_recode

pytestmark = pytest.mark.gpu
OSSL = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "k233_openssl.json")))["vectors"]


def H(s):
    return int(s, 16)


def gpu_msm(dvp, scalars, bases, inf=None):
    xy, is_inf = dvp.curve.multi_scalar_mul(scalars, bases, inf)
    return np_to_pt(xy, is_inf)


def test_mulgen_against_openssl(dvp):
    ks = [H(e["k"]) for e in OSSL]
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(to_limbs(ks + [0]))
    for i, e in enumerate(OSSL):
        assert np_to_pt(xy[i], inf[i]) == (H(e["x"]), H(e["y"]))
    assert inf[-1] == 1  # 0 * G = neutral


def test_msm_edge_cases(dvp):
    g = [co.k233_mulgen(k) for k in (1, 2, 3, 4, 5)]
    G = pts_to_np(g)
    assert gpu_msm(dvp, to_limbs([1]), G[:1]) == g[0]
    assert gpu_msm(dvp, to_limbs([o.P - 1]), G[2:3]) == o.k233_neg(g[2])
    assert gpu_msm(dvp, to_limbs([0, 0, 0]), G[:3]) is None            # all-zero scalars
    assert gpu_msm(dvp, to_limbs([1, o.P - 1]), G[[3, 3]]) is None     # P + (-P)
    assert gpu_msm(dvp, to_limbs([1, 1]), G[[3, 3]]) == co.k233_mulgen(8)  # P + P inside one bucket
    assert gpu_msm(dvp, np.zeros((0, 4), np.uint64), np.zeros((0, 8), np.uint64)) is None  # empty
    inf = np.array([0, 1, 0], dtype=np.uint8)                              # neutral among the bases
    assert gpu_msm(dvp, to_limbs([7, 9, 11]), G[:3], inf) == co.k233_mulgen(7 * 1 + 11 * 3)
    with pytest.raises(dvp.DvpError) as ei:                                 # scalar >= p is rejected
        gpu_msm(dvp, to_limbs([5, o.P]), G[:2])
    assert ei.value.status == -1 and ei.value.index == 1


def test_msm_all_equal_bases_like_reference(dvp):
    """test_msm, src/curve.rs:218-232 (10 000 random scalars on G)."""
    n = 10000
    s = rand_fr_np(n, 11)
    G = np.tile(pts_to_np([o.G_STD]), (n, 1))
    assert gpu_msm(dvp, s, G) == co.k233_mulgen(sum(from_limbs(s)) % o.P)


def test_msm_vs_reference_shaped_cpu(dvp):
    n = 777
    k, s = rand_fr_np(n, 21), rand_fr_np(n, 22)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    assert gpu_msm(dvp, s, bases) == co.msm(s, bases, threads=4)


def test_msm_skewed_scalars(dvp):
    """many equal / tiny scalars: one bucket receives most points (load-balance path of the reduction)."""
    n = 5000
    k = rand_fr_np(n, 31)
    bases, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    s = np.zeros((n, 4), dtype=np.uint64)
    s[:, 0] = 1
    s[::7, 0] = 2
    s[::11, 0] = 0
    assert gpu_msm(dvp, s, bases) == co.k233_mulgen(np_dot_mod(s, k))


@pytest.mark.parametrize("log_n", [12, 16])
def test_msm_config2(dvp, log_n):
    """BASELINE config #2: 2^16 random scalars/bases, bit-exact vs the CPU restatement."""
    n = 1 << log_n
    k, s = rand_fr_np(n, 41 + log_n), rand_fr_np(n, 42 + log_n)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    got = gpu_msm(dvp, s, bases)
    assert got == co.k233_mulgen(np_dot_mod(s, k))
    if log_n == 12:  # and directly against the per-point scalar-mult + add-tree CPU shape
        assert got == co.msm(s, bases, threads=8)


def test_codec_roundtrip_and_invalid(dvp):
    ks = [1, 2, 3, 0xDEADBEEF, o.P - 1] + [random.Random(5).randrange(o.P) for _ in range(20)]
    enc = dvp.curve.point_scalar_mul_gen_batch_bytes(to_limbs(ks + [0]))
    for i, k in enumerate(ks):
        assert enc[i].tobytes() == co.xsk233_encode(co.k233_mulgen(k))
    assert enc[-1].tobytes() == bytes(30)
    xy, inf = dvp.curve.from_bytes(enc)
    for i, k in enumerate(ks):
        assert np_to_pt(xy[i], inf[i]) == co.k233_mulgen(k)
    assert inf[-1] == 1
    assert (dvp.curve.to_bytes(xy, inf) == enc).all()
    rnd = random.Random(6)
    seen_bad = 0
    for _ in range(24):
        w = rnd.getrandbits(233).to_bytes(30, "little")
        exp, ok = co.xsk233_decode(w)
        try:
            x, i_ = dvp.curve.from_bytes(np.frombuffer(w, dtype=np.uint8))
            assert ok and np_to_pt(x[0], i_[0]) == exp
        except dvp.DvpError as e:
            assert not ok and e.status == -2 and e.index == 0
            seen_bad += 1
    assert seen_bad > 0


@pytest.mark.parametrize("rule", range(1, 12))
def test_codec_rule_variants(dvp, rule):
    """dvp_codec_set_rule: every presentation of the encoded element that tools/pin_xsk233.py can name (w / w^2 / sqrt w,
    "+1", byte order) -- GPU encode == the oracle's own formula for that rule, GPU decode inverts it, invalid bytes agree, and a
    proof-shaped round trip (mulgen -> bytes -> wire-format MSM) holds under the rule.  Rule 0 is the default everywhere else."""
    ks = [1, 2, 3, o.P - 1] + [random.Random(50 + rule).randrange(o.P) for _ in range(12)]
    try:
        dvp.check(dvp.lib.dvp_codec_set_rule(rule))
        assert dvp.lib.dvp_codec_get_rule() == rule
        enc = dvp.curve.point_scalar_mul_gen_batch_bytes(to_limbs(ks + [0]))
        for i, k in enumerate(ks):
            assert enc[i].tobytes() == o.xsk233_encode(co.k233_mulgen(k), rule), (rule, k)
            assert o.xsk233_decode(enc[i].tobytes(), rule) == (co.k233_mulgen(k), True)
        assert enc[-1].tobytes() == bytes(30)
        xy, inf = dvp.curve.from_bytes(enc)
        for i, k in enumerate(ks):
            assert np_to_pt(xy[i], inf[i]) == co.k233_mulgen(k)
        assert inf[-1] == 1 and (dvp.curve.to_bytes(xy, inf) == enc).all()
        rnd = random.Random(60 + rule)
        for _ in range(8):
            w = rnd.getrandbits(233).to_bytes(30, "big" if rule & 2 else "little")
            exp, ok = o.xsk233_decode(w, rule)
            try:
                x, i_ = dvp.curve.from_bytes(np.frombuffer(w, dtype=np.uint8))
                assert ok and np_to_pt(x[0], i_[0]) == exp
            except dvp.DvpError as e:
                assert not ok and e.status == -2
        n = 64
        k, s = rand_fr_np(n, 70 + rule), rand_fr_np(n, 71 + rule)
        out = dvp.curve.multi_scalar_mul_bytes(s.view(np.uint8).reshape(n, 32), dvp.curve.point_scalar_mul_gen_batch_bytes(k))
        assert out == o.xsk233_encode(co.k233_mulgen(np_dot_mod(s, k)), rule)
    finally:
        dvp.check(dvp.lib.dvp_codec_set_rule(0))
    assert dvp.lib.dvp_codec_set_rule(12) == -1 and dvp.lib.dvp_codec_get_rule() == 0


def test_msm_wire_format(dvp):
    """scalars 32-B LE + bases 30-B encodings in, 30-B encoding out (the reference's file payloads)."""
    n = 300
    k, s = rand_fr_np(n, 51), rand_fr_np(n, 52)
    enc = dvp.curve.point_scalar_mul_gen_batch_bytes(k)
    out = dvp.curve.multi_scalar_mul_bytes(s.view(np.uint8).reshape(n, 32), enc)
    assert out == co.xsk233_encode(co.k233_mulgen(np_dot_mod(s, k)))


@pytest.mark.parametrize("slide", [0, 3])  # signed aligned binary windows (the default) / tau-adic aligned windows
@pytest.mark.parametrize("hint", [0, 1 << 10, 1 << 24])
def test_fixed_base_msm_context(dvp, hint, slide):
    """dvp_msm_ctx_*: pre-rotated bases, shared bucket set; full range, sub-ranges (the per-GPU shards) and a
    neutral base, for several window sizes (range_hint drives the choice; 2^24 forces c = 20, two-level sort), with both
    table flavours (signed binary windows over rows 2^(o_w) P, tau-adic windows over rows tau^(o_w) P)."""
    n = 6000
    k, s = rand_fr_np(n, 61), rand_fr_np(n, 62)
    bases, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    inf = np.zeros(n, dtype=np.uint8)
    inf[5] = 1
    knobs = {"DVP_MSM_ALIGNED_SIGNED": 0 if slide == 3 else 1}
    if hint <= n:
        with dvp.tune(**knobs):
            fb = dvp.curve.FixedBaseMsm(bases, inf, hint)
    else:
        with dvp.tune(DVP_MSM_FIXED_C=20, **knobs):
            fb = dvp.curve.FixedBaseMsm(bases, inf, 0)
    ks, ss = from_limbs(k), from_limbs(s)

    def expect(lo, hi):
        return co.k233_mulgen(sum(ss[i] * ks[i] for i in range(lo, hi) if i != 5) % o.P)

    xy, is_inf = fb.run(s)
    assert np_to_pt(xy, is_inf) == expect(0, n)
    # pair rounds all the way down (normally only while a round has >= 2^19 additions), with 1, 3 and 64 additions per
    # shared inversion at most (the device picks the count per round; one chip-full holds this whole input)
    for bmax in (1, 3, 64):
        with dvp.tune(DVP_MSM_AFF_MIN=64, DVP_MSM_AFF_BMAX=bmax):
            xy, is_inf = fb.run(s)
            assert np_to_pt(xy, is_inf) == expect(0, n)
            xy, is_inf = fb.run(s[7:4000], 7, 4000)
            assert np_to_pt(xy, is_inf) == expect(7, 4000)
    parts = []
    for lo, hi in ((0, 1500), (1500, 1501), (1501, 6000), (10, 10)):
        xy, is_inf = fb.run(s[lo:hi], lo, hi)
        got = np_to_pt(xy, is_inf)
        assert got == (expect(lo, hi) if hi > lo else None)
        parts.append(got)
    acc = None
    for pt in parts:
        acc = o.k233_add(acc, pt)
    assert acc == expect(0, n)  # the shards add up to the whole (what the all-gather + local add relies on)
    # a scalar >= p is refused with its index, whichever kernel recodes (level 1 of the sort reads the scalars itself by default)
    bad = s.copy()
    bad[4321] = to_limbs([o.P])[0]
    for fused in (0, 1):
        with dvp.tune(DVP_MSM_SORT_FUSED=fused):
            with pytest.raises(dvp.DvpError) as ei:
                fb.run(bad)
            assert ei.value.status == -1 and ei.value.index == 4321
            xy, is_inf = fb.run(s)
            assert np_to_pt(xy, is_inf) == expect(0, n)


def test_msm_heavy_skew_2_18(dvp):
    """2^18 scalars drawn from {0, 1, 2, 3}: a handful of buckets receive ~2^16 points each (R1CS witnesses
    look like this: mostly bits and small values).  Exercises ~17 pair rounds and the skew-balanced reducer."""
    n = 1 << 18
    k = rand_fr_np(n, 71)
    bases, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    rng = np.random.default_rng(72)
    s = np.zeros((n, 4), dtype=np.uint64)
    s[:, 0] = rng.integers(0, 4, size=n)
    assert gpu_msm(dvp, s, bases) == co.k233_mulgen(np_dot_mod(s, k))
    fb = dvp.curve.FixedBaseMsm(bases)
    xy, is_inf = fb.run(s)
    assert np_to_pt(xy, is_inf) == co.k233_mulgen(np_dot_mod(s, k))


M = "msm.hip:"
FAST_TABLE = [M + "k_accum_affine_fast<true,true>", M + "k_accum_affine_fast<true,false>", M + "k_accum_affine_rest<true>"]
FAST_ROUNDS = [M + "k_accum_affine_fast<false,true>", M + "k_accum_affine_fast<false,false>", M + "k_accum_affine_rest<false>"]
GENERAL = [M + "k_accum_affine<true,true>", M + "k_accum_affine<true,false>", M + "k_accum_affine<false,true>", M + "k_accum_affine<false,false>"]
PAIRS = [M + "k_bucket_pairs", M + "k_bucket_rest"]
GATHERS = [M + "k_bucket_gather_items", M + "k_bucket_gather_aff"]
ROUNDS = [M + "k_affine_round<true,false,false>", M + "k_affine_round<false,false,false>", M + "k_affine_round<false,false,true>"]


def reducer_route(dvp, n, windows, aff_min, pairs_max, fast=1):
    """the launch census of one MSM of the exceptional-pairs input against the route msm_core takes for it; returns whether that
    route keeps a rest list that this input must fill.  e = n x windows entries; rounds planned: ra_plan with (e >> ra_plan) >= aff_min
    > (e >> (ra_plan + 1)).  The input's buckets hold hundreds of points, so every planned round runs and:
      no round   -> the reducer reads table entries: k_accum_affine_fast<true,*> + k_accum_affine_rest<true> (DVP_MSM_BUCKET_PAIRS_MAX
                    only applies behind a round), the general k_accum_affine<true,*> with DVP_MSM_ACCUM_FAST = 0;
      1 .. 4     -> more than 12 points per bucket are left: k_bucket_pairs + k_bucket_rest with DVP_MSM_BUCKET_PAIRS_MAX = 100000,
                    else the reducer on the rounds' output, k_accum_affine_fast<false,*> + _rest<false> / k_accum_affine<false,*>;
      more       -> (DVP_MSM_AFF_MIN = 32, 512) how many points the last round leaves is the device's business: one per bucket goes
                    through k_bucket_gather_aff; the census still shows that the knob kept the other family out.
    The rest list is non-empty where the route keeps one and at most one round ran: the buckets are full of equal and opposite
    points then.  (Measured on this input: four rounds have used the exceptional pairs up, the list is empty from there on.)"""
    e, ra_plan = n * windows, 0
    while (e >> (ra_plan + 1)) >= aff_min:
        ra_plan += 1
    where = (n, windows, aff_min, pairs_max, fast, ra_plan)
    first = (FAST_TABLE if fast else GENERAL[:2]) if ra_plan == 0 else (FAST_ROUNDS if fast else GENERAL[2:])
    others = [x for x in FAST_TABLE + FAST_ROUNDS + GENERAL if x not in first]
    if ra_plan == 0:
        assert_census(dvp, [first[0][:first[0].index("<")] + "*"], others + PAIRS + GATHERS + ROUNDS, where)
        if fast:
            assert_census(dvp, [first[-1]], [], where)
    elif ra_plan <= 4:
        assert_census(dvp, [ROUNDS[0]], [GATHERS[0]], where)
        if pairs_max >= 100000:
            assert_census(dvp, PAIRS, FAST_TABLE + FAST_ROUNDS + GENERAL + GATHERS + [M + "k_bucket_gather"], where)
        else:
            assert_census(dvp, [first[0][:first[0].index("<")] + "*", M + "k_bucket_gather"], others + PAIRS + GATHERS, where)
            if fast:
                assert_census(dvp, [first[-1]], [], where)
    else:
        assert_census(dvp, ROUNDS[:1], [GATHERS[0]] + FAST_TABLE + GENERAL[:2] + (PAIRS if pairs_max == 0 else []) +
                      (FAST_ROUNDS + GENERAL[2:] + [M + "k_bucket_gather"] if pairs_max >= 100000 else []) + (FAST_ROUNDS if not fast else GENERAL[2:]), where)
    keeps_list = ra_plan <= 1 and (fast or (ra_plan == 1 and pairs_max >= 100000))
    if keeps_list:
        assert rest_len(dvp) > 0, where
    return keeps_list


def test_bucket_reduction_exceptional_pairs(dvp):
    """what the pair rounds leave (k_bucket_pairs / k_bucket_rest): bases drawn from eight points and their negatives,
    scalars from five values, so that the buckets the rounds hand over hold equal points (P + P), opposite points
    (P - P) and the infinity markers earlier rounds made of them -- the pairs the fast formulas refuse and the list
    redoes.  Fixed-base and one-shot, the rounds stopped at several depths (after none and after one as well: DVP_MSM_AFF_MIN =
    2^19 / 2^15, where the reducer's own exception-free first level and its rest list take the table entries / the first round's
    output), against the fan-in-K reducer route (DVP_MSM_BUCKET_PAIRS_MAX=0) and the oracle.  Beside every oracle comparison the
    launch census shows the route that ran (reducer_route), and the rest list's length that it was used."""
    bases, s, sv, ks, exp = exceptional_pairs_input()
    lo, hi = 100, 3000
    exp_part = co.k233_mulgen(sum(a * b for a, b in zip(sv[lo:hi], ks[lo:hi])) % o.P)
    listed = 0
    for c in (8, 11):
        with dvp.tune(DVP_MSM_FIXED_C=c):
            fb = dvp.curve.FixedBaseMsm(bases)
        w_fx, w_os = fb.plan()[1], (234 + c - 1) // c  # entries per point that really exist (the overflow windows stay empty)
        for aff_min in (32, 512, 4096, 1 << 15, 1 << 19):
            for pairs_max in (0, 12, 100000):
                with dvp.tune(DVP_MSM_AFF_MIN=aff_min, DVP_MSM_BUCKET_PAIRS_MAX=pairs_max, DVP_MSM_C=c, DVP_MSM_ROUND_PIPELINE=int(aff_min != 512)):
                    dvp.lib.dvp_profile_reset()
                    assert np_to_pt(*fb.run(s)) == exp, (c, aff_min, pairs_max)
                    listed += reducer_route(dvp, len(sv), w_fx, aff_min, pairs_max)
                    dvp.lib.dvp_profile_reset()
                    assert np_to_pt(*fb.run(s[lo:hi], lo, hi)) == exp_part, (c, aff_min, pairs_max)
                    listed += reducer_route(dvp, hi - lo, w_fx, aff_min, pairs_max)
                    dvp.lib.dvp_profile_reset()
                    assert gpu_msm(dvp, s, bases) == exp, (c, aff_min, pairs_max)
                    listed += reducer_route(dvp, len(sv), w_os, aff_min, pairs_max)
                if pairs_max == 0:
                    # round 6: the reducer's first level without exceptional branches + its rest list (k_accum_affine_fast / _rest), its last
                    # level on rows of 16 lanes, ld_add_nodbl's doubling from a copy, the one-shot tail's group sums -- each switched off in turn
                    for knob in ("DVP_MSM_ACCUM_FAST", "DVP_MSM_ACCUM_HEX_MAX", "DVP_MSM_TAIL_GROUPS"):
                        off = {"DVP_MSM_ACCUM_FAST": FAST_TABLE + FAST_ROUNDS, "DVP_MSM_ACCUM_HEX_MAX": [M + "k_accum_proj<16>"], "DVP_MSM_TAIL_GROUPS": [M + "k_tail_groups"]}[knob]
                        with dvp.tune(DVP_MSM_AFF_MIN=aff_min, DVP_MSM_BUCKET_PAIRS_MAX=0, DVP_MSM_C=c, **{knob: 0}):
                            dvp.lib.dvp_profile_reset()
                            assert np_to_pt(*fb.run(s)) == exp, (c, aff_min, knob)
                            reducer_route(dvp, len(sv), w_fx, aff_min, 0, fast=int(knob != "DVP_MSM_ACCUM_FAST"))
                            assert_census(dvp, [], off, (c, aff_min, knob))
                            dvp.lib.dvp_profile_reset()
                            assert gpu_msm(dvp, s, bases) == exp, (c, aff_min, knob)
                            reducer_route(dvp, len(sv), w_os, aff_min, 0, fast=int(knob != "DVP_MSM_ACCUM_FAST"))
                            assert_census(dvp, [M + "k_tail<false>"], off, (c, aff_min, knob))
        fb.close()
    assert listed >= 2 * 2 * 3 * 2  # both windows, AFF_MIN 2^15 and 2^19, every DVP_MSM_BUCKET_PAIRS_MAX, fixed-base and one-shot at the least


def test_msm_multiplier_form_knobs(dvp):
    """the knobs that choose a multiplier form or a launch shape and that no other test sets, each at a value that really switches the
    path where msm_core reads it, on the exceptional-pair input above and on 3 000 random points, fixed-base and one-shot, against
    the oracle:
      DVP_GF_INV_TABS 0 / 2 -- gf_sqr_tables(): the inversion's runs of 14 and 7 squarings plain / both as table passes;
      DVP_MSM_HEX_MAX=0 -- no merge level and no tail on rows of 16 lanes (quads up to DVP_MSM_QUAD_MAX additions instead);
      DVP_MSM_QUAD_MAX=2^30 with HEX_MAX=0 -- EVERY merge level on quads; =1 with HEX_MAX=0 -- every level of more than one addition
        one lane per addition (the Karatsuba form);
      DVP_MSM_ACCUM_QUAD_MAX=2^30 / 1 -- the fan-in reducer (forced with DVP_MSM_BUCKET_PAIRS_MAX=0; its row-of-16 last level off) all
        quads / none, on table entries (no pair rounds) and on the affine output of a few pair rounds (DVP_MSM_AFF_MIN=4096), there
        with and without the exception-free first level (k_accum_affine_fast / k_accum_affine);
      DVP_MSM_AFF_TPB 64 / 128, DVP_MSM_AFF_BMIN 1 / 136 (= DVP_MSM_AFF_BMAX, the most it accepts) -- the pair rounds, which
        DVP_MSM_AFF_MIN=32 makes run at this size;
      DVP_FX_HI at both ends of what msm_fixed_settle accepts (0 <= h <= 10, 1 <= key bits - h <= 15): 0 / 9 for c = 11 (10 key bits),
        2 / 10 for c = 18 (17 key bits); read when the context is created.
    Beside each oracle comparison of a setting the launch census shows the variants the setting names ran and their complement under
    that knob did not (paths, below)."""
    big = 1 << 30
    xb, xs, _, _, xexp = exceptional_pairs_input()
    n = 3000
    k, s = rand_fr_np(n, 4101), rand_fr_np(n, 4102)
    rb, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    rexp = co.k233_mulgen(np_dot_mod(s, k))
    inputs = ((xb, xs, xexp), (rb, s, rexp))
    reducer = dict(DVP_MSM_BUCKET_PAIRS_MAX=0, DVP_MSM_ACCUM_HEX_MAX=0)
    rounds = dict(DVP_MSM_AFF_MIN=32)
    settings = [
        dict(DVP_GF_INV_TABS=0, **rounds), dict(DVP_GF_INV_TABS=2, **rounds), dict(DVP_GF_INV_TABS=0), dict(DVP_GF_INV_TABS=2),
        dict(DVP_MSM_HEX_MAX=0), dict(DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=big), dict(DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=1),
        dict(DVP_MSM_ACCUM_QUAD_MAX=big, **reducer), dict(DVP_MSM_ACCUM_QUAD_MAX=1, **reducer),
        dict(DVP_MSM_ACCUM_QUAD_MAX=big, DVP_MSM_ACCUM_FAST=0, DVP_MSM_AFF_MIN=4096, **reducer),
        dict(DVP_MSM_ACCUM_QUAD_MAX=1, DVP_MSM_ACCUM_FAST=0, DVP_MSM_AFF_MIN=4096, **reducer),
        dict(DVP_MSM_ACCUM_QUAD_MAX=big, DVP_MSM_AFF_MIN=4096, **reducer), dict(DVP_MSM_ACCUM_QUAD_MAX=1, DVP_MSM_AFF_MIN=4096, **reducer),
        dict(DVP_MSM_AFF_TPB=64, **rounds), dict(DVP_MSM_AFF_TPB=128, **rounds),
        dict(DVP_MSM_AFF_BMIN=1, **rounds), dict(DVP_MSM_AFF_BMIN=136, **rounds),
    ]
    for knob in ("DVP_GF_INV_TABS", "DVP_MSM_HEX_MAX", "DVP_MSM_QUAD_MAX", "DVP_MSM_ACCUM_QUAD_MAX", "DVP_MSM_AFF_TPB", "DVP_MSM_AFF_BMIN"):
        assert any(knob in st for st in settings)
    merges = {g: [f"{M}k_merge<{g},true>", f"{M}k_merge<{g},false>"] for g in (1, 4, 16)}
    proj = {g: f"{M}k_accum_proj<{g}>" for g in (1, 4, 16)}

    def paths(st, one_shot, random_points):
        """(variants that ran, variants that did not) under the setting `st`, from the launch census: what the knob selects where
        msm_core reads it, and its complement.  c = 11: 1 024 buckets fixed-base, 23 x 2 048 one-shot; every merge level has at least
        ten additions, so DVP_MSM_QUAD_MAX = 1 leaves none to the quads."""
        ran, idle = [], []
        if st.get("DVP_MSM_AFF_MIN", 1 << 19) == 32:  # the pair rounds run (one-word descriptors: DVP_MSM_ROUND_DENSE is 0)
            ran += ROUNDS[:2]
            idle += ROUNDS[2:] + FAST_TABLE + GENERAL[:2]
        elif "DVP_MSM_AFF_MIN" not in st:
            idle += ROUNDS
        if st.get("DVP_MSM_HEX_MAX") == 0:
            idle += merges[16] + [M + "k_tail<true>"]
            ran += [M + "k_tail<false>"]
            if st.get("DVP_MSM_QUAD_MAX") == big:
                ran, idle = ran + merges[4], idle + merges[1]
            elif st.get("DVP_MSM_QUAD_MAX") == 1:
                ran, idle = ran + merges[1], idle + merges[4]
        if "DVP_MSM_ACCUM_QUAD_MAX" in st:  # the fan-in reducer, forced; its last level never on rows of 16
            quad = st["DVP_MSM_ACCUM_QUAD_MAX"] == big
            q, nq = ("true", "false") if quad else ("false", "true")
            idle += PAIRS + [proj[16], proj[1] if quad else proj[4]]
            behind_rounds = st.get("DVP_MSM_AFF_MIN") == 4096
            ind, nind = ("false", "true") if behind_rounds else ("true", "false")
            fast = st.get("DVP_MSM_ACCUM_FAST", 1)
            name = "k_accum_affine_fast" if fast else "k_accum_affine"
            mine = [f"{M}{name}<{ind},{q}>"] + ([f"{M}k_accum_affine_rest<{ind}>"] if fast else [])
            idle += [x for x in FAST_TABLE + FAST_ROUNDS + GENERAL if x not in mine]
            # (3 000 random points one-shot: ~1.4 points per bucket, the largest holds a handful: four planned rounds leave one point
            # per bucket and k_bucket_gather_aff takes them -- no reducer level runs, whatever the knob; everywhere else the named one does)
            if not (behind_rounds and one_shot and random_points):
                ran += mine + [M + "k_bucket_gather"]
            if behind_rounds:
                ran += ROUNDS[:1]
        return ran, idle

    for bases, sc, exp in inputs:
        with dvp.tune(DVP_MSM_FIXED_C=11):
            fb = dvp.curve.FixedBaseMsm(bases)
        assert np_to_pt(*fb.run(sc)) == exp and gpu_msm(dvp, sc, bases) == exp  # the defaults
        for st in settings:
            with dvp.tune(DVP_MSM_C=11, **st):
                dvp.lib.dvp_profile_reset()
                assert np_to_pt(*fb.run(sc)) == exp, st
                assert_census(dvp, *paths(st, False, bases is rb), (st, "fixed-base"))
                dvp.lib.dvp_profile_reset()
                assert gpu_msm(dvp, sc, bases) == exp, st
                assert_census(dvp, *paths(st, True, bases is rb), (st, "one-shot"))
        fb.close()
        for c, his in ((11, (0, 9)), (18, (2, 10))):
            for h in his:
                with dvp.tune(DVP_MSM_FIXED_C=c, DVP_FX_HI=h):
                    fb = dvp.curve.FixedBaseMsm(bases)
                for aff_min in (32, 1 << 19):
                    with dvp.tune(DVP_MSM_AFF_MIN=aff_min):
                        assert np_to_pt(*fb.run(sc)) == exp, (c, h, aff_min)
                fb.close()


def test_merge_tree_equal_and_opposite_buckets(dvp):
    """the merge tree's exceptional additions (k_merge, lambda-projective: equal operands are doubled from a copy read back,
    opposite ones give infinity): bases P, P, Q, -Q with scalars 2, 3, 4, 5 put the SAME point into buckets 2 and 3 and opposite
    points into buckets 4 and 5, which level 0 adds -- with few buckets (one quad per addition) and with 2^17 (one lane per
    addition); then the same with the pairs one level up (scalars 4, 6 / 8, 10: buckets (4,5)+(6,7) and (8,9)+(10,11))"""
    kp, kq = 0x1234567, 0x7654321
    P, Q = co.k233_mulgen(kp), co.k233_mulgen(kq)
    bases = pts_to_np([P, P, Q, o.k233_neg(Q)])
    for sv in ([2, 3, 4, 5], [4, 6, 8, 10], [1, 1, 3, 3], [6, 7, 1 << 100, (1 << 100) + 1]):
        exp = co.k233_mulgen(((sv[0] + sv[1]) * kp + (sv[2] - sv[3]) * kq) % o.P)
        for c in (8, 18):
            with dvp.tune(DVP_MSM_FIXED_C=c):
                fb = dvp.curve.FixedBaseMsm(bases)
            assert np_to_pt(*fb.run(to_limbs(sv))) == exp, (sv, c)
            fb.close()
        for c in (4, 12):
            with dvp.tune(DVP_MSM_C=c):
                assert gpu_msm(dvp, to_limbs(sv), bases) == exp, (sv, c)


def test_points_add_like_curvepoint_add(dvp):
    """CurvePoint::add (src/curve.rs:84-90): generic, doubling, P + (-P), neutral on either side -- vs the oracle group law"""
    import pyref as o2
    rnd = random.Random(44)
    ks = [rnd.randrange(1, o.P) for _ in range(6)]
    pts = [co.k233_mulgen(k) for k in ks]
    neg = lambda p: (p[0], p[0] ^ p[1])
    a = [pts[0], pts[1], pts[2], pts[3], pts[4], pts[5]]
    b = [pts[1], pts[1], neg(pts[2]), pts[0], pts[4], pts[3]]
    a_inf = np.array([0, 0, 0, 1, 0, 1], dtype=np.uint8)
    b_inf = np.array([0, 0, 0, 0, 1, 1], dtype=np.uint8)
    xy, inf = dvp.curve.add(pts_to_np(a), pts_to_np(b), a_inf, b_inf)
    exp = [o2.k233_add(a[0], b[0]), o2.k233_add(a[1], a[1]), None, b[3], a[4], None]
    for i, e in enumerate(exp):
        assert np_to_pt(xy[i], bool(inf[i])) == e, i


@pytest.mark.parametrize("log_n", [20, 22])
def test_msm_full_size_dlog_and_linearity(dvp, log_n):
    """full size, oracle-backed: bases k_i*G, so MSM(s) must equal (sum s_i k_i)*G computed by the OpenSSL-pinned C
    oracle -- for the one-shot and the fixed-base path (the shape of the reference's test_msm, src/curve.rs:218-232);
    plus the reference's linearity property MSM(s) + MSM(t) == MSM(s + t) (src/curve.rs:198-215)"""
    n = 1 << log_n
    k = rand_fr_np(n, 81)
    bases, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    s, t = rand_fr_np(n, 82), rand_fr_np(n, 83)
    fb = dvp.curve.FixedBaseMsm(bases)
    exp_s = co.k233_mulgen(np_dot_mod_fast(s, k))
    ps_one, ps_fix = gpu_msm(dvp, s, bases), np_to_pt(*fb.run(s))
    assert ps_one == exp_s and ps_fix == exp_s
    if log_n == 20:
        exp_t = co.k233_mulgen(np_dot_mod_fast(t, k))
        assert np_to_pt(*fb.run(t)) == exp_t
        st_sum = to_limbs([(a + b) % o.P for a, b in zip(from_limbs(s), from_limbs(t))])
        pst = np_to_pt(*fb.run(st_sum))
        assert o.k233_add(exp_s, exp_t) == pst == gpu_msm(dvp, st_sum, bases)
    fb.close()


def test_fixed_base_vs_one_shot_randomised(dvp):
    """differential sweep: every fixed-base window size 8..21 of the signed and 8..20 of the tau-adic aligned windows (both sort
    flavours, 4/8/16-slot pair rounds) against the one-shot path on random sub-ranges, plus scalars with long runs of
    zero / one digits"""
    rnd = random.Random(2026)
    n = 3000
    k = rand_fr_np(n, 91)
    bases, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    s = rand_fr_np(n, 92)
    special = [0, 1, 2, o.P - 1, o.P - 2, (1 << 231) - 1, 1 << 230, (1 << 116) + 1, 0xFFFFFFFFFFFFFFFF, (o.P - 1) // 2, 3 << 200]
    # worst cases of the tau-adic recoding: corners of the reduction's fundamental region (longest expansions, 236 of the
    # proven 240 digits) and the rounding boundaries of its fixed-point quotients (tau.cuh)
    special += tau_adversarial_scalars()
    assert max(len(co.tau_digits(x)) for x in special) >= 236
    s[: len(special)] = to_limbs(special)
    ks, ss = from_limbs(k), from_limbs(s)
    # slide: 0 = aligned windows of signed binary digits (the default flavour), 3 = aligned tau-adic windows
    for c, slide in [(c, 0) for c in range(8, 22)] + [(c, 3) for c in range(8, 21)]:
        with dvp.tune(DVP_MSM_FIXED_C=c, DVP_MSM_ALIGNED_SIGNED=0 if slide == 3 else 1,
                      DVP_MSM_AFF_MIN=rnd.choice([16, 256, 4096, 1 << 19]),
                      DVP_MSM_AFF_BMAX=rnd.choice([2, 7, 48]), DVP_MSM_SORT_FUSED=c & 1, DVP_MSM_ROUND_PIPELINE=(c >> 1) & 1):
            fb = dvp.curve.FixedBaseMsm(bases)
            if slide == 0:  # 234 bits in ceil(234 / c) windows evened out; all windows narrow = the plan of c - 1 (19 -> 18, 21 -> 20)
                ce = c
                while (234 + ce - 1) // ce * ce - 234 >= (234 + ce - 1) // ce:
                    ce -= 1
                assert fb.plan() == (ce, (234 + ce - 1) // ce)
            else:
                assert fb.plan() == (c, (234 + c - 1) // c + 1)
            for _ in range(3):
                lo = rnd.randrange(0, n - 1)
                hi = rnd.randrange(lo + 1, n + 1)
                xy, is_inf = fb.run(s[lo:hi], lo, hi)
                exp = co.k233_mulgen(sum(ss[i] * ks[i] for i in range(lo, hi)) % o.P)
                assert np_to_pt(xy, is_inf) == exp, (c, slide, lo, hi)
                assert gpu_msm(dvp, s[lo:hi], bases[lo:hi]) == exp, (c, slide, lo, hi)
            fb.close()


def test_one_shot_randomised_shapes_and_knobs(dvp):
    """differential sweep of the ONE-SHOT path (per-window bucket sets): random sizes 1..40 000, scalar populations
    (uniform / tiny / few distinct values / zeros and p-1 mixed in), neutral bases, every window size the cost model can
    pick (4..15), several reducer fan-ins, pair rounds all the way down and switched off -- each against the
    discrete-log identity with the OpenSSL-pinned oracle"""
    rnd = random.Random(4242)
    nmax = 40000
    k = rand_fr_np(nmax, 191)
    bases, _ = dvp.curve.point_scalar_mul_gen_batch(k)
    ks = from_limbs(k)
    for trial in range(28):
        n = rnd.choice([1, 2, 3, 63, 64, 65, 1000, 4097, rnd.randrange(1, nmax)])
        lo = rnd.randrange(0, nmax - n + 1)
        kind = trial % 4
        if kind == 0:
            sv = [rnd.randrange(o.P) for _ in range(n)]
        elif kind == 1:
            sv = [rnd.randrange(0, 16) for _ in range(n)]
        elif kind == 2:
            vals = [rnd.randrange(o.P) for _ in range(3)]
            sv = [rnd.choice(vals) for _ in range(n)]
        else:
            sv = [rnd.choice([0, o.P - 1, 1, rnd.randrange(o.P)]) for _ in range(n)]
        inf = np.zeros(n, dtype=np.uint8)
        if n > 4 and trial % 3 == 0:
            inf[rnd.randrange(n)] = 1
        exp = co.k233_mulgen(sum(s * ks[lo + i] for i, s in enumerate(sv) if not inf[i]) % o.P)
        knobs = dict(DVP_MSM_C=rnd.choice([0, 4, 7, 11, 15]), DVP_MSM_K=rnd.choice([0, 2, 5, 64]),
                     DVP_MSM_AFF_MIN=rnd.choice([1, 64, 1 << 19]), DVP_MSM_PROJ=int(trial % 7 == 6), DVP_MSM_AFF_BMAX=rnd.choice([1, 5, 48]))
        with dvp.tune(**knobs):
            assert gpu_msm(dvp, to_limbs(sv), bases[lo:lo + n], inf) == exp, (trial, n, knobs)


@pytest.mark.parametrize("c", [8, 13, 18, 19, 20, 21])
def test_signed_recode_words_vs_restatement(dvp, c):
    """k_recode_signed (the small-table flavour: aligned windows of signed binary digits) word for word against the textbook
    signed-digit decomposition restated in tests/msm_stage_cases.py (signed_recode): 234 bits in W = ceil(234 / c) windows, the W c - 234 LOW windows one bit
    narrower (so no window is short: a short top window would pile every scalar into a handful of buckets); window w holds
    its bits plus the carry from below, a digit above half its range becomes digit - 2^width with a carry;
    sum_w d_w 2^(o_w) is the scalar and |d_w| <= 2^(width_w - 1).  A c whose windows would all be narrow is refused
    (it is the plan of c - 1)."""
    import ctypes as C

    rnd = random.Random(500 + c)
    W = C.c_int(0)
    n_win = (234 + c - 1) // c
    n_narrow = n_win * c - 234
    rc = dvp.lib.dvp_debug_recode_signed(None, 0, c, None, C.byref(W))
    if n_narrow >= n_win:
        assert rc == -1
        return
    dvp.check(rc, "windows")
    assert W.value == n_win
    widths = [c - 1 if w < n_narrow else c for w in range(n_win)]
    assert sum(widths) == 234
    vals = [0, 1, 2, (1 << c) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << (c - 2)), (1 << (c - 2)) + 1, o.P - 1, (1 << 231) - 1, 1 << 230,
            int("1" * 231, 2)] + [rnd.randrange(o.P) for _ in range(1500)] + [rnd.randrange(1 << rnd.randrange(1, 232)) for _ in range(300)]
    # every window at exactly half its range, and one past it (the wrap / carry boundary of each width)
    off = 0
    for wd in widths[:-1]:
        vals += [1 << (off + wd - 1), (1 << (off + wd - 1)) + (1 << off), ((1 << wd) - 1) << off]
        off += wd
    s = to_limbs(vals)
    words = np.zeros((W.value, len(vals)), dtype=np.uint32)
    dvp.check(dvp.lib.dvp_debug_recode_signed(s.ctypes.data, len(vals), c, words.ctypes.data, C.byref(W)), "recode")
    for i, x in enumerate(vals):
        exp = signed_recode(x, c)  # the restatement (tests/msm_stage_cases.py): [(o_w, d_w)], sum_w d_w 2^(o_w) = x asserted there
        assert len(exp) == n_win and sum(d << o_w for o_w, d in exp) == x
        for w, (_, d) in enumerate(exp):
            word = int(words[w, i])
            if d == 0:
                assert word == 0, (c, i, w)
            else:
                assert word >> 31 == 1 and ((word >> 20) & 0xFF) == w and bool(word & 0x10000000) == (d < 0), (c, i, w, hex(word))
                assert (word & 0xFFFFF) == (abs(d) & ((1 << (c - 1)) - 1)), (c, i, w, d, hex(word))  # bucket key; 2^(c-1) -> bucket 0
