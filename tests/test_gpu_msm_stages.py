"""GPU tests (-m gpu): the MSM bucket pipeline stage by stage.  One MSM is run with the stage capture armed
(dvp_debug_msm_capture_arm / _fetch: the production path plus device-to-device copies at its stage boundaries) and every captured array
is compared, bit for bit, with the plain-Python restatements of tests/msm_stage_cases.py (check_capture):
  (a) cnt / off / items against bucket membership and the sort's layout; (b) every round's counts, offsets and descriptor words;
  (c) every output slot of every pair round against the group law on discrete logarithms (c_oracle.k233_mulgen);
  (d) every bucket after the leftover reducer; (e) the MSM's own result against the oracle;
  (f) to (i) the bucket array behind every merge level, bucket 0 kept aside, the tail's group sums and the result as the tail kernel wrote it.
Every expectation of a stage is computed from the captured input of that stage; the order inside a bucket is the sort's own.

The placement matrix (test_placement_matrix) runs placement_input(), whose bucket COUNTS put exceptional pairs at chosen lanes, waves,
workgroups and chain positions of k_affine_round's shared inversion, across workgroup sizes, inversion sharing, descriptor forms and
bookkeeping modes; assert_placement is its class coverage condition -- a class that does not occur fails the test."""
import ctypes as C

import numpy as np
import pytest

import pyref as o
import c_oracle as co
import msm_stage_cases as sc
from msm_cases import exceptional_pairs_input, random_input, distinct_input, assert_census, census, rest_len
from util import to_limbs, from_limbs, np_to_pt, rand_fr_np, pts_to_np

pytestmark = pytest.mark.gpu
ARENA = 96 << 20
M = "msm.hip:"


def capture(dvp, run, arena=ARENA):
    """arms the calling thread's next MSM, runs it, fetches and parses its capture: (what run() returned, Capture)"""
    lib = dvp.lib
    dvp.check(lib.dvp_debug_msm_capture_arm(arena), "arm")
    try:
        got = run()
        need = C.c_size_t(0)
        dvp.check(lib.dvp_debug_msm_capture_fetch(None, 0, C.byref(need)), "fetch size")
        buf = np.zeros(need.value // 4, dtype=np.uint32)
        dvp.check(lib.dvp_debug_msm_capture_fetch(buf.ctypes.data, need.value, C.byref(need)), "fetch")
    finally:
        lib.dvp_debug_msm_capture_arm(0)
    return got, sc.parse_capture(buf)


@pytest.fixture(scope="module")
def mg():
    return sc.Mulgen()


@pytest.fixture(scope="module")
def placement(dvp):
    """placement_input() as a fixed-base context at c = 8 (128 buckets): (context, scalar limbs, scalars, logs, the oracle's result)"""
    logs, scalars, _ = sc.placement_input()
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(to_limbs(logs))
    assert not inf.any()
    with dvp.tune(DVP_MSM_FIXED_C=sc.PLACE_C):
        fb = dvp.curve.FixedBaseMsm(bases)
    assert fb.plan() == (8, 30) and fb.table()[1]
    yield fb, to_limbs(scalars), scalars, logs, co.k233_mulgen(sum(s * k for s, k in zip(scalars, logs)) % o.P)
    fb.close()


@pytest.mark.parametrize("bmin", [1, 3])
@pytest.mark.parametrize("share", [0, 1])
@pytest.mark.parametrize("tpb", [64, 128, 256])
def test_placement_matrix(dvp, placement, mg, tpb, share, bmin):
    """placement_input() through every combination of workgroup size, shared inversion, descriptor form and bookkeeping mode, with one
    and with three slots per thread (at 600 slots a round is far below a chip-full: B = DVP_MSM_AFF_BMIN); the bookkeeping per round (0),
    for all rounds on a side stream (1) and on the caller's stream (2).  Per run: checks (a) to (i),
    six rounds, the route k_bucket_gather_aff, the header's echo of the knobs, and the class coverage condition
    (msm_stage_cases.assert_placement): round 0 holds P + P / P - P at lane 0 and lane 63 of wave 0, lane 0 of a later wave, the last
    lane of a workgroup, the first thread of the second workgroup, the last live thread of the partly filled last workgroup, chain
    positions 0 and B - 1 of one thread, over a whole wave and a whole workgroup (a pair, or the leftover of a bucket of +-P: nothing
    generic); lane 0 of wave 0 and the round's last slot are P - P under any order; every neutral-operand class occurs in a round >= 1."""
    fb, s_np, scalars, logs, exp = placement
    for pipeline in (0, 1, 2):
        for dense in (0, 1):
            knobs = dict(DVP_MSM_AFF_MIN=1, DVP_MSM_AFF_BMIN=bmin, DVP_MSM_AFF_TPB=tpb, DVP_MSM_AFF_SHARE_INV=share,
                         DVP_MSM_ROUND_DENSE=dense, DVP_MSM_ROUND_PIPELINE=pipeline)
            with dvp.tune(**knobs):
                got, cap = capture(dvp, lambda: np_to_pt(*fb.run(s_np)))
            h = cap.hdr
            where = (tpb, share, bmin, pipeline, dense)
            assert got == exp, ("result", where)  # (e)
            assert (h["flavour"], h["c"], h["W"], h["n_narrow"], h["nkeys"], h["n_total"], h["i0"], h["n"]) == (3, 8, 30, 6, 128, len(logs), 0, len(logs)), h
            assert (h["tpb"], h["bmin"], h["pipeline"], h["dense"], h["ra"], h["max_cnt"]) == (tpb, bmin, pipeline, int(dense and pipeline != 0), 6, 33), (h, where)
            assert h["share"] == [int(bool(share) and tpb > 64)] * 6 and h["route"] == sc.ROUTES.index("k_bucket_gather_aff"), (h, where)
            try:
                classes, bucket_logs = sc.check_capture(cap, logs, scalars, mulgen=mg)  # (a) - (d)
                found = sc.assert_placement(h, classes)
            except AssertionError as e:
                raise AssertionError((where,) + e.args) from e
            assert co.k233_mulgen(sc.weighted_sum(h, bucket_logs)) == exp
            print(where, "O-operand classes at named positions:", {r: {k: v for k, v in f.items() if set(v) & set(sc.O_CLASSES) and not k.startswith("a whole")} for r, f in found.items()})
    assert mg.calls <= 10000


def one_shot(dvp, bases, s_np):
    xy, is_inf = dvp.curve.multi_scalar_mul(s_np, bases)
    return np_to_pt(xy, is_inf)


def test_one_shot_exceptional_pairs(dvp):
    """exceptional_pairs_input(4096), one-shot at c = 8 (31 windows of bucket sets of their own), pair rounds all the way down: buckets of
    hundreds of equal and opposite points, every class of slot in most rounds"""
    bases, s_np, sv, ks, exp = exceptional_pairs_input(4096)
    with dvp.tune(DVP_MSM_C=8, DVP_MSM_AFF_MIN=1):
        got, cap = capture(dvp, lambda: one_shot(dvp, bases, s_np))
    assert got == exp
    h = cap.hdr
    assert (h["flavour"], h["c"], h["W"], h["nkeys"], h["n"], h["sign_mask"]) == (0, 8, 31, 31 << 8, 4096, 0) and h["ra"] >= 8, h
    classes, bucket_logs = sc.check_capture(cap, ks, sv)
    assert co.k233_mulgen(sc.weighted_sum(h, bucket_logs)) == exp
    # ~150 buckets of ~800 points +-P_j, j < 8: a sixteenth of the first round's sums are neutral, so the next round meets them on either
    # side and on both (expected counts in the thousands / hundreds); a neutral LEFTOVER needs an odd bucket to end in one and is chance
    assert set(classes[0]) >= {"generic", "P+P", "P-P"} and set().union(*map(set, classes[1:])) >= {"O+Q", "P+O", "O+O"}


def test_one_shot_random(dvp):
    """random_input(3000), one-shot at c = 8: ~11 points per bucket, generic additions and leftovers"""
    seed = 8800
    bases, s_np, exp = random_input(dvp, 3000, seed)
    ks, sv = from_limbs(rand_fr_np(3000, seed)), from_limbs(s_np)
    with dvp.tune(DVP_MSM_C=8, DVP_MSM_AFF_MIN=1):
        got, cap = capture(dvp, lambda: one_shot(dvp, bases, s_np))
    assert got == exp
    assert (cap.hdr["flavour"], cap.hdr["c"], cap.hdr["n"]) == (0, 8, 3000) and cap.hdr["ra"] >= 4, cap.hdr
    classes, bucket_logs = sc.check_capture(cap, ks, sv)
    assert co.k233_mulgen(sc.weighted_sum(cap.hdr, bucket_logs)) == exp
    assert set(classes[0]) == {"generic", "leftover"}


def test_dev_entry_on_a_stream(dvp):
    """the _dev entry on a stream of the caller's: the copies ride that stream and the fetch waits for it"""
    import torch

    n, seed = 300, 8810
    bases, s_np, exp = random_input(dvp, n, seed)
    ks, sv = from_limbs(rand_fr_np(n, seed)), from_limbs(s_np)
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(s_np.view(np.int64)).to(dev)
    d_b = torch.from_numpy(np.ascontiguousarray(bases).view(np.int64)).to(dev)
    d_out = torch.zeros(10, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def run():
        dvp.curve.multi_scalar_mul_dev(d_s.data_ptr(), d_b.data_ptr(), None, n, d_out.data_ptr(), d_out.data_ptr() + 64, st.cuda_stream)

    with dvp.tune(DVP_MSM_C=8, DVP_MSM_AFF_MIN=1, DVP_MSM_AFF_BMIN=1):
        _, cap = capture(dvp, run)
    st.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert np_to_pt(out[:8], bool(out[8] & 0xFFFFFFFF)) == exp
    _, bucket_logs = sc.check_capture(cap, ks, sv)
    assert co.k233_mulgen(sc.weighted_sum(cap.hdr, bucket_logs)) == exp


@pytest.fixture(scope="module")
def exceptional_ctx(dvp):
    bases, s_np, sv, ks, _ = exceptional_pairs_input(4096)
    with dvp.tune(DVP_MSM_FIXED_C=8):
        fb = dvp.curve.FixedBaseMsm(bases)
    yield fb, s_np, sv, ks
    fb.close()


@pytest.mark.parametrize("route,knobs", [
    ("k_bucket_pairs", dict(DVP_MSM_BUCKET_PAIRS_MAX=100000)),
    ("reducer_fast", dict(DVP_MSM_BUCKET_PAIRS_MAX=0, DVP_MSM_ACCUM_FAST=1)),
    ("reducer_general", dict(DVP_MSM_BUCKET_PAIRS_MAX=0, DVP_MSM_ACCUM_FAST=0)),
])
def test_leftover_routes_behind_one_round(dvp, exceptional_ctx, mg, route, knobs):
    """the three leftover routes that add points, each behind ONE pair round (DVP_MSM_AFF_MIN = 2^14 over 1 200 x 30 entries) of the
    exceptional input's bases 100 .. 1300 (i0 > 0): buckets of hundreds of equal and opposite points and the neutral markers the round
    made of them reach the reducer -- k_bucket_pairs' rest list and the fan-in reducer's are non-empty"""
    fb, s_np, sv, ks = exceptional_ctx
    lo, hi = 100, 1300
    exp = co.k233_mulgen(sum(a * b for a, b in zip(sv[lo:hi], ks[lo:hi])) % o.P)
    with dvp.tune(DVP_MSM_AFF_MIN=1 << 14, **knobs):
        dvp.lib.dvp_profile_reset()
        got, cap = capture(dvp, lambda: np_to_pt(*fb.run(s_np[lo:hi], lo, hi)))
        listed = rest_len(dvp)
    assert got == exp
    h = cap.hdr
    assert (h["ra"], h["i0"], h["n"], h["n_total"], sc.ROUTES[h["route"]]) == (1, lo, hi - lo, 4096, route), h
    assert listed > 0 or route == "reducer_general"
    if route == "k_bucket_pairs":
        assert_census(dvp, [M + "k_bucket_pairs", M + "k_bucket_rest"], [M + "k_bucket_gather", M + "k_accum_affine*"], route)
    else:
        assert_census(dvp, [M + ("k_accum_affine_fast*" if route == "reducer_fast" else "k_accum_affine<*"), M + "k_bucket_gather"], [M + "k_bucket_pairs"], route)
    _, bucket_logs = sc.check_capture(cap, ks, sv[lo:hi], mulgen=mg)
    assert co.k233_mulgen(sc.weighted_sum(h, bucket_logs)) == exp


def test_leftover_route_gather_items(dvp, mg):
    """no pair round and one point per bucket: k_bucket_gather_items reads the table through the sorted items"""
    bases, s_np, exp = distinct_input(dvp, 16)
    ks = from_limbs(rand_fr_np(16, 9401))
    with dvp.tune(DVP_MSM_FIXED_C=8):
        fb = dvp.curve.FixedBaseMsm(bases)
    got, cap = capture(dvp, lambda: np_to_pt(*fb.run(s_np)))
    fb.close()
    assert got == exp and (cap.hdr["ra"], sc.ROUTES[cap.hdr["route"]], cap.hdr["max_cnt"]) == (0, "k_bucket_gather_items", 1), cap.hdr
    _, bucket_logs = sc.check_capture(cap, ks, list(range(1, 17)), mulgen=mg)
    assert co.k233_mulgen(sc.weighted_sum(cap.hdr, bucket_logs)) == exp


def test_capture_arming_and_small_buffers(dvp, placement):
    """a fetch without a captured MSM is refused; an arena too small for the MSM's copies gives an error, the size it wanted and NO blob;
    a host buffer too small is refused and the capture stays; only the armed MSM is captured; armed or not, an MSM makes the same kernel
    launches and host waits (the launch census and the wait counters of the two runs are equal)"""
    fb, s_np, scalars, logs, exp = placement
    lib = dvp.lib
    need = C.c_size_t(7)
    assert lib.dvp_debug_msm_capture_fetch(None, 0, C.byref(need)) == -1 and need.value == 0
    dvp.check(lib.dvp_debug_msm_capture_arm(4096))
    assert np_to_pt(*fb.run(s_np)) == exp
    buf = np.full(1024, 0xA5A5A5A5, dtype=np.uint32)
    assert lib.dvp_debug_msm_capture_fetch(buf.ctypes.data, buf.nbytes, C.byref(need)) == -1 and need.value == 0
    assert lib.dvp_last_error_index() > 4096 and (buf == 0xA5A5A5A5).all()
    assert lib.dvp_debug_msm_capture_fetch(None, 0, C.byref(need)) == -1  # consumed
    dvp.check(lib.dvp_debug_msm_capture_arm(ARENA))
    assert np_to_pt(*fb.run(s_np)) == exp
    assert np_to_pt(*fb.run(s_np)) == exp  # not armed any more: the capture still holds the first of the two
    dvp.check(lib.dvp_debug_msm_capture_fetch(None, 0, C.byref(need)))
    assert need.value > 4096
    assert lib.dvp_debug_msm_capture_fetch(buf.ctypes.data, buf.nbytes, C.byref(need)) == -1 and (buf == 0xA5A5A5A5).all()
    big = np.zeros(need.value // 4, dtype=np.uint32)
    dvp.check(lib.dvp_debug_msm_capture_fetch(big.ctypes.data, big.nbytes, C.byref(need)))
    assert sc.parse_capture(big).hdr["n"] == len(logs)
    assert lib.dvp_debug_msm_capture_fetch(None, 0, C.byref(need)) == -1  # consumed
    # the same launches and host waits, armed or not
    counts = []
    for armed in (0, 1):
        lib.dvp_profile_reset()
        if armed:
            _, cap = capture(dvp, lambda: fb.run(s_np))
        else:
            fb.run(s_np)
        waits = []
        for name in (b"host_waits_stream", b"host_waits_side"):
            ms, n = C.c_double(0), C.c_uint64(0)
            dvp.check(lib.dvp_profile_read(name, C.byref(ms), C.byref(n)))
            waits.append(int(n.value))
        counts.append((census(dvp, ("msm.hip:",)), waits))
    assert counts[0] == counts[1] and sum(counts[0][0].values()) > 10
