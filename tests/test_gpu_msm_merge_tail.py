"""GPU tests (-m gpu): the back end of the MSM -- k_merge<1 | 4 | 16, FIRST>, k_tail_groups, k_tail<true | false> -- level by level on
placed inputs.  tests/msm_stage_cases.py builds MSMs with ONE base per bucket whose logarithm is chosen (placed_scalars), so that what
every addition of every merge level and of the tails' add trees meets -- P + P, P - P, a neutral operand on either side or both, and in
which lane group, wave and workgroup -- is laid out beforehand (merge_placed_logs, tail_targets) and proven on the logarithms alone by
the CPU suite.  Here each such MSM runs with the stage capture armed; check_capture compares the bucket array behind every merge level,
bucket 0 kept aside, the group sums and the result (both entry kinds: the affine point, and the 30-byte encoding the tail kernel makes
from the inversion it shares with the affine conversion) bit for bit with the oracle; assert_merge_placement / assert_tail_placement
demand the class coverage from the classes the capture yielded; the launch census proves which instantiation ran."""
import ctypes as C

import numpy as np
import pytest

import pyref as o
import c_oracle as co
import msm_stage_cases as sc
from msm_cases import assert_census
from util import to_limbs, np_to_pt

pytestmark = pytest.mark.gpu
M = "msm.hip:"
# lanes per addition of EVERY merge level (all levels here have between 2 and 512 additions), and the signed tail that comes with it
LANES = {16: dict(DVP_MSM_HEX_MAX=1 << 30), 4: dict(DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=1 << 30), 1: dict(DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=1)}
MERGES = [f"{M}k_merge<{g},{f}>" for g in (1, 4, 16) for f in ("true", "false")]
TAIL_KERNELS = {0: ["k_tail<true>"], 1: ["k_tail<false>"], 2: ["k_tail<false>"], 3: ["k_tail_groups", "k_tail<false>"]}
ALL_TAILS = ["k_tail<true>", "k_tail<false>", "k_tail_groups"]


ARENA = 96 << 20


def capture(dvp, run):
    """arms the calling thread's next MSM, runs it, fetches and parses its capture: (what run() returned, Capture)"""
    lib = dvp.lib
    dvp.check(lib.dvp_debug_msm_capture_arm(ARENA), "arm")
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


class Placed:
    """the placed MSMs of one flavour and window size: name -> (first base, last base + 1, scalars, bucket logarithms); fixed-base: ONE
    context over all their bases side by side, an MSM runs over its own range of it"""

    def __init__(self, dvp, flavour, c, logs_by_name, **create_knobs):
        self.dvp, self.flavour, self.c, self.runs, self.base_logs = dvp, flavour, c, {}, []
        for name, bucket_logs in logs_by_name.items():
            logs, scalars, _ = sc.placed_scalars(flavour, c, bucket_logs)
            self.runs[name] = (len(self.base_logs), len(self.base_logs) + len(logs), scalars, bucket_logs)
            self.base_logs += logs
        self.bases, inf = dvp.curve.point_scalar_mul_gen_batch(to_limbs(self.base_logs))
        assert not inf.any()
        self.fb = None
        if flavour & 1:
            with dvp.tune(DVP_MSM_FIXED_C=c, **create_knobs):
                self.fb = dvp.curve.FixedBaseMsm(self.bases)
            assert self.fb.plan() == (c, sc.plan_windows(flavour, c)[0]) and self.fb.table()[1] == (flavour == 3)

    def close(self):
        if self.fb:
            self.fb.close()

    def run(self, name, knobs, mg, enc_rule=None, tail=None, lanes=None):
        """one captured MSM under `knobs`; enc_rule = None: the affine entry, else the entry that also returns the 30-byte encoding, under
        that codec rule.  Compares the returned point (and encoding) with the oracle, the header with the plan, the census with the
        kernels `lanes` / `tail` name, and runs check_capture -> (header, Checked)"""
        dvp, lib = self.dvp, self.dvp.lib
        lo, hi, scalars, bucket_logs = self.runs[name]
        s_np = to_limbs(scalars)
        where = (self.flavour, self.c, name, knobs, enc_rule)

        def go():
            if enc_rule is None:
                if self.fb:
                    return np_to_pt(*self.fb.run(s_np, lo, hi)), None
                return np_to_pt(*dvp.curve.multi_scalar_mul(s_np, self.bases[lo:hi])), None
            xy, is_inf, enc = np.zeros(8, dtype=np.uint64), C.c_int(0), np.zeros(30, dtype=np.uint8)
            b = np.ascontiguousarray(self.bases[lo:hi])
            args = (self.fb._h, s_np.ctypes.data, None, lo, hi) if self.fb else (None, s_np.ctypes.data, b.ctypes.data, 0, hi - lo)
            dvp.check(lib.dvp_debug_msm_enc(*args, xy.ctypes.data, C.byref(is_inf), enc.ctypes.data), "dvp_debug_msm_enc")
            return np_to_pt(xy, bool(is_inf.value)), enc.tobytes()

        dvp.check(lib.dvp_codec_set_rule(enc_rule or 0))
        try:
            with dvp.tune(**({} if self.fb else dict(DVP_MSM_C=self.c)), **knobs):
                lib.dvp_profile_reset()
                (got, enc), cap = capture(dvp, go)
                if lanes is not None:
                    ran = [f"{M}k_merge<{lanes},true>", f"{M}k_merge<{lanes},false>"]
                    assert_census(dvp, ran, [m for m in MERGES if m not in ran], where)
                if tail is not None:
                    assert_census(dvp, [M + k for k in TAIL_KERNELS[tail]], [M + k for k in ALL_TAILS if k not in TAIL_KERNELS[tail]], where)
        finally:
            dvp.check(lib.dvp_codec_set_rule(0))
        h = cap.hdr
        W, nn, nk = sc.plan_windows(self.flavour, self.c)
        assert (h["flavour"], h["c"], h["W"], h["n_narrow"], h["nkeys"], h["i0"], h["n"]) == (self.flavour, self.c, W, nn, nk, lo if self.fb else 0, hi - lo), (h, where)
        assert (h["ra"], h["max_cnt"], sc.ROUTES[h["route"]]) == (0, 1, "k_bucket_gather_items"), (h, where)
        assert (h["enc"], h["rule"]) == (int(enc_rule is not None), enc_rule or 0), (h, where)
        if lanes is not None:
            assert h["group"] == [lanes] * (self.c - 1 if self.flavour == 3 else self.c), (h, where)
        if tail is not None:
            assert h["tail"] == tail, (sc.TAILS[h["tail"]], where)
        try:
            res = sc.check_capture(cap, self.base_logs if self.fb else self.base_logs[lo:hi], scalars, mulgen=mg)
        except AssertionError as e:
            raise AssertionError((where,) + e.args) from e
        assert res[1] == [x % sc.R for x in bucket_logs], where  # every bucket holds the point that was placed there
        exp = None if res.total == 0 else co.k233_mulgen(res.total)
        assert got == exp, ("result", where)
        if enc_rule is not None:
            assert enc == sc.encode_point(res.total, enc_rule, mg) and (res.total != 0 or enc == bytes(30)), ("encoding", where)
        return h, res


def merge_runs(placed, mg, lanes):
    """the three variants under `lanes` lanes per addition: [(group, merge classes)]; "mm" goes through the encoding entry"""
    out = []
    for variant in ("pp", "mm", "o0"):
        h, res = placed.run(variant, LANES[lanes], mg, enc_rule=0 if variant == "mm" else None, lanes=lanes)
        assert res.merge == sc.merge_classes(placed.flavour, placed.c, placed.runs[variant][3])
        out.append((h["group"], res.merge))
    return out


@pytest.fixture(scope="module")
def merge_c8(dvp):
    p = Placed(dvp, 3, 8, {v: sc.merge_placed_logs(3, 8, v) for v in ("pp", "mm", "o0")})
    yield p
    p.close()


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_merge_tree_128_buckets(merge_c8, mg, lanes):
    """fixed-base signed digits at c = 8: seven levels, each inside one workgroup.  k_merge<lanes, true> and k_merge<lanes, false> meet
    every class; P + P and P - P at addition 0 (at level 0 the lane that also keeps bucket 0 aside: populated, and neutral in "o0") and
    at the last live addition of a partly filled workgroup; with 4 and 16 lanes P + P in the first group of a wave and the last of a
    workgroup, and one wave with P + P, P - P, a neutral operand and a generic addition side by side; behind level 0 P + P at slot 0 (the
    lane that hands T_right over) and at slot j, and an exceptional slot 0 at level 1, where T_right stays in place"""
    found = sc.assert_merge_placement(merge_runs(merge_c8, mg, lanes))
    assert set(found) == {(lanes, True), (lanes, False)}
    print(lanes, found)


@pytest.fixture(scope="module")
def merge_c11(dvp):
    p = Placed(dvp, 3, 11, {v: sc.merge_placed_logs(3, 11, v) for v in ("pp", "mm", "o0")})
    yield p
    p.close()


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_merge_tree_1024_buckets(merge_c11, mg, lanes):
    """fixed-base signed digits at c = 11: levels of 512 / 512 / 384 / .. additions -- with one lane per addition two workgroups and, at
    level 2, a half-filled second one whose last live lane adds P + P ("pp") and P - P ("o0"); the last lane of workgroup 0 and the
    first of workgroup 1 at level 0 are P + P and P - P.  (Level 0 fills its workgroups: no partly filled one there.)"""
    runs = merge_runs(merge_c11, mg, lanes)
    found = sc.assert_merge_placement(runs, require_first=tuple(x for x in sc.MERGE_CONDITIONS if x != "last addition"))
    assert set(found) == {(lanes, True), (lanes, False)}
    merges = [m for _, m in runs]
    assert len(merges[0][2]) == 384 and [m[2][383] for m in merges] == ["P+P", "P+O", "P-P"]
    assert [(m[0][255], m[0][256]) for m in merges] == [("P+P", "P+P"), ("P-P", "P-P"), ("P+P", "P+P")]


@pytest.fixture(scope="module")
def merge_one_shot(dvp):
    p = Placed(dvp, 0, 4, {v: sc.merge_placed_logs(0, 4, v) for v in ("pp", "mm", "o0")})
    yield p
    p.close()


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_merge_tree_one_shot_windows(merge_one_shot, mg, lanes):
    """one-shot at c = 4: 61 windows of 16 buckets, four levels of at most 488 additions over all windows at once, and the group sums of
    k_tail_groups behind them.  Pattern 0 of a window is no bucket, so addition 0 of level 0 cannot be placed (the signed shapes do
    that); everything else the windows allow is demanded"""
    runs = merge_runs(merge_one_shot, mg, lanes)
    found = sc.assert_merge_placement(runs, ("classes", "groups", "neighbours", "slots"), ("classes", "neighbours"))
    assert set(found) == {(lanes, True), (lanes, False)}


def tail_runs(placed, mg, knobs, shape, both_entries):
    """the four variants under one tail shape: the affine entry and the encoding entry (codec rule 1 for "b", else rule 0)"""
    out = []
    for variant in sc.TAIL_VARIANTS:
        entries = [None, int(variant == "b")] if both_entries else [None if variant in ("a", "c") else int(variant == "b")]
        for rule in entries:
            h, res = placed.run(variant, knobs, mg, enc_rule=rule, tail=shape)
            assert res.tail["points"] == sc.tail_targets(placed.flavour, placed.c, variant) and (res.total == 0) == (variant == "z")
        out.append(res.tail)
    return out


@pytest.fixture(scope="module")
def tails_signed(dvp):
    ps = [Placed(dvp, 3, c, {v: sc.tail_placed_logs(3, c, sc.tail_targets(3, c, v)) for v in sc.TAIL_VARIANTS}) for c in (8, 11)]
    yield ps
    for p in ps:
        p.close()


@pytest.mark.parametrize("shape,knobs", [(0, {}), (1, dict(DVP_MSM_HEX_MAX=0))])
def test_signed_tails(tails_signed, mg, shape, knobs):
    """k_tail<true> and (DVP_MSM_HEX_MAX = 0) k_tail<false> with n_narrow = -3, at c = 8 (eight points) and c = 11 (eleven: a leftover):
    an empty bit slot through its doublings, P + P and P - P at the first and the last pair of the first level (2^(t+1) A[2 + t] = 2^t
    A[1 + t]; at c = 8 the last pair's partner is bucket 0), a neutral operand on either side and on both, bucket 0 populated and empty,
    a finite result and a neutral one -- through the affine entry and through the encoding entry, codec rules 0 and 1"""
    runs = []
    for p in tails_signed:
        runs += tail_runs(p, mg, knobs, shape, both_entries=p.c == 8)
    found = sc.assert_tail_placement(runs)
    assert found["parity"] == [0, 1]
    print(sc.TAILS[shape], found)


@pytest.fixture(scope="module")
def tails_fixed_tau(dvp):
    p = Placed(dvp, 1, 8, {v: sc.tail_placed_logs(1, 8, sc.tail_targets(1, 8, v)) for v in sc.TAIL_VARIANTS}, DVP_MSM_ALIGNED_SIGNED=0)
    yield p
    p.close()


def test_frobenius_tail_fixed_base(tails_fixed_tau, mg):
    """the fixed-base tau-adic flavour (DVP_MSM_ALIGNED_SIGNED = 0) at c = 8: k_tail<false> alone over eight points lambda^t A[1 + t] of
    one bucket set of 256 -- the same classes as the signed tails, P + P from A[2 + t] = A[1 + t] / lambda"""
    runs = tail_runs(tails_fixed_tau, mg, {}, 2, both_entries=True)
    sc.assert_tail_placement(runs, tuple(x for x in sc.TAIL_CONDITIONS if x != "parity"))


@pytest.fixture(scope="module")
def tails_one_shot(dvp):
    p = Placed(dvp, 0, 4, {v: sc.tail_placed_logs(0, 4, sc.tail_targets(0, 4, v)) for v in sc.TAIL_VARIANTS})
    yield p
    p.close()


@pytest.mark.parametrize("shape,knobs", [(2, dict(DVP_MSM_TAIL_GROUPS=0)), (3, {})])
def test_one_shot_tails(tails_one_shot, mg, shape, knobs):
    """one-shot at c = 4, 244 points lambda^k A[(w << c) + 1 + t]: k_tail<false> alone (DVP_MSM_TAIL_GROUPS = 0) and k_tail_groups +
    k_tail<false> with n_narrow = -4 (16 group sums, each compared; the last group holds 4 points).  Groups: sixteen neutral points; a
    neutral sum through P - P; two neighbouring sums equal and two opposite, so the tree over the sums meets P + P and P - P.  The last
    pair of the single-workgroup tail's first level lies in the overflow windows, which no scalar reaches: it stays neutral"""
    runs = tail_runs(tails_one_shot, mg, knobs, shape, both_entries=False)
    skip = {"parity"} | ({"last pair"} if shape == 2 else set())
    found = sc.assert_tail_placement(runs, tuple(x for x in sc.TAIL_CONDITIONS if x not in skip))
    if shape == 3:
        assert found["groups"]["partly filled"] == [4] * 4 and runs[0]["parts"][5] == 0 == runs[0]["parts"][6]
        print(found["groups"])


def test_one_shot_tail_of_whole_groups(dvp, mg):
    """W c is a multiple of 16 for c = 6 alone among the widths the plan offers (c = 4 .. 15: 244, 245, 240, 245, 248, 243, 250, 253, 252,
    247, 252, 255): 40 windows, 15 full groups"""
    assert [cc for cc in range(4, 16) if sc.plan_windows(0, cc)[0] * cc % 16 == 0] == [6]
    p = Placed(dvp, 0, 6, {"a": sc.tail_placed_logs(0, 6, sc.tail_targets(0, 6, "a"))})
    h, res = p.run("a", {}, mg, enc_rule=0, tail=3)
    assert h["nparts"] == 15 and len(res.tail["points"]) == 240 and all(len(g[0]) == 8 for g in res.tail["groups"])
