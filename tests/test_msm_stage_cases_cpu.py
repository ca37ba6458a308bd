"""CPU tests of tests/msm_stage_cases.py: the stage restatements against each other and against the oracle, on synthetic captures (the
pipeline run by the restatements themselves, the points from c_oracle.k233_mulgen) -- so that what test_gpu_msm_stages.py holds the
device to is itself pinned, and its checker is known to refuse a capture that is wrong in one word."""
import random

import numpy as np
import pytest

import pyref as o
import c_oracle as co
import msm_stage_cases as sc
from util import to_limbs, pts_to_np

R = o.P


def make_hdr(flavour, c, n, dense=0, tpb=256, bmin=1):
    """the header of an MSM over n bases used whole: flavour 3 = fixed-base signed windows, 1 = fixed-base tau-adic, 0 = one-shot"""
    W, nn = sc.window_split(c)
    if flavour == 1:
        W += 1  # one overflow window
    elif flavour == 0:
        W += (240 - 234 + c - 1) // c
    nkeys = 1 << (c - 1) if flavour == 3 else (1 << c if flavour == 1 else W << c)
    return dict(magic=sc.MAGIC, version=sc.VERSION, hdr_words=sc.HDR_WORDS, flavour=flavour, c=c, W=W, n_narrow=nn, nkeys=nkeys,
                sign_mask=0x80000000 if flavour == 3 else 0, n_total=n, i0=0, n=n, ra=0, ra_plan=40, dense=dense, pipeline=2 if dense else 0,
                tpb=tpb, aff_cap=196608, bmax=136, bmin=bmin, route=1, K=8, max_cnt=0, items_len=0)


def inputs(n, seed):
    rnd = random.Random(seed)
    logs = [rnd.randrange(1, R) for _ in range(n)]
    # equal and opposite bases and repeated scalars: buckets with P + P, P - P and, a round later, neutral operands
    for i in range(0, n - 3, 4):
        logs[i + 1] = logs[i]
        logs[i + 2] = R - logs[i]
    vals = [rnd.randrange(R) for _ in range(3)] + [1, 5, 64, 65, 127, 128, 129, 255]
    scalars = [rnd.choice(vals) for _ in range(n)]
    return logs, scalars


MG = sc.Mulgen()


@pytest.mark.parametrize("flavour,c,dense", [(3, 8, 0), (3, 8, 1), (1, 8, 0), (0, 4, 0), (0, 4, 1)])
def test_synthetic_capture_passes_and_sums_to_the_oracle_msm(flavour, c, dense):
    """membership, layout, bookkeeping (both descriptor forms), group law and bucket weights agree with each other, and the weighted sum
    over the buckets is the oracle's MSM of the same scalars and bases"""
    n = 48
    logs, scalars = inputs(n, 100 + flavour)
    hdr = make_hdr(flavour, c, n, dense)
    mem = sc.membership(hdr, scalars)
    ra = max(max(sum(v.values()) for v in mem.values()) - 1, 0).bit_length()
    cap = sc.synthetic_capture(hdr, logs, scalars, random.Random(7), ra, MG)
    classes, bucket_logs = sc.check_capture(cap, logs, scalars, mulgen=MG)
    assert len(classes) == ra and all(len(cl) == t for cl, t in zip(classes, cap.hdr["total"]))
    total = sc.weighted_sum(cap.hdr, bucket_logs)
    assert total == sum(s * k for s, k in zip(scalars, logs)) % R
    bases = pts_to_np([co.k233_mulgen(k) for k in logs])
    assert co.k233_mulgen(total) == co.msm(to_limbs(scalars), bases)
    seen = {x for cl in classes for x in cl}
    assert seen <= set(sc.CLASSES) and "generic" in seen and seen & {"P+P", "P-P"}, seen  # (which exceptional ones: the drawn order's business)
    # the last round leaves one point per bucket
    assert max(int(x) for x in cap.rounds[-1]["ocnt"]) == 1


def test_checker_refuses_one_wrong_word():
    """a capture that differs from a right one in one place fails at the stage that place belongs to"""
    n = 48
    logs, scalars = inputs(n, 103)
    hdr = make_hdr(3, 8, n, 1)
    good = lambda: sc.synthetic_capture(hdr, logs, scalars, random.Random(9), 3, MG)
    sc.check_capture(good(), logs, scalars, mulgen=MG)

    def refused(mutate, stage):
        cap = good()
        mutate(cap)
        with pytest.raises(AssertionError) as ei:
            sc.check_capture(cap, logs, scalars, mulgen=MG)
        assert ei.value.args and ei.value.args[0][0] == stage, ei.value.args

    def flip_point(cap):
        pts = cap.rounds[1]["pts"].copy()
        pts[2, 3] ^= 1
        cap.rounds[1]["pts"] = pts

    def swap_items(cap):  # an item in the neighbouring bucket
        k = next(k for k in range(1, hdr["nkeys"] - 1) if cap.cnt[k] and cap.cnt[k + 1])
        a, b = int(cap.off[k]), int(cap.off[k + 1])
        cap.items[a], cap.items[b] = cap.items[b], cap.items[a]

    def bad_desc(cap):
        d = cap.rounds[2]["desc"]
        d[0], d[2] = d[2], d[0]

    def bad_spare(cap):
        k = next(k for k in range(hdr["nkeys"]) if cap.cnt[k] & 1)
        cap.items[int(cap.off[k]) + int(cap.cnt[k])] = 0

    def bad_bucket(cap):
        k = next(k for k in range(hdr["nkeys"]) if cap.cnt[k])
        cap.bkt[k, 8] ^= 2

    def bad_count(cap):
        cap.rounds[0]["ocnt"][1] += 1

    refused(flip_point, "pair round")
    refused(swap_items, "sort")
    refused(bad_spare, "sort")
    refused(bad_desc, "bookkeeping")
    refused(bad_count, "bookkeeping")
    refused(bad_bucket, "leftovers")


def test_dense_and_word_descriptors_describe_the_same_pairing():
    rnd = random.Random(5)
    for _ in range(50):
        c_in = [rnd.choice([0, 0, 1, 2, 3, 4, 5, 8, 33]) for _ in range(rnd.randrange(1, 40))]
        o_in, at = [], 0
        for c in c_in:
            o_in.append(at)
            at += c
        o_in.append(at)
        c_out, o_out = sc.halve(c_in)
        total = o_out[-1]
        word = sc.round_slots(dict(dense=0), 1, sc.desc_words(c_in, o_in, o_out), total)
        dense = sc.round_slots(dict(dense=1), 1, sc.desc_dense(c_in, o_in, o_out), total)
        assert sorted(word) == sorted(dense, key=lambda t: t[2]) == [(a, b, s) for s, (a, b, _) in enumerate(word)]
        # additions first, leftovers behind them
        npair = sum(1 for _, b, _ in dense if b is not None)
        assert all((b is not None) == (s < npair) for s, (_, b, _) in enumerate(dense))
        # every input is read exactly once
        used = sorted(x for a, b, _ in dense for x in ((a,) if b is None else (a, b)))
        assert used == list(range(o_in[-1]))


def test_sort_layout_and_halving():
    assert sc.sort_offsets([0, 1, 2, 3, 0, 5]) == [0, 0, 2, 4, 8, 8, 14]
    assert sc.halve([0, 1, 2, 3, 33]) == ([0, 1, 1, 2, 17], [0, 0, 1, 2, 4, 21])
    assert sc.desc_words([3, 2], [0, 3, 5], [0, 2, 3]) == [0 | sc.PAIR, 2, 3 | sc.PAIR]


def test_classifier_on_hand_made_slots():
    a, b = 12345, 999
    assert sc.classify(a, b) == "generic"
    assert sc.classify(a, a) == "P+P"
    assert sc.classify(a, R - a) == "P-P"
    assert sc.classify(0, b) == "O+Q"
    assert sc.classify(a, 0) == "P+O"
    assert sc.classify(0, 0) == "O+O"
    assert sc.classify(a, None) == "leftover"
    assert sc.classify(0, None) == "leftover O"
    assert set(sc.CLASSES) == {sc.classify(*t) for t in ((a, b), (a, a), (a, R - a), (0, b), (a, 0), (0, 0), (a, None), (0, None))}


def test_slot_geometry():
    cap = 196608
    # a small round is one chip-full of one slot per thread, unless bmin asks for more
    assert sc.slots_per_thread(650, cap, 136, 1) == 1 and sc.slots_per_thread(650, cap, 136, 3) == 3
    # 2.2 chip-fulls of 48 at bmax = 48: three chip-fulls, ceil(106 / 3) slots each
    assert sc.slots_per_thread(106 * cap, cap, 48, 1) == 36
    assert sc.slots_per_thread(65 * cap, cap, 136, 8) == 65 and sc.slots_per_thread(137 * cap, cap, 136, 8) == 69
    assert sc.slots_per_thread(0, cap, 136, 1) == 1
    for total, B, tpb in ((650, 1, 256), (650, 3, 128), (7, 3, 64), (1, 1, 64), (1301, 3, 256)):
        pos = [sc.slot_position(s, total, B, tpb) for s in range(total)]
        nthr = -(-total // B)
        assert all(p.nthr == nthr and p.thread < nthr and p.chain < B for p in pos)
        assert len({(p.thread, p.chain) for p in pos}) == total
        assert all(p.thread == p.wg * tpb + p.wave * 64 + p.lane and p.lane < 64 and p.wave < tpb // 64 for p in pos)
        # lane-consecutive slots: a thread's k-th slot is k * nthr + thread
        assert all(s == p.chain * nthr + p.thread for s, p in enumerate(pos))


def test_signed_recode_and_tau_windows():
    rnd = random.Random(11)
    for c in (8, 13, 20):
        W, nn = sc.window_split(c)
        assert sum(sc.window_widths(c, W, nn)) == 234
        for x in [0, 1, (1 << (c - 1)), (1 << c) - 1, R - 1] + [rnd.randrange(R) for _ in range(50)]:
            exp = sc.signed_recode(x, c)
            assert [o_w for o_w, _ in exp] == sc.window_starts(c, W, nn)
            assert all(abs(d) <= 1 << (wd - 1) for (_, d), wd in zip(exp, sc.window_widths(c, W, nn)))
    assert (sc.LAMBDA * sc.LAMBDA + sc.LAMBDA + 2) % R == 0
    for x in [1, 2, R - 1] + [rnd.randrange(R) for _ in range(20)]:
        W, nn = sc.window_split(8)
        pats = sc.tau_windows(x, 8, W + 1, nn)
        assert sum(sc.pattern_weight(d, o_w) for d, o_w in zip(pats, sc.window_starts(8, W + 1, nn))) % R == x


class _Order:
    """an order inside every bucket: the sorted one, its reverse, or drawn"""

    def __init__(self, kind):
        self.kind, self.rnd = kind, random.Random(31)

    def shuffle(self, lst):
        if self.kind == "reversed":
            lst.reverse()
        elif self.kind == "drawn":
            self.rnd.shuffle(lst)


@pytest.mark.parametrize("order", ["sorted", "reversed", "drawn"])
@pytest.mark.parametrize("dense,bmin", [(0, 1), (1, 1), (0, 3), (1, 3)])
def test_placement_input_reaches_the_named_positions(dense, bmin, order):
    """placement_input's bucket counts put exceptional pairs at every named position of the first round for the three workgroup sizes,
    under three different orders inside the buckets, and the class coverage condition holds for each of them"""
    logs, scalars, regions = sc.placement_input()
    assert len(logs) <= 1200 and max(scalars) < 1 << 8
    for tpb in (64, 128, 256):
        hdr = make_hdr(3, sc.PLACE_C, len(logs), dense, tpb=tpb, bmin=bmin)
        cap = sc.synthetic_capture(hdr, logs, scalars, _Order(order), 6, MG)
        assert cap.hdr["max_cnt"] == 33 and cap.hdr["total"][0] == 600
        classes, bucket_logs = sc.check_capture(cap, logs, scalars, mulgen=MG)
        sc.assert_placement(cap.hdr, classes)
        assert sc.weighted_sum(cap.hdr, bucket_logs) == sum(s * k for s, k in zip(scalars, logs)) % R
    # only the two lowest windows are populated
    rows = {(int(w) & 0x7FFFFFFF) // len(logs) for w in cap.items if int(w) != sc.NONE}
    assert rows == {0, 1} and any(int(w) >> 31 and int(w) != sc.NONE for w in cap.items)


# ---- the merge tree and the tails (capture version 2) ----------------------------------------------------------------------------

def test_normalisers_agree_with_the_oracle_points():
    """a point in lambda-projective and in Lopez-Dahab coordinates with Z != 1 normalises to the oracle's (x, y), one by one and through
    the shared inversion; Z = 0 is the marker (0, 0)"""
    rnd = random.Random(3)
    rows_lam, rows_ld, want = [], [], []
    for k in (1, 2, 3, R - 1, rnd.randrange(R)):
        x, y = co.k233_mulgen(k)
        z = rnd.getrandbits(233) | 1
        rows_lam.append(np.concatenate([sc.int_to_words(co.gf_mul(x, z)), sc.int_to_words(co.gf_mul(x ^ co.gf_mul(y, co.gf_inv(x)), z)), sc.int_to_words(z)]))
        rows_ld.append(np.concatenate([sc.int_to_words(co.gf_mul(x, z)), sc.int_to_words(co.gf_mul(y, co.gf_mul(z, z))), sc.int_to_words(z)]))
        want.append(x.to_bytes(32, "little") + y.to_bytes(32, "little"))
    zero = np.concatenate([sc.int_to_words(5), sc.int_to_words(7), sc.int_to_words(0)])
    assert [sc.lam_to_affine_bytes(r) for r in rows_lam] == want == [sc.ld_to_affine_bytes(r) for r in rows_ld]
    assert sc.to_affine_many(rows_lam + [zero], lam=True) == want + [bytes(64)] == sc.to_affine_many(rows_ld + [zero], lam=False)
    assert sc.lam_to_affine_bytes(zero) == bytes(64) and sc.to_affine_many([], lam=True) == []


def test_merge_levels_end_in_totals_and_bit_sums():
    """the level rule, applied level after level, keeps the invariant and ends with slot 0 = the total and slot 1 + t = the sum of the
    buckets with bit t set; its additions are numbered block (j + 1) + slot"""
    rnd = random.Random(17)
    start = [rnd.randrange(R) for _ in range(64)]
    logs = list(start)
    for j in range(5):  # blocks of 32: two of them
        logs, adds = sc.merge_level(logs, j)
        sc.assert_merge_invariant(start, logs, j)
        assert len(adds) == (64 >> (j + 1)) * (j + 1)
    for b in (0, 32):
        assert logs[b] == sum(start[b:b + 32]) % R
        assert all(logs[b + 1 + t] == sum(start[b + i] for i in range(32) if (i >> t) & 1) % R for t in range(5))
    with pytest.raises(AssertionError):
        sc.assert_merge_invariant(start, logs[:5] + [logs[5] ^ 1] + logs[6:], 4)
    # level 1 of one block of four: (b0 + b1) + (b2 + b3), b1 + b3, T_right = b2 + b3
    l0, _ = sc.merge_level([1, 2, 4, 8], 0)
    l1, adds = sc.merge_level(l0, 1)
    assert l0 == [3, 2, 12, 8] and adds == [(3, 12), (2, 8)] and l1 == [15, 10, 12, 8]


def test_tail_points_and_add_tree():
    """the signed tail weighs slot 1 + t by 2^t and bucket 0 by 2^(c-1); the Frobenius tail weighs slot 1 + t of window w by lambda^(o_w
    + t); the add tree pairs neighbours and passes an unpaired last entry on"""
    hdr = make_hdr(3, 8, 4)
    A = list(range(100, 228))
    assert sc.tail_points(hdr, A, 7) == [(A[1 + t] << t) % R for t in range(7)] + [7 << 7]
    hdr = make_hdr(0, 4, 4)
    A = list(range(1, hdr["nkeys"] + 1))
    pts = sc.tail_points(hdr, A, 0)
    starts = sc.window_starts(4, hdr["W"], hdr["n_narrow"])
    assert len(pts) == hdr["W"] * 4 and all(pts[4 * w + t] == A[16 * w + 1 + t] * pow(sc.LAMBDA, starts[w] + t, R) % R for w in range(hdr["W"]) for t in range(4))
    hdr = make_hdr(1, 8, 4)
    assert sc.tail_points(hdr, list(range(256)), 0) == [(1 + t) * pow(sc.LAMBDA, t, R) % R for t in range(8)]
    total, levels = sc.add_tree([5, 5, 3, R - 3, 0, 9, 4, 0, 0, 0, 11])
    assert total == 34 and levels[0] == ["P+P", "P-P", "O+Q", "P+O", "O+O", "leftover"] and levels[1] == ["P+O", "generic", "O+Q"]
    assert levels[2] == ["generic", "leftover"] and levels[3] == ["generic"] and sc.add_tree([]) == (0, []) and sc.add_tree([4]) == (4, [])


@pytest.mark.parametrize("flavour,c,tail,enc,rule", [(3, 8, 0, 1, 0), (3, 8, 1, 0, 0), (3, 11, 0, 1, 1), (1, 8, 2, 1, 0), (0, 4, 3, 1, 0), (0, 4, 2, 0, 0)])
def test_synthetic_version_2_capture(flavour, c, tail, enc, rule):
    """synthetic_capture's merge levels, save0, group sums and result are accepted, the total is the oracle's MSM, and check_capture
    returns the merge and tail classes beside the pair it always returned"""
    n = 40
    logs, scalars = inputs(n, 200 + flavour + c)
    hdr = dict(make_hdr(flavour, c, n), tail=tail, enc=enc, rule=rule)
    cap = sc.synthetic_capture(hdr, logs, scalars, random.Random(2), 2, MG)
    res = sc.check_capture(cap, logs, scalars, mulgen=MG)
    classes, bucket_logs = res
    levels = c - 1 if flavour == 3 else c
    assert len(res.merge) == levels == cap.hdr["levels"] and all(len(res.merge[j]) == (cap.hdr["nkeys"] >> (j + 1)) * (j + 1) for j in range(levels))
    assert res.total == sum(s * k for s, k in zip(scalars, logs)) % R == sc.weighted_sum(cap.hdr, bucket_logs)
    assert res.tail["shape"] == tail and (res.tail["groups"] is not None) == (tail == 3)
    assert len(res.tail["points"]) == (c if flavour & 1 else cap.hdr["W"] * c)
    if tail == 3:
        assert cap.hdr["nparts"] == (cap.hdr["W"] * c + 15) // 16 == len(res.tail["parts"])
    assert (cap.res_enc is not None) == bool(enc) and (cap.save0 is not None) == (flavour == 3)
    assert {x for lv in res.merge for x in lv} <= set(sc.MERGE_CLASSES)


def test_checker_refuses_one_wrong_word_behind_the_buckets():
    """a capture that differs from a right one in one word of a merge level, of save0, of a group sum, of the result or of the encoding is
    refused with that stage named; so is a T_right that a level did not hand over (slot j + 1 stale, j != 1), a save0 that holds the
    merged slot 0 instead of bucket 0, and an infinity word that contradicts the point"""
    n = 40

    def refused(hdr, logs, scalars, mutate, stage, where=()):
        cap = sc.synthetic_capture(hdr, logs, scalars, random.Random(9), 2, MG)
        sc.check_capture(cap, logs, scalars, mulgen=MG)
        mutate(cap)
        with pytest.raises(AssertionError) as ei:
            sc.check_capture(cap, logs, scalars, mulgen=MG)
        args = ei.value.args[0]
        assert args[0] == stage and args[1:1 + len(where)] == where, args

    logs, scalars = inputs(n, 301)
    signed = dict(make_hdr(3, 8, n), enc=1)

    def flip(section, *idx):
        def f(cap):
            a = getattr(cap, section)
            if idx[:-1]:
                a = a[idx[0]] if len(idx) == 2 else a[idx[0]][idx[1]]
            a[idx[-1]] ^= 4
        return f

    # level 3, block 2 (slots 32 ..), slot 1: a slot the level wrote; a slot it did not write is not compared at that level
    refused(signed, logs, scalars, flip("levels", 3, 33, 2), "merge", ("level", 3, "block", 2, "slot", 1))
    refused(signed, logs, scalars, flip("levels", 0, 127, 20), "merge", ("level", 0, "block", 63, "slot", 1))
    refused(signed, logs, scalars, flip("save0", 9), "save0")
    refused(signed, logs, scalars, flip("res_xy", 15), "result", ("xy",))

    def flip_inf(cap):
        cap.res_inf ^= 1

    def flip_enc(cap):
        cap.res_enc = cap.res_enc[:29] + bytes([cap.res_enc[29] ^ 1])

    refused(signed, logs, scalars, flip_inf, "result", ("inf",))
    refused(signed, logs, scalars, flip_enc, "encoding")
    for j in (0, 2, 4, 6):  # slot j + 1 of block 0 as the level before left it
        def stale(cap, j=j):
            cap.levels[j][j + 1] = cap.levels[j - 1][j + 1] if j else np.concatenate([cap.bkt[1][:16], sc.int_to_words(1)])
        refused(signed, logs, scalars, stale, "merge", ("level", j, "block", 0, "slot", j + 1, "T_right"))

    def merged_slot0(cap):  # what slot 0 holds after level 0 (b0 + b1), as a Lopez-Dahab point
        k = (sc.check_capture(cap, logs, scalars, mulgen=MG)[1][0] + sc.check_capture(cap, logs, scalars, mulgen=MG)[1][1]) % R
        cap.save0 = np.concatenate([np.frombuffer(MG.words(k), dtype="<u4"), sc.int_to_words(1)])

    refused(signed, logs, scalars, merged_slot0, "save0")
    one_shot = dict(make_hdr(0, 4, n), enc=1, rule=1)
    l2, s2 = inputs(n, 302)
    refused(one_shot, l2, s2, flip("parts", 5, 1), "tail groups", ("group", 5))
    refused(one_shot, l2, s2, flip("parts", 15, 17), "tail groups", ("group", 15))
    def flip_t_right(cap):  # the first finite T_right of level 3
        i = next(i for i in range(4, cap.hdr["nkeys"], 16) if cap.levels[3][i][16:].any())
        cap.levels[3][i][0] ^= 1
    refused(one_shot, l2, s2, flip_t_right, "merge", ("level", 3))
    refused(one_shot, l2, s2, flip_enc, "encoding", ("rule", 1))
    # a header that names another tail shape than the flavour can run
    def wrong_shape(cap):
        cap.hdr["tail"] = 0
    refused(one_shot, l2, s2, wrong_shape, "tail")


# ---- placed inputs for the merge tree and the tails --------------------------------------------------------------------------------

ONE_SHOT_MERGE = dict(require=("classes", "groups", "neighbours", "slots"), require_first=("classes", "neighbours"))


def placed_capture(flavour, c, bucket_logs, **hdr_extra):
    """the synthetic capture of the MSM placed_scalars builds for these bucket logarithms: no pair round, one item per bucket"""
    base_logs, scalars, keys = sc.placed_scalars(flavour, c, bucket_logs)
    hdr = dict(make_hdr(flavour, c, len(base_logs)), route=0, **hdr_extra)
    assert (hdr["W"], hdr["n_narrow"], hdr["nkeys"]) == sc.plan_windows(flavour, c)
    cap = sc.synthetic_capture(hdr, base_logs, scalars, random.Random(1), 0, MG)
    return cap, base_logs, scalars


@pytest.mark.parametrize("flavour,c", [(3, 8), (3, 11), (0, 4)])
def test_merge_placement_is_reached_by_the_restatement_alone(flavour, c):
    """merge_placed_logs through placed_scalars (every scalar's window property asserted there, with the signed recoding or the oracle's
    tau-adic digits) puts the chosen logarithm into every bucket, and the schedule meets assert_merge_placement for 1, 4 and 16 lanes
    per addition: in full at 128 buckets; at 1 024 all but a last addition in a partly filled workgroup of level 0 (two full ones), with
    level 2's last addition, the last lane of workgroup 0 and the first of workgroup 1 named; one-shot at c = 4 what its windows allow"""
    runs = []
    for variant in ("pp", "mm", "o0"):
        want = sc.merge_placed_logs(flavour, c, variant)
        cap, base_logs, scalars = placed_capture(flavour, c, want)
        assert cap.hdr["max_cnt"] == 1
        res = sc.check_capture(cap, base_logs, scalars, mulgen=MG)
        assert res[1] == want and res.merge == sc.merge_classes(flavour, c, want)
        runs.append(res.merge)
    for G in (1, 4, 16):
        with_g = [([G] * len(m), m) for m in runs]
        if flavour == 0:
            found = sc.assert_merge_placement(with_g, **ONE_SHOT_MERGE)
        elif c == 8:
            found = sc.assert_merge_placement(with_g)
        else:
            found = sc.assert_merge_placement(with_g, require_first=tuple(x for x in sc.MERGE_CONDITIONS if x != "last addition"))
        assert set(found) == {(G, True), (G, False)}
    if c == 11:
        assert 384 % 256 and [m[2][383] for m in runs] == ["P+P", "P+O", "P-P"]
        assert [(m[0][255], m[0][256]) for m in runs] == [("P+P", "P+P"), ("P-P", "P-P"), ("P+P", "P+P")]
    if flavour == 3:  # addition 0 of level 0, the lane that keeps bucket 0 aside
        assert [m[0][0] for m in runs] == ["P+P", "P-P", "O+Q"]


def test_merge_placement_fails_when_a_class_is_missing():
    rnd = random.Random(4)
    merge = sc.merge_classes(3, 8, [rnd.randrange(1, R) for _ in range(128)])
    assert {x for lv in merge for x in lv} == {"generic"}
    with pytest.raises(AssertionError):
        sc.assert_merge_placement([([16] * 7, merge)])
    good = [([4] * 7, sc.merge_classes(3, 8, sc.merge_placed_logs(3, 8, v))) for v in ("pp", "mm", "o0")]
    sc.assert_merge_placement(good)
    for drop in ("pp", "mm", "o0"):  # every variant is needed
        with pytest.raises(AssertionError):
            sc.assert_merge_placement([g for g, v in zip(good, ("pp", "mm", "o0")) if v != drop])


TAIL_SHAPES = [(3, 8, 0), (3, 8, 1), (3, 11, 0), (3, 11, 1), (1, 8, 2), (0, 4, 2), (0, 4, 3), (0, 6, 3)]


@pytest.mark.parametrize("flavour,c,shape", TAIL_SHAPES)
def test_tail_placement_is_reached_by_the_restatement_alone(flavour, c, shape):
    """tail_targets through tail_placed_logs and placed_scalars makes the tail's points exactly the targets, and the four variants meet
    assert_tail_placement for every tail shape.  Parity is met by c = 8 and c = 11 together.  The single-workgroup Frobenius tail of a
    one-shot MSM has its last first-level pair in the overflow windows, which no scalar reaches.  W c is a multiple of 16 at c = 6 only
    (c = 4 .. 15: 244, 245, 240, 245, 248, 243, 250, 253, 252, 247, 252, 255): there the last group is full"""
    runs = []
    for variant in sc.TAIL_VARIANTS if c != 6 else ("a",):
        E = sc.tail_targets(flavour, c, variant)
        cap, base_logs, scalars = placed_capture(flavour, c, sc.tail_placed_logs(flavour, c, E), tail=shape, enc=1, rule=variant == "b")
        res = sc.check_capture(cap, base_logs, scalars, mulgen=MG)
        assert res.tail["points"] == E and res.tail["shape"] == shape and (res.total == 0) == (variant == "z")
        runs.append(res.tail)
    if c == 6:
        assert len(E) % 16 == 0 and [W * cc % 16 == 0 for cc in range(4, 16) for W in [sc.plan_windows(0, cc)[0]]] == [cc == 6 for cc in range(4, 16)]
        return
    skip = {"parity"} | ({"last pair"} if (flavour, shape) == (0, 2) else set())
    found = sc.assert_tail_placement(runs, tuple(x for x in sc.TAIL_CONDITIONS if x not in skip))
    assert found["parity"] == [c & 1 if flavour & 1 else 0]
    with pytest.raises(AssertionError):  # the variants are needed: "a" alone has no neutral result
        sc.assert_tail_placement(runs[:1], ("result",))
    if flavour == 3 and shape == 0:
        both = runs + [sc.tail_restated(dict(flavour=3, c=19 - c), sc.merged_array(3, 19 - c, sc.tail_placed_logs(3, 19 - c, sc.tail_targets(3, 19 - c, "a"))), 1, 0)]
        sc.assert_tail_placement(both)
