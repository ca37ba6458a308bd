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
    return dict(magic=sc.MAGIC, version=1, hdr_words=sc.HDR_WORDS, flavour=flavour, c=c, W=W, n_narrow=nn, nkeys=nkeys,
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
