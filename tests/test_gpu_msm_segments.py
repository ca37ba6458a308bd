"""GPU tests (-m gpu) of dvp_msm_segments: many independent multi_scalar_mul (src/curve.rs:141-158) over consecutive slices in one
call.  The reference value everywhere is the C oracle's reference-shaped MSM on each slice (c_oracle.msm: one scalar multiplication
per point plus complete additions), which shares nothing with the code under test; O is checked as inf == 1 with all-zero
coordinates.  Every segment of every case is compared.  Inputs and oracle sums are computed once per module and never changed."""
import ctypes as C
import random

import numpy as np
import pytest

import c_oracle as co
import point_cases as pc
import points_mul_cases as pm
from util import np_to_pt, pts_to_np, to_limbs

pytestmark = pytest.mark.gpu
R = pm.R
NONE64 = (1 << 64) - 1
EINVAL, EDECODE, EPOINT = -1, -2, -9
KNOB = b"DVP_MSM_SEG_PIECE"
PIECES = [None, 2, 3]  # None = the default in force
GARBAGE = (0x1234, 0x5678)  # what sits behind an infinity flag


class piece:
    """DVP_MSM_SEG_PIECE = p inside the block (None: left alone); the previous value comes back in a finally"""

    def __init__(self, dvp, p):
        self.dvp, self.p = dvp, p

    def __enter__(self):
        v = C.c_longlong(0)
        self.dvp.check(self.dvp.lib.dvp_tune_get(KNOB, C.byref(v)))
        self.prev = v.value
        if self.p is not None:
            self.dvp.check(self.dvp.lib.dvp_tune_set(KNOB, self.p))

    def __exit__(self, *exc):
        self.dvp.lib.dvp_tune_set(KNOB, self.prev)
        return False


def seg_ptr_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def oracle_sums(s, xy, inf, sp):
    """c_oracle.msm on every slice"""
    out = []
    for a, b in zip(sp[:-1], sp[1:]):
        a, b = int(a), int(b)
        out.append(co.msm(s[a:b], xy[a:b], None if inf is None else inf[a:b]))
    return out


def oracle_add(p, q):
    a, ai = co._pt_in(p)
    b, bi = co._pt_in(q)
    o = np.zeros(8, dtype=np.uint64)
    oi = C.c_int(0)
    co.lib().dvo_k233_add(co._p(a), ai, co._p(b), bi, co._p(o), C.byref(oi))
    return co._pt_out(o, oi)


def check_sums(xy, inf, want, what=""):
    assert xy.shape == (len(want), 8) and inf.shape == (len(want),)
    for j, w in enumerate(want):
        if w is None:
            assert inf[j] == 1 and not xy[j].any(), (what, j)
        else:
            assert inf[j] == 0 and np_to_pt(xy[j]) == w, (what, j)


def seeded_points(dvp, n, seed):
    rnd = random.Random(seed)
    xy, binf = dvp.curve.point_scalar_mul_gen_batch(to_limbs([rnd.randrange(1, R) for _ in range(n)]))
    assert not binf.any()
    return xy, [rnd.randrange(R) for _ in range(n)]


LENGTHS = [0, 1, 2, 63, 64, 65, 0, 0, 130, 257, 1, 0]


@pytest.fixture(scope="module")
def shapes(dvp):
    """the 583-point layout: empty segments first, last and adjacent, boundaries at and around wave edges; infinity flags at index 0,
    at n - 1 and at the first and last point of the 130-point segment, garbage coordinates behind them"""
    sp = seg_ptr_of(LENGTHS)
    n = int(sp[-1])
    assert n == 583
    xy, ks = seeded_points(dvp, n, 4100)
    xy = xy.copy()
    inf = np.zeros(n, dtype=np.uint8)
    for i in (0, n - 1, int(sp[8]), int(sp[9]) - 1):
        inf[i] = 1
        xy[i] = pts_to_np([GARBAGE])[0]
    s = to_limbs(ks)
    return dict(s=s, xy=xy, inf=inf, sp=sp, want=oracle_sums(s, xy, inf, sp))


@pytest.fixture(scope="module")
def one_segment(dvp):
    xy, ks = seeded_points(dvp, 1025, 4200)
    s = to_limbs(ks)
    return dict(s=s, xy=xy, want=co.msm(s, xy))


@pytest.fixture(scope="module")
def singletons(dvp):
    xy, ks = seeded_points(dvp, 257, 4300)
    ks[5] = 0
    s = to_limbs(ks)
    sp = np.arange(258, dtype=np.uint64)
    return dict(s=s, xy=xy, sp=sp, want=oracle_sums(s, xy, None, sp))


@pytest.fixture(scope="module")
def random_cut(dvp):
    """1000 points cut into 37 segments at seeded random places; segment 18 is not empty"""
    n, n_seg = 1000, 37
    xy, ks = seeded_points(dvp, n, 4400)
    rnd = random.Random(4401)
    sp = np.array([0] + sorted(rnd.randrange(n + 1) for _ in range(n_seg - 1)) + [n], dtype=np.uint64)
    assert sp[19] > sp[18]
    s = to_limbs(ks)
    return dict(s=s, ks=ks, xy=xy, sp=sp, want=oracle_sums(s, xy, None, sp), whole=co.msm(s, xy))


@pytest.fixture(scope="module")
def exceptional(dvp):
    """segments over two seeded points A = ka Pa, B = kb Pb: -A is (r - ka) Pa, a zero product is k = 0"""
    rnd = random.Random(4500)
    bases, _ = seeded_points(dvp, 2, 4501)
    ka, kb = rnd.randrange(1, R), rnd.randrange(1, R)
    term = {"A": (ka, 0), "-A": (R - ka, 0), "B": (kb, 1), "-B": (R - kb, 1), "O": (0, 0)}
    segs = [
        ["A", "A"], ["A", "-A"], ["O", "A"], ["A", "O"], ["O", "O"],
        ["A", "B", "A", "B"],      # P = 2: a doubling between piece sums
        ["A", "B", "-A", "-B"],    # opposite piece sums
        ["A", "-A", "B", "B"],     # O plus a piece sum
        ["A", "B", "B", "A"],      # equal sums from different orders, unequal Z
        ["A", "B", "-A", "-B", "A", "B", "-A", "-B", "A"],  # the first eight cancel: O meets a single point at the third level
    ]
    ks = [term[t][0] for seg in segs for t in seg]
    xy = np.stack([bases[term[t][1]] for seg in segs for t in seg])
    sp = seg_ptr_of([len(seg) for seg in segs])
    s = to_limbs(ks)
    want = oracle_sums(s, xy, None, sp)
    A, B = co.k233_mul(ka, np_to_pt(bases[0]), frob=False), co.k233_mul(kb, np_to_pt(bases[1]), frob=False)
    AB = oracle_add(A, B)
    # the products are what their names say
    assert want == [oracle_add(A, A), None, A, A, None, oracle_add(AB, AB), None, oracle_add(B, B), oracle_add(AB, AB), A]
    return dict(s=s, xy=xy, sp=sp, want=want)


@pytest.mark.parametrize("p", PIECES)
def test_shapes(dvp, shapes, one_segment, singletons, p):
    c = shapes
    with piece(dvp, p):
        xy, inf = dvp.curve.multi_scalar_mul_segments(c["s"], c["xy"], c["sp"], c["inf"])
        check_sums(xy, inf, c["want"], (p, "layout"))
        assert sum(1 for w in c["want"] if w is None) == 6  # four empty segments and two whose only point is flagged
        # one segment: the oracle, and the one-shot MSM
        o = one_segment
        xy, inf = dvp.curve.multi_scalar_mul_segments(o["s"], o["xy"], [0, 1025])
        check_sums(xy, inf, [o["want"]], (p, "B = 1"))
        m_xy, m_inf = dvp.curve.multi_scalar_mul(o["s"], o["xy"])
        assert not m_inf and m_xy.tobytes() == xy[0].tobytes()
        # one point per segment: dvp_points_mul, bit for bit
        g = singletons
        xy, inf = dvp.curve.multi_scalar_mul_segments(g["s"], g["xy"], g["sp"])
        check_sums(xy, inf, g["want"], (p, "B = n"))
        p_xy, p_inf = dvp.curve.point_scalar_mul(g["s"], g["xy"])
        assert p_xy.tobytes() == xy.tobytes() and p_inf.tobytes() == inf.tobytes() and inf[5] == 1


def test_out_of_range_piece_is_the_default(dvp, shapes):
    c = shapes
    ref = dvp.curve.multi_scalar_mul_segments(c["s"], c["xy"], c["sp"], c["inf"])
    for p in (0, 1, 65):
        with piece(dvp, p):
            got = dvp.curve.multi_scalar_mul_segments(c["s"], c["xy"], c["sp"], c["inf"])
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), p
    check_sums(ref[0], ref[1], c["want"], "default")


@pytest.mark.parametrize("p", PIECES)
def test_exceptional_operands_at_every_level(dvp, exceptional, p):
    c = exceptional
    with piece(dvp, p):
        xy, inf = dvp.curve.multi_scalar_mul_segments(c["s"], c["xy"], c["sp"])
    check_sums(xy, inf, c["want"], p)


@pytest.mark.parametrize("p", PIECES)
def test_sum_of_segments_is_the_msm(dvp, random_cut, p):
    """the reference's own identity (test_msm, src/curve.rs:218-232) over a cut"""
    c = random_cut
    with piece(dvp, p):
        xy, inf = dvp.curve.multi_scalar_mul_segments(c["s"], c["xy"], c["sp"])
    check_sums(xy, inf, c["want"], p)
    total = None
    for j in range(37):
        total = oracle_add(total, None if inf[j] else np_to_pt(xy[j]))
    assert total == c["whole"] and total is not None
    m_xy, m_inf = dvp.curve.multi_scalar_mul(c["s"], c["xy"])
    assert not m_inf and np_to_pt(m_xy) == total


def test_dev_flavour(dvp, random_cut):
    import torch

    c = random_cut
    n, n_seg = 1000, 37
    mid = 18
    j = (int(c["sp"][mid]) + int(c["sp"][mid + 1])) // 2  # a lane of the middle segment
    ks = list(c["ks"])
    ks[j] = R + 3
    without = list(c["ks"])
    without[j] = 0
    a, b = int(c["sp"][mid]), int(c["sp"][mid + 1])
    want_bad = list(c["want"])
    want_bad[mid] = co.msm(to_limbs(without)[a:b], c["xy"][a:b])
    side = torch.cuda.Stream()
    wb = dvp.curve.segments_work_bytes(n, n_seg)
    t_xy = torch.from_numpy(c["xy"].view(np.int64)).cuda()
    t_out = torch.full((n_seg, 64), 0xA5, dtype=torch.uint8, device="cuda")
    t_oinf = torch.full((n_seg,), 0xA5, dtype=torch.uint8, device="cuda")
    t_work = torch.full((wb,), 0xA5, dtype=torch.uint8, device="cuda")
    t_sum = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")

    def run(scalars):
        t_s = torch.from_numpy(to_limbs(scalars).view(np.int64)).cuda()
        torch.cuda.synchronize()
        dvp.curve.multi_scalar_mul_segments_dev(t_s.data_ptr(), t_xy.data_ptr(), 0, n, c["sp"], t_out.data_ptr(), t_oinf.data_ptr(),
                                                t_work.data_ptr(), wb, t_sum.data_ptr(), side.cuda_stream)
        side.synchronize()
        first, cnt = (int(v) for v in t_sum.cpu().numpy().view(np.uint64))
        return t_out.cpu().numpy().view(np.uint64).reshape(n_seg, 8), t_oinf.cpu().numpy(), first, cnt

    xy, inf, first, cnt = run(ks)
    assert (first, cnt) == (j, 1)
    check_sums(xy, inf, want_bad, "one lane gives O")
    xy, inf, first, cnt = run(c["ks"])  # the same buffers, clean scalars: the call resets the summary
    assert (first, cnt) == (NONE64, 0)
    check_sums(xy, inf, c["want"], "second call")


def test_host_errors(dvp, shapes):
    c = shapes
    n, n_seg = c["xy"].shape[0], len(LENGTHS)
    p = dvp._native.ptr
    bad = c["s"].copy()
    bad[300] = to_limbs([R])[0]
    bad[400] = to_limbs([(1 << 256) - 1])[0]
    oxy = np.full((n_seg, 8), 0x5A5A5A5A, dtype=np.uint64)
    oinf = np.full(n_seg, 0xEE, dtype=np.uint8)
    assert dvp.lib.dvp_msm_segments(p(bad), p(c["xy"]), p(c["inf"]), n, p(c["sp"]), n_seg, p(oxy), p(oinf)) == EINVAL
    assert dvp.lib.dvp_last_error_index() == 300
    assert (oxy == 0x5A5A5A5A).all() and (oinf == 0xEE).all()
    with pytest.raises(dvp.DvpError) as e:
        dvp.curve.multi_scalar_mul_segments(bad, c["xy"], c["sp"], c["inf"])
    assert e.value.status == EINVAL and e.value.index == 300
    coset = next(q for q in pc.load() if q["cls"] == pc.COSET_N and not q["inf"] and q["x"])
    xy = c["xy"].copy()
    j = 350  # behind the bad scalar at 300: the point is still what is reported
    assert not c["inf"][j]
    xy[j] = pts_to_np([(coset["x"], coset["y"])])[0]
    prev = dvp.curve.strict_points()
    try:
        dvp.curve.set_strict_points(True)
        assert dvp.lib.dvp_msm_segments(p(bad), p(xy), p(c["inf"]), n, p(c["sp"]), n_seg, p(oxy), p(oinf)) == EPOINT
        assert dvp.lib.dvp_last_error_index() == j
        assert (oxy == 0x5A5A5A5A).all() and (oinf == 0xEE).all()
        got = dvp.curve.multi_scalar_mul_segments(c["s"], c["xy"], c["sp"], c["inf"])  # clean points pass, garbage behind flags included
        check_sums(got[0], got[1], c["want"], "strict, clean")
    finally:
        dvp.curve.set_strict_points(prev)
    assert dvp.curve.strict_points() == prev


def test_wire_format(dvp, singletons):
    g = singletons
    n = 65
    sp = np.array([0, 20, 20, 41, 65], dtype=np.uint64)  # four segments, one empty
    s = g["s"][:n]
    xy = g["xy"][:n]
    want = oracle_sums(s, xy, None, sp)
    assert want[1] is None
    s32 = s.view(np.uint8).reshape(n, 32)
    enc = np.frombuffer(b"".join(co.xsk233_encode(np_to_pt(xy[i])) for i in range(n)), dtype=np.uint8).reshape(n, 30).copy()
    out = dvp.curve.multi_scalar_mul_segments_bytes(s32, enc, sp)
    assert out.shape == (4, 30)
    for j in range(4):
        a, b = int(sp[j]), int(sp[j + 1])
        assert out[j].tobytes() == co.xsk233_encode(want[j]), j
        assert out[j].tobytes() == dvp.curve.multi_scalar_mul_bytes(s32[a:b], enc[a:b]), j
    rnd = random.Random(91)
    while True:  # bytes that are no encoding, by the oracle's own decoder
        junk = rnd.getrandbits(233).to_bytes(30, "little")
        if not co.xsk233_decode(junk)[1]:
            break
    enc[23] = np.frombuffer(junk, dtype=np.uint8)
    with pytest.raises(dvp.DvpError) as e:
        dvp.curve.multi_scalar_mul_segments_bytes(s32, enc, sp)
    assert e.value.status == EDECODE and e.value.index == 23
