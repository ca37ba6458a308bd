"""GPU tests (-m gpu) of dvp_points_mul, the vector of variable-base scalar multiplications (src/curve.rs:113-126).  Every product is
compared bit for bit with the C oracle's INTEGER double-and-add (c_oracle.k233_mul(.., frob=False)), which shares nothing with the
tau-adic machinery under test; the OpenSSL vectors are a second, external reference.  The oracle's products are computed once per
module and never changed."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import c_oracle as co
import point_cases as pc
import points_mul_cases as pm
import pyref as o
from util import np_to_pt, pts_to_np, to_limbs

pytestmark = pytest.mark.gpu
OSSL = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "k233_openssl.json")))["vectors"]
R = pm.R
NONE64 = (1 << 64) - 1
EINVAL, EDECODE, EPOINT = -1, -2, -9
KNOB = b"DVP_POINTS_MUL_W"


class width:
    """DVP_POINTS_MUL_W = w inside the block; the previous value comes back in a finally"""

    def __init__(self, dvp, w):
        self.dvp, self.w = dvp, w

    def __enter__(self):
        v = C.c_longlong(0)
        self.dvp.check(self.dvp.lib.dvp_tune_get(KNOB, C.byref(v)))
        self.prev = v.value
        self.dvp.check(self.dvp.lib.dvp_tune_set(KNOB, self.w))

    def __exit__(self, *exc):
        self.dvp.lib.dvp_tune_set(KNOB, self.prev)
        return False


def ref_mul(k, pt):
    return None if pt is None else co.k233_mul(k, pt, frob=False)


def pack(pts):
    """[(x, y) or None] -> (xy [n, 8], inf [n]); a point at infinity keeps garbage coordinates behind its flag"""
    xy = pts_to_np([p if p is not None else (0x1234, 0x5678) for p in pts])
    inf = np.array([p is None for p in pts], dtype=np.uint8)
    return xy, inf


def check_products(xy, inf, want, what=""):
    assert xy.shape == (len(want), 8) and inf.shape == (len(want),)
    for i, w in enumerate(want):
        if w is None:
            assert inf[i] == 1 and not xy[i].any(), (what, i)
        else:
            assert inf[i] == 0 and np_to_pt(xy[i]) == w, (what, i)


@pytest.fixture(scope="module")
def base_points():
    """G, two seeded multiples of G, and O"""
    rnd = random.Random(20240)
    return [o.G_STD, co.k233_mulgen(rnd.randrange(1, R)), co.k233_mulgen(rnd.randrange(1, R)), None]


@pytest.fixture(scope="module")
def case_products(base_points):
    """S x the four points, and the oracle's products: shared by every width"""
    S = pm.scalar_cases()
    ks = [k for k in S for _ in base_points]
    pts = [p for _ in S for p in base_points]
    return ks, pts, [ref_mul(k, p) for k, p in zip(ks, pts)]


SHAPES = [1, 63, 64, 65, 255, 256, 257, 1025]


@pytest.fixture(scope="module")
def shape_products(dvp):
    """per n: seeded random pairs with an infinity flag at index 0, at n - 1 and at a wave boundary (where n has one)"""
    out = {}
    for n in SHAPES:
        rnd = random.Random(700 + n)
        bases_k = to_limbs([rnd.randrange(1, R) for _ in range(n)])
        xy, binf = dvp.curve.point_scalar_mul_gen_batch(bases_k)
        assert not binf.any()
        ks = [rnd.randrange(R) for _ in range(n)]
        flagged = sorted({0, n - 1} | ({64} if n > 64 else set()) | ({63} if n > 63 else set()))
        pts = [np_to_pt(xy[i]) for i in range(n)]
        out[n] = dict(ks=ks, xy=xy, flagged=flagged, want_all=[ref_mul(k, p) for k, p in zip(ks, pts)])
    return out


def test_openssl_vectors(dvp):
    ks = [int(v["k"], 16) for v in OSSL]
    assert len(ks) == 64
    g = pts_to_np([o.G_STD] * len(ks))
    xy, inf = dvp.curve.point_scalar_mul(to_limbs(ks), g)
    for i, v in enumerate(OSSL):
        assert inf[i] == 0 and np_to_pt(xy[i]) == (int(v["x"], 16), int(v["y"], 16)), v["k"]


@pytest.mark.parametrize("w", pm.WIDTHS)
def test_scalar_cases_times_points(dvp, case_products, w):
    ks, pts, want = case_products
    xy, inf = pack(pts)
    with width(dvp, w):
        got_xy, got_inf = dvp.curve.point_scalar_mul(to_limbs(ks), xy, inf)
    check_products(got_xy, got_inf, want, w)
    assert sum(1 for x in want if x is None) >= len(pm.scalar_cases())  # k = 0 and P = O are in there


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("w", pm.WIDTHS)
def test_shapes(dvp, shape_products, w, n):
    c = shape_products[n]
    inf = np.zeros(n, dtype=np.uint8)
    inf[c["flagged"]] = 1
    want = [None if i in c["flagged"] else p for i, p in enumerate(c["want_all"])]
    with width(dvp, w):
        got_xy, got_inf = dvp.curve.point_scalar_mul(to_limbs(c["ks"]), c["xy"], inf)
        check_products(got_xy, got_inf, want, (w, n, "flags"))
        got_xy, got_inf = dvp.curve.point_scalar_mul(to_limbs(c["ks"]), c["xy"], None)  # inf == NULL
        check_products(got_xy, got_inf, c["want_all"], (w, n, "no flags"))


@pytest.mark.parametrize("w", pm.WIDTHS)
def test_broadcast_scalar(dvp, shape_products, w):
    c = shape_products[257]
    k = c["ks"][5]
    with width(dvp, w):
        one_xy, one_inf = dvp.curve.point_scalar_mul(to_limbs([k]), c["xy"])
        all_xy, all_inf = dvp.curve.point_scalar_mul(to_limbs([k] * 257), c["xy"])
    assert one_xy.tobytes() == all_xy.tobytes() and one_inf.tobytes() == all_inf.tobytes()
    assert not one_inf.any() and np_to_pt(one_xy[5]) == c["want_all"][5]
    assert np_to_pt(one_xy[256]) == ref_mul(k, np_to_pt(c["xy"][256]))


def test_distributive_identity(dvp, shape_products):
    """(k1 + k2) P = k1 P + k2 P through dvp_points_add (src/curve.rs:198)"""
    c = shape_products[257]
    rnd = random.Random(8)
    k1 = [rnd.randrange(R) for _ in range(257)]
    k2 = [rnd.randrange(R) for _ in range(257)]
    k2[0] = (R - k1[0]) % R  # a sum that is 0
    k2[1] = k1[1]            # a doubling
    lhs = dvp.curve.point_scalar_mul(to_limbs([(a + b) % R for a, b in zip(k1, k2)]), c["xy"])
    a_xy, a_inf = dvp.curve.point_scalar_mul(to_limbs(k1), c["xy"])
    b_xy, b_inf = dvp.curve.point_scalar_mul(to_limbs(k2), c["xy"])
    rhs = dvp.curve.add(a_xy, b_xy, a_inf, b_inf)
    assert lhs[0].tobytes() == rhs[0].tobytes() and lhs[1].tobytes() == rhs[1].tobytes()
    assert lhs[1][0] == 1 and not lhs[1][1:].any()


def test_sum_of_products_is_the_msm(dvp):
    """n = 300: the lane-wise products folded with dvp_points_add equal dvp_msm_affine of the same inputs (src/curve.rs:218)"""
    n = 300
    rnd = random.Random(9)
    xy, binf = dvp.curve.point_scalar_mul_gen_batch(to_limbs([rnd.randrange(1, R) for _ in range(n)]))
    ks = to_limbs([rnd.randrange(R) for _ in range(n)])
    p_xy, p_inf = dvp.curve.point_scalar_mul(ks, xy)
    while p_xy.shape[0] > 1:  # fold halves: 300 -> 150 -> 75 -> 38 -> 19 -> 10 -> 5 -> 3 -> 2 -> 1
        m = p_xy.shape[0]
        h = (m + 1) // 2
        b_xy = np.zeros((h, 8), dtype=np.uint64)
        b_inf = np.ones(h, dtype=np.uint8)
        b_xy[: m - h] = p_xy[h:]
        b_inf[: m - h] = p_inf[h:]
        p_xy, p_inf = dvp.curve.add(p_xy[:h], b_xy, p_inf[:h], b_inf)
    m_xy, m_inf = dvp.curve.multi_scalar_mul(ks, xy)
    assert bool(p_inf[0]) == m_inf and p_xy[0].tobytes() == m_xy.tobytes()


def _dev_call(dvp, ks, xy, inf, stream=None, in_place=False, summary=None, n_scalars=None):
    """dvp_points_mul_dev on torch tensors -> (xy, inf, first bad scalar or None, how many)"""
    import torch

    n = xy.shape[0]
    st = stream if stream is not None else torch.cuda.current_stream()
    t_s = torch.from_numpy(to_limbs(ks).view(np.int64)).cuda()
    t_xy = torch.from_numpy(np.ascontiguousarray(xy).view(np.int64)).cuda()
    t_inf = None if inf is None else torch.from_numpy(np.ascontiguousarray(inf, dtype=np.uint8)).cuda()
    t_out = t_xy if in_place else torch.full((n, 8), 0x5A5A, dtype=torch.int64, device="cuda")
    t_oinf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    if summary is None:
        summary = torch.full((2,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dvp.curve.point_scalar_mul_dev(t_s.data_ptr(), len(ks) if n_scalars is None else n_scalars, t_xy.data_ptr(), 0 if t_inf is None else t_inf.data_ptr(), n,
                                   t_out.data_ptr(), t_oinf.data_ptr(), summary.data_ptr(), st.cuda_stream)
    st.synchronize()
    first, cnt = (int(v) for v in summary.cpu().numpy().view(np.uint64))
    return t_out.cpu().numpy().view(np.uint64), t_oinf.cpu().numpy(), (None if first == NONE64 else first), cnt


def test_non_canonical_scalars(dvp, shape_products):
    c = shape_products[257]
    ks = list(c["ks"])
    ks[70] = R
    ks[200] = (1 << 256) - 1
    oxy = np.full((257, 8), 0x5A5A5A5A, dtype=np.uint64)
    oinf = np.full(257, 0xEE, dtype=np.uint8)
    p = dvp._native.ptr
    s = to_limbs(ks)
    assert dvp.lib.dvp_points_mul(p(s), 257, p(c["xy"]), None, 257, p(oxy), p(oinf)) == EINVAL
    assert dvp.lib.dvp_last_error_index() == 70
    assert (oxy == 0x5A5A5A5A).all() and (oinf == 0xEE).all()
    with pytest.raises(dvp.DvpError) as e:
        dvp.curve.point_scalar_mul(s, c["xy"])
    assert e.value.status == EINVAL and e.value.index == 70
    one = to_limbs([R])  # the broadcast scalar
    assert dvp.lib.dvp_points_mul(p(one), 1, p(c["xy"]), None, 257, p(oxy), p(oinf)) == EINVAL and dvp.lib.dvp_last_error_index() == 0
    got_xy, got_inf, first, cnt = _dev_call(dvp, ks, c["xy"], None)
    assert (first, cnt) == (70, 2)
    want = [None if i in (70, 200) else q for i, q in enumerate(c["want_all"])]
    check_products(got_xy, got_inf, want, "dev")


def test_dev_flavour(dvp, shape_products):
    import torch

    c = shape_products[257]
    side = torch.cuda.Stream()
    got_xy, got_inf, first, cnt = _dev_call(dvp, c["ks"], c["xy"], None, stream=side)  # a non-default stream, d_inf == NULL
    assert (first, cnt) == (None, 0)
    check_products(got_xy, got_inf, c["want_all"], "side stream")
    inf = np.zeros(257, dtype=np.uint8)
    inf[c["flagged"]] = 1
    want = [None if i in c["flagged"] else q for i, q in enumerate(c["want_all"])]
    got_xy, got_inf, first, cnt = _dev_call(dvp, c["ks"], c["xy"], inf, stream=side, in_place=True)  # d_out_xy == d_xy
    assert (first, cnt) == (None, 0)
    check_products(got_xy, got_inf, want, "in place")
    # two calls back to back on one summary buffer, which the caller never touches: the first leaves a finding, the second none
    summary = torch.zeros(2, dtype=torch.int64, device="cuda")
    ks = list(c["ks"])
    ks[3] = R + 5
    _, _, first, cnt = _dev_call(dvp, ks, c["xy"], None, summary=summary)
    assert (first, cnt) == (3, 1)
    got_xy, got_inf, first, cnt = _dev_call(dvp, c["ks"], c["xy"], None, summary=summary)
    assert (first, cnt) == (None, 0)
    check_products(got_xy, got_inf, c["want_all"], "second call")
    # broadcast on the device: stride 0
    got_xy, got_inf, first, cnt = _dev_call(dvp, [c["ks"][5]], c["xy"][:65], None, n_scalars=1)
    assert (first, cnt) == (None, 0) and np_to_pt(got_xy[5]) == c["want_all"][5] and not got_inf.any()


def test_strict_mode(dvp, shape_products):
    c = shape_products[65]
    cases = pc.load()
    coset = next(q for q in cases if q["cls"] == pc.COSET_N and not q["inf"] and q["x"])
    xy = c["xy"].copy()
    j = 41
    xy[j] = pts_to_np([(coset["x"], coset["y"])])[0]
    ks = list(c["ks"])
    prev = dvp.curve.strict_points()
    try:
        dvp.curve.set_strict_points(True)
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.point_scalar_mul(to_limbs(ks), xy)
        assert e.value.status == EPOINT and e.value.index == j
        bad_ks = list(ks)
        bad_ks[7] = R  # a bad scalar at a smaller index: the point is still what is reported
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.point_scalar_mul(to_limbs(bad_ks), xy)
        assert e.value.status == EPOINT and e.value.index == j
        got = dvp.curve.point_scalar_mul(to_limbs(ks), c["xy"])  # clean points pass
        check_products(got[0], got[1], c["want_all"], "strict, clean")
        dvp.curve.set_strict_points(False)
        got = dvp.curve.point_scalar_mul(to_limbs(ks), xy)  # strict off: DVP_OK, the other lanes as ever
        keep = [i for i in range(65) if i != j]
        check_products(got[0][keep], got[1][keep], [c["want_all"][i] for i in keep], "strict off")
    finally:
        dvp.curve.set_strict_points(prev)


@pytest.mark.parametrize("rule", [0, 3])
def test_wire_format(dvp, shape_products, rule):
    c = shape_products[65]
    pts = [np_to_pt(c["xy"][i]) for i in range(65)]
    pts[9] = None
    ks = list(c["ks"])
    ks[11] = 0
    want = [None if (q is None or k == 0) else w for q, k, w in zip(pts, ks, c["want_all"])]
    s32 = to_limbs(ks).view(np.uint8).reshape(65, 32)
    try:
        dvp.check(dvp.lib.dvp_codec_set_rule(rule))
        enc = np.frombuffer(b"".join(o.xsk233_encode(q, rule) for q in pts), dtype=np.uint8).reshape(65, 30).copy()
        out = dvp.curve.point_scalar_mul_bytes(s32, enc)
        for i, w in enumerate(want):
            assert out[i].tobytes() == o.xsk233_encode(w, rule), (rule, i)
        rnd = random.Random(90 + rule)
        while True:  # bytes that are no encoding, by the oracle's own decoder
            junk = rnd.getrandbits(233).to_bytes(30, "big" if rule & 2 else "little")
            if not o.xsk233_decode(junk, rule)[1]:
                break
        j = 23
        enc[j] = np.frombuffer(junk, dtype=np.uint8)
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.point_scalar_mul_bytes(s32, enc)
        assert e.value.status == EDECODE and e.value.index == j
    finally:
        dvp.check(dvp.lib.dvp_codec_set_rule(0))


@pytest.mark.parametrize("w", pm.WIDTHS)
def test_recoder_on_the_device(dvp, w):
    rnd = random.Random(1000 + w)
    ks = pm.scalar_cases() + [rnd.randrange(R) for _ in range(20000)]
    n = len(ks)
    nd = C.c_int(0)
    alpha = np.zeros(2 << (w - 2), dtype=np.int32)
    assert dvp.lib.dvp_debug_recode_tnaf(None, 0, w, None, C.byref(nd), alpha.ctypes.data) == 0
    L = nd.value
    digits = np.full((n, L), 99, dtype=np.int8)
    s = to_limbs(ks)
    dvp.check(dvp.lib.dvp_debug_recode_tnaf(s.ctypes.data, n, w, digits.ctypes.data, C.byref(nd), alpha.ctypes.data), "recode")
    assert nd.value == L
    d = digits.astype(np.int64)
    nzmask = d != 0
    # odd, |u| < 2^(w-1)
    assert ((np.abs(d[nzmask]) & 1) == 1).all() and (np.abs(d[nzmask]) < (1 << (w - 1))).all()
    # at most one non-zero digit among any w consecutive positions
    c = np.cumsum(nzmask, axis=1)
    win = c[:, w - 1:] - np.concatenate([np.zeros((n, 1), dtype=c.dtype), c[:, :-w]], axis=1)
    assert win.max() <= 1
    # nothing at or beyond the bound: the remainder after L positions is zero exactly when the evaluation identity holds with L digits
    lam = pm.lam()
    a = {2 * e + 1: (int(alpha[2 * e]), int(alpha[2 * e + 1])) for e in range(1 << (w - 2))}
    # sum_j d_j tau^j exactly in Z[tau]: chunks of 16 positions by Horner in int64 (|value| < 2^13 there), the chunks combined with
    # python ints modulo r through tau -> lambda
    beta = np.zeros(1 << w, dtype=np.int64)
    gamma = np.zeros(1 << w, dtype=np.int64)
    for u, (b, g) in a.items():
        beta[u], gamma[u] = b, g
        beta[-u % (1 << w)], gamma[-u % (1 << w)] = -b, -g
    idx = d % (1 << w)
    acc = np.zeros(n, dtype=object)
    for c0 in range(0, L, 16):
        ca = np.zeros(n, dtype=np.int64)
        cb = np.zeros(n, dtype=np.int64)
        for j in range(min(L, c0 + 16) - 1, c0 - 1, -1):
            ca, cb = -2 * cb + beta[idx[:, j]], ca - cb + gamma[idx[:, j]]
        acc = (acc + (ca.astype(object) + cb.astype(object) * lam) * pow(lam, c0, R)) % R
    wrong = [hex(k) for k, v in zip(ks, acc) if v != k]
    assert not wrong, wrong[:4]
    # the set reaches every digit value on the device as well
    assert set(np.unique(d[: len(pm.scalar_cases())])) - {0} == {sg * u for u in a for sg in (1, -1)}
