"""GPU tests (-m gpu) of the affine point check: k_points_check's classes against the definitions on the recorded case set
(tests/point_cases.py), the wave / workgroup edges, the optional arguments, the summary's reset, and strict mode through every
entry that takes affine points from a caller."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import point_cases as pc
import pyref as o
from util import np_to_pt, pts_to_np

pytestmark = pytest.mark.gpu
VEC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_vectors.json")))
NONE64 = (1 << 64) - 1
EPOINT = -9


@pytest.fixture(scope="module")
def cases():
    cs = pc.load()
    return cs, pc.arrays(cs)


@pytest.fixture(scope="module")
def valid(dvp):
    """1000 points of E[r]: (k + 1) G from the library's own fixed-base multiplication"""
    s = np.zeros((1000, 4), dtype=np.uint64)
    s[:, 0] = np.arange(1, 1001, dtype=np.uint64)
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(s)
    assert not inf.any()
    return xy


@pytest.fixture(scope="module")
def bad64(valid):
    """64 valid bases with base 17 replaced by its + N image (P + N, N = (0,1): on the curve, reduced, outside E[r])"""
    b = valid[:64].copy()
    b[17] = pts_to_np([o.k233_add(np_to_pt(valid[17]), o.N_STD)])[0]
    return b


class strict:
    """strict mode on inside the block; the previous value comes back in a finally"""

    def __init__(self, dvp):
        self.dvp = dvp

    def __enter__(self):
        self.prev = self.dvp.curve.strict_points()
        self.dvp.curve.set_strict_points(True)

    def __exit__(self, *exc):
        self.dvp.curve.set_strict_points(self.prev)
        return False


def host_check(dvp, xy, inf=None, want_classes=True):
    """dvp_points_check itself -> (status, classes or None, first bad index or None, n_bad)"""
    nat = dvp._native
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 8)
    n = xy.shape[0]
    classes = np.full(n, 0xEE, dtype=np.uint8) if want_classes else None
    n_bad = C.c_size_t(12345)
    rc = dvp.lib.dvp_points_check(nat.ptr(xy), None if inf is None else nat.ptr(np.ascontiguousarray(inf, dtype=np.uint8)), n,
                                  None if classes is None else nat.ptr(classes), C.byref(n_bad))
    first = int(dvp.lib.dvp_last_error_index()) if rc == EPOINT else None
    return rc, classes, first, int(n_bad.value)


def dev_check(dvp, xy, inf=None, want_classes=True, summary=None):
    """dvp_points_check_dev on torch tensors -> (classes or None, first bad index or None, n_bad); `summary` = a caller's 16-byte
    tensor, else a fresh one filled with garbage (the entry resets it, the caller does not)"""
    import torch

    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 8)
    n = xy.shape[0]
    t_xy = torch.from_numpy(xy.view(np.int64)).cuda()
    t_inf = None if inf is None else torch.from_numpy(np.ascontiguousarray(inf, dtype=np.uint8)).cuda()
    t_cls = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") if want_classes else None
    if summary is None:
        summary = torch.full((2,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dvp.curve.check_points_dev(t_xy.data_ptr(), None if t_inf is None else t_inf.data_ptr(), n, None if t_cls is None else t_cls.data_ptr(),
                               summary.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    first, n_bad = (int(v) for v in summary.cpu().numpy().view(np.uint64))
    return (None if t_cls is None else t_cls.cpu().numpy()), (None if first == NONE64 else first), n_bad


def test_classes_on_every_case_host(dvp, cases):
    cs, (xy, inf, want) = cases
    rc, classes, first, n_bad = host_check(dvp, xy, inf)
    wrong = [(c["label"], int(g), int(w)) for c, g, w in zip(cs, classes, want) if g != w]
    assert not wrong, wrong
    assert classes.tobytes() == want.tobytes()
    assert rc == EPOINT and first == int(np.nonzero(want)[0][0]) and n_bad == int(np.count_nonzero(want))
    # the python mirror: the same classes, no exception
    classes2, first2 = dvp.curve.check_points(xy, inf)
    assert classes2.tobytes() == want.tobytes() and first2 == first


def test_classes_on_every_case_dev(dvp, cases):
    cs, (xy, inf, want) = cases
    classes, first, n_bad = dev_check(dvp, xy, inf)
    assert classes.tobytes() == want.tobytes(), [(c["label"], int(g), int(w)) for c, g, w in zip(cs, classes, want) if g != w]
    assert first == int(np.nonzero(want)[0][0]) and n_bad == int(np.count_nonzero(want))


def test_each_case_alone(dvp, cases):
    """every case as a vector of its own: the class does not depend on what the other lanes of the wave hold"""
    cs, (xy, inf, want) = cases
    for k in range(len(cs)):
        rc, classes, first, n_bad = host_check(dvp, xy[k:k + 1], inf[k:k + 1])
        assert classes[0] == want[k], cs[k]["label"]
        assert (rc, first, n_bad) == ((EPOINT, 0, 1) if want[k] else (0, None, 0)), cs[k]["label"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_vector_shapes(dvp, valid, cases, n):
    """the wave and workgroup edges and a ragged last block: all valid, then one bad point at index 0, at n - 1, and at both"""
    _, (cxy, _, cwant) = cases
    bad = cxy[int(np.nonzero(cwant == pc.COSET_N)[0][0])]
    v = valid[:n]
    rc, classes, first, n_bad = host_check(dvp, v)
    assert (rc, first, n_bad) == (0, None, 0) and not classes.any()
    classes, first, n_bad = dev_check(dvp, v)
    assert (first, n_bad) == (None, 0) and not classes.any()  # summary {~0, 0}
    for where in ([0], [n - 1], [0, n - 1]):
        w = v.copy()
        w[where] = bad
        want = np.zeros(n, dtype=np.uint8)
        want[where] = pc.COSET_N
        rc, classes, first, n_bad = host_check(dvp, w)
        assert rc == EPOINT and first == min(where) and n_bad == len(set(where)), where
        assert classes.tobytes() == want.tobytes()
        classes, first, n_bad = dev_check(dvp, w)
        assert first == min(where) and n_bad == len(set(where)) and classes.tobytes() == want.tobytes(), where


def test_optional_arguments(dvp, cases):
    cs, (xy, inf, want) = cases
    first_bad, count = int(np.nonzero(want)[0][0]), int(np.count_nonzero(want))
    rc, classes, first, n_bad = host_check(dvp, xy, inf, want_classes=False)  # classes == NULL
    assert (rc, classes, first, n_bad) == (EPOINT, None, first_bad, count)
    assert dvp.lib.dvp_points_check(dvp._native.ptr(xy), dvp._native.ptr(inf), len(cs), None, None) == EPOINT  # and n_bad == NULL
    # inf == NULL: the points behind an infinity flag are judged by their coordinates
    want_noinf = np.array([pc.class_by_trace(c["x"], c["y"], 0) for c in cs], dtype=np.uint8)
    assert (want_noinf != want).any()
    rc, classes, first, n_bad = host_check(dvp, xy, None)
    assert rc == EPOINT and classes.tobytes() == want_noinf.tobytes() and n_bad == int(np.count_nonzero(want_noinf))
    classes, first, n_bad = dev_check(dvp, xy, None)
    assert classes.tobytes() == want_noinf.tobytes() and first == int(np.nonzero(want_noinf)[0][0])
    classes, first, n_bad = dev_check(dvp, xy, inf, want_classes=False)  # d_classes == NULL
    assert (classes, first, n_bad) == (None, first_bad, count)


def test_second_call_with_one_summary_buffer(dvp, valid, cases):
    import torch

    _, (xy, inf, want) = cases
    summary = torch.zeros(2, dtype=torch.int64, device="cuda")
    _, first, n_bad = dev_check(dvp, xy, inf, summary=summary)
    assert first == int(np.nonzero(want)[0][0]) and n_bad == int(np.count_nonzero(want))
    _, first, n_bad = dev_check(dvp, valid[:300], None, summary=summary)  # the same buffer, untouched by the caller
    assert (first, n_bad) == (None, 0)


def _scalars(n):
    s = np.zeros((n, 4), dtype=np.uint64)
    s[:, 0] = np.arange(3, 3 + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 8)
    s[:, 1] = np.arange(n, dtype=np.uint64) + np.uint64(11)
    return s


def test_strict_off_takes_a_coset_base(dvp, bad64):
    """PINS TODAY'S BEHAVIOUR, which is not a good one: with strict mode off (the default) dvp_msm_affine takes a base outside E[r]
    without complaint and returns DVP_OK with some point.  Strict mode is what a host turns on to get DVP_EPOINT instead."""
    assert not dvp.curve.strict_points()
    dvp.curve.multi_scalar_mul(_scalars(64), bad64)  # raises on any status but DVP_OK


def test_strict_msm_affine(dvp, valid, bad64):
    with strict(dvp):
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.multi_scalar_mul(_scalars(64), bad64)
        assert e.value.status == EPOINT and e.value.index == 17 and "index 17" in str(e.value)
        got = dvp.curve.multi_scalar_mul(_scalars(64), valid[:64])  # valid bases pass
    assert not got[1]
    assert got[0].tobytes() == dvp.curve.multi_scalar_mul(_scalars(64), valid[:64])[0].tobytes()
    assert not dvp.curve.strict_points()


def test_strict_fixed_base_msm(dvp, valid, bad64):
    want = dvp.curve.multi_scalar_mul(_scalars(64), valid[:64])
    with strict(dvp):
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.FixedBaseMsm(bad64)
        assert e.value.status == EPOINT and e.value.index == 17
        h = C.c_void_p(0x1234)  # *out is not written on failure
        assert dvp.lib.dvp_msm_ctx_create(dvp._native.ptr(bad64), None, 64, 0, C.byref(h)) == EPOINT and h.value == 0x1234
        fb = dvp.curve.FixedBaseMsm(valid[:64])
        try:
            got = fb.run(_scalars(64))
        finally:
            fb.close()
    assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes()


def test_strict_points_add_and_encode(dvp, valid, bad64):
    a = valid[100:164]
    with strict(dvp):
        with pytest.raises(dvp.DvpError) as e:  # the bad point in b, a clean: b's index
            dvp.curve.add(a, bad64)
        assert e.value.status == EPOINT and e.value.index == 17
        a_bad = a.copy()
        a_bad[40] = bad64[17]
        with pytest.raises(dvp.DvpError) as e:  # both bad: operand a is reported first, although b's bad point has the smaller index
            dvp.curve.add(a_bad, bad64)
        assert e.value.status == EPOINT and e.value.index == 40
        inf = np.zeros(64, dtype=np.uint8)
        inf[17] = 1
        dvp.curve.add(a, bad64, None, inf)  # behind an infinity flag the coordinates are not judged
        with pytest.raises(dvp.DvpError) as e:
            dvp.curve.to_bytes(bad64)
        assert e.value.status == EPOINT and e.value.index == 17
        assert dvp.curve.to_bytes(a).shape == (64, 30)
    assert dvp.curve.to_bytes(bad64).shape == (64, 30)  # strict off again: no check


def test_strict_prover(dvp, cases):
    """the toy circuit (2^3 constraints, the smallest prover the suite uses): a rejected SRS vector leaves the prover as one whose
    vector was never set, and the accepted SRS gives the bytes of a prover that was never strict"""
    _, (cxy, _, cwant) = cases
    order4 = cxy[int(np.nonzero(cwant == pc.ORDER4)[0][0])]
    g = dvp.gnark_r1cs
    inst = g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 2)
    td = dvp.srs.Trapdoor(*(int(x, 16) for x in VEC["toy"]["trapdoor"]))
    pub, prv = list(o.TOY_PUBLIC), list(o.TOY_PRIVATE)
    ref = dvp.proving.Prover(inst)
    pv = dvp.proving.Prover(inst)
    unset = dvp.proving.Prover(inst)
    try:
        srs = dvp.srs.verifier_runs_setup(ref, inst, td)
        ref.set_srs(srs)
        want = ref.prove(pub, prv).to_bytes()
        assert len(want) == 118
        vecs = srs.as_list()
        for which in (0, 1, 2, 4):  # a prover whose vector 3 was never set: the status a proof attempt gives
            xy, inf = vecs[which]
            dvp.check(dvp.lib.dvp_prover_set_srs_affine(unset._h, which, dvp._native.ptr(np.ascontiguousarray(xy)), dvp._native.ptr(np.ascontiguousarray(inf)), xy.shape[0]))
        with pytest.raises(dvp.DvpError) as e:
            unset.prove(pub, prv)
        unset_status = e.value.status
        with strict(dvp):
            pv.set_srs(srs)
            assert pv.prove(pub, prv).to_bytes() == want
            xy, inf = (np.ascontiguousarray(a).copy() for a in vecs[3])
            xy[5] = order4
            inf[5] = 0
            rc = dvp.lib.dvp_prover_set_srs_affine(pv._h, 3, dvp._native.ptr(xy), dvp._native.ptr(inf), xy.shape[0])
            assert rc == EPOINT and dvp.lib.dvp_last_error_index() == 5
            with pytest.raises(dvp.DvpError) as e:  # not a proof over the rejected bases, nor over the ones set before
                pv.prove(pub, prv)
            assert e.value.status == unset_status
            # the device-pointer setter: the same
            import torch

            t_xy = torch.from_numpy(xy.view(np.int64)).cuda()
            t_inf = torch.from_numpy(inf).cuda()
            torch.cuda.synchronize()
            assert dvp.lib.dvp_prover_set_srs_affine_dev(pv._h, 3, t_xy.data_ptr(), t_inf.data_ptr(), xy.shape[0]) == EPOINT
            assert dvp.lib.dvp_last_error_index() == 5
            with pytest.raises(dvp.DvpError) as e:
                pv.prove(pub, prv)
            assert e.value.status == unset_status
            pv.set_srs(srs)
            assert pv.prove(pub, prv).to_bytes() == want
    finally:
        for q in (ref, pv, unset):
            q.close()
    assert not dvp.curve.strict_points()


def test_decoded_points_pass(dvp, cases):
    """codec_decode's own subgroup test and k_points_check agree: what dvp_points_decode returns for encodings of the case set's E[r]
    points passes the check (and strict mode lets them through encode again)"""
    cs, (xy, inf, want) = cases
    keep = np.array([c["cls"] == pc.OK and not c["inf"] for c in cs])
    pts = xy[keep]
    assert pts.shape[0] >= 8
    with strict(dvp):
        enc = dvp.curve.to_bytes(pts)
        dxy, dinf = dvp.curve.from_bytes(enc)
        assert not dinf.any() and dxy.tobytes() == pts.tobytes()
        rc, classes, first, n_bad = host_check(dvp, dxy, dinf)
        assert (rc, first, n_bad) == (0, None, 0) and not classes.any()
        assert dvp.curve.to_bytes(dxy, dinf).tobytes() == enc.tobytes()
