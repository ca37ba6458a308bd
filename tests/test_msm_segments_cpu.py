"""CPU tests of dvp_msm_segments: the parts of the ABI that need no device -- declarations, empty calls, the CSR checks on seg_ptr,
argument checks, the arithmetic of dvp_msm_segments_work_bytes and the piece-length knob."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ENTRIES = ("dvp_msm_segments", "dvp_msm_segments_work_bytes", "dvp_msm_segments_dev", "dvp_msm_segments_xsk233")
KNOB = b"DVP_MSM_SEG_PIECE"
FAKE = 0x10000  # a non-NULL "device pointer" for calls that must be refused before anything is dereferenced


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(dvp_[a-z0-9_]+)\s*\(", txt))


def u64(vals):
    return np.array(vals, dtype=np.uint64)


def test_entries_are_declared_exported_and_bound(nat):
    assert set(ENTRIES) <= _declared("dvpari.h")
    lib = C.CDLL(nat.LIB_PATH)
    for s in ENTRIES:
        assert hasattr(lib, s), s
        assert s in nat._SIGS and s in nat.EXPORTED, s


def test_python_mirror_exists(dvp):
    for f in ("multi_scalar_mul_segments", "multi_scalar_mul_segments_dev", "multi_scalar_mul_segments_bytes", "segments_work_bytes"):
        assert callable(getattr(dvp.curve, f)), f


def test_no_segments_touches_nothing(dvp, nat):
    p = nat.ptr
    sp = u64([0])
    assert dvp.lib.dvp_msm_segments(None, None, None, 0, p(sp), 0, None, None) == 0
    assert dvp.lib.dvp_msm_segments(None, None, None, 0, None, 0, None, None) == 0
    assert dvp.lib.dvp_msm_segments_xsk233(None, None, 0, None, 0, None) == 0
    assert dvp.lib.dvp_msm_segments_dev(None, None, None, 0, None, 0, None, None, None, 0, None, None) == 0
    xy, inf = dvp.curve.multi_scalar_mul_segments(np.zeros((0, 4), np.uint64), np.zeros((0, 8), np.uint64), [0])
    assert xy.shape == (0, 8) and inf.shape == (0,)


def test_no_points_gives_neutral_elements_without_a_device(dvp, nat):
    p = nat.ptr
    sp = u64([0, 0, 0, 0])
    oxy = np.full((3, 8), 0x5A, dtype=np.uint64)
    oinf = np.full(3, 0x5A, dtype=np.uint8)
    assert dvp.lib.dvp_msm_segments(None, None, None, 0, p(sp), 3, p(oxy), p(oinf)) == 0
    assert not oxy.any() and (oinf == 1).all()
    enc = np.full((3, 30), 0x5A, dtype=np.uint8)
    assert dvp.lib.dvp_msm_segments_xsk233(None, None, 0, p(sp), 3, p(enc)) == 0
    assert not enc.any()  # the neutral element's encoding
    xy, inf = dvp.curve.multi_scalar_mul_segments(np.zeros((0, 4), np.uint64), np.zeros((0, 8), np.uint64), sp)
    assert xy.shape == (3, 8) and not xy.any() and (inf == 1).all()
    out = dvp.curve.multi_scalar_mul_segments_bytes(np.zeros((0, 32), np.uint8), np.zeros((0, 30), np.uint8), sp)
    assert out.shape == (3, 30) and not out.any()


def _all_flavours(dvp, nat, n, sp):
    """the three entries on one seg_ptr, outputs sentinel-filled: [(status, error index)], and the outputs must stay untouched"""
    p = nat.ptr
    n_seg = len(sp) - 1
    s = np.ones((max(n, 1), 4), dtype=np.uint64)
    xy = np.ones((max(n, 1), 8), dtype=np.uint64)
    oxy = np.full((n_seg, 8), 0x5A, dtype=np.uint64)
    oinf = np.full(n_seg, 0x5A, dtype=np.uint8)
    s32 = np.ones((max(n, 1), 32), dtype=np.uint8)
    enc = np.zeros((max(n, 1), 30), dtype=np.uint8)
    oenc = np.full((n_seg, 30), 0x5A, dtype=np.uint8)
    res = []
    res.append((dvp.lib.dvp_msm_segments(p(s), p(xy), None, n, p(sp), n_seg, p(oxy), p(oinf)), dvp.lib.dvp_last_error_index()))
    res.append((dvp.lib.dvp_msm_segments_xsk233(p(s32), p(enc), n, p(sp), n_seg, p(oenc)), dvp.lib.dvp_last_error_index()))
    wb = dvp.lib.dvp_msm_segments_work_bytes(n, n_seg)
    res.append((dvp.lib.dvp_msm_segments_dev(FAKE, FAKE, None, n, p(sp), n_seg, FAKE, FAKE, FAKE, wb, FAKE, None), dvp.lib.dvp_last_error_index()))
    assert (oxy == 0x5A).all() and (oinf == 0x5A).all() and (oenc == 0x5A).all()
    return res


def test_bad_segment_pointers_need_no_device(dvp, nat):
    n = 10
    cases = [
        (u64([1, 4, 10]), 0),          # seg_ptr[0] != 0
        (u64([0, 4, 3, 10]), 1),       # a decreasing pair: segment 1
        (u64([0, 4, 7, 7, 6, 10]), 3),
        (u64([0, 4, 9]), 1),           # last entry short of n: the last segment
        (u64([0, 4, 11]), 1),          # last entry beyond n
        (u64([0, 12, 10]), 0),         # an entry beyond n in the middle
        (u64([0, 1 << 40, 10]), 0),    # far beyond 32 bits
    ]
    for sp, want in cases:
        for status, idx in _all_flavours(dvp, nat, n, sp):
            assert (status, idx) == (EINVAL, want), (sp.tolist(), status, idx)
    # the same with n = 0: only all-zero offsets are sound
    for status, idx in _all_flavours(dvp, nat, 0, u64([0, 0, 1])):
        assert (status, idx) == (EINVAL, 1)


def test_invalid_arguments_need_no_device(dvp, nat):
    p = nat.ptr
    n = 3
    sp = u64([0, 1, 3])
    s = np.ones((n, 4), dtype=np.uint64)
    xy = np.ones((n, 8), dtype=np.uint64)
    oxy = np.full((2, 8), 0x5A, dtype=np.uint64)
    oinf = np.full(2, 0x5A, dtype=np.uint8)
    f = dvp.lib.dvp_msm_segments
    assert f(None, p(xy), None, n, p(sp), 2, p(oxy), p(oinf)) == EINVAL
    assert f(p(s), None, None, n, p(sp), 2, p(oxy), p(oinf)) == EINVAL
    assert f(p(s), p(xy), None, n, None, 2, p(oxy), p(oinf)) == EINVAL
    assert f(p(s), p(xy), None, n, p(sp), 2, None, p(oinf)) == EINVAL
    assert f(p(s), p(xy), None, n, p(sp), 2, p(oxy), None) == EINVAL
    assert f(p(s), p(xy), None, 1 << 32, p(sp), 2, p(oxy), p(oinf)) == EINVAL
    assert f(p(s), p(xy), None, n, p(sp), 1 << 32, p(oxy), p(oinf)) == EINVAL
    s32 = np.ones((n, 32), dtype=np.uint8)
    enc = np.zeros((n, 30), dtype=np.uint8)
    oenc = np.full((2, 30), 0x5A, dtype=np.uint8)
    g = dvp.lib.dvp_msm_segments_xsk233
    assert g(None, p(enc), n, p(sp), 2, p(oenc)) == EINVAL
    assert g(p(s32), None, n, p(sp), 2, p(oenc)) == EINVAL
    assert g(p(s32), p(enc), n, None, 2, p(oenc)) == EINVAL
    assert g(p(s32), p(enc), n, p(sp), 2, None) == EINVAL
    assert g(p(s32), p(enc), 1 << 32, p(sp), 2, p(oenc)) == EINVAL
    assert g(p(s32), p(enc), n, p(sp), 1 << 32, p(oenc)) == EINVAL
    assert (oxy == 0x5A).all() and (oinf == 0x5A).all() and (oenc == 0x5A).all()
    h = dvp.lib.dvp_msm_segments_dev
    wb = dvp.lib.dvp_msm_segments_work_bytes(n, 2)
    ok = dict(d_scalars=FAKE, d_xy=FAKE, d_inf=None, n=n, seg_ptr=p(sp), n_seg=2, d_out_xy=FAKE, d_out_inf=FAKE, d_work=FAKE, work_bytes=wb,
              d_summary=FAKE, stream=None)
    for name in ("d_scalars", "d_xy", "seg_ptr", "d_out_xy", "d_out_inf", "d_work", "d_summary"):
        a = dict(ok)
        a[name] = None
        assert h(*a.values()) == EINVAL, name
    for name in ("n", "n_seg"):
        a = dict(ok)
        a[name] = 1 << 32
        assert h(*a.values()) == EINVAL, name
    for short in (0, wb - 1):
        a = dict(ok)
        a["work_bytes"] = short
        assert h(*a.values()) == EINVAL, short


def test_work_bytes_arithmetic(dvp):
    f = dvp.curve.segments_work_bytes
    ns = [0, 1, 2, 3, 63, 64, 65, 1000, 1 << 16, (1 << 16) + 1, 1 << 20, 3 << 20, (1 << 32) - 1]
    segs = [0, 1, 2, 37, 1 << 10, 1 << 16, 1 << 20, (1 << 32) - 1]
    for n in ns:
        for b in segs:
            assert f(n, b) >= 65 * n, (n, b)
    for b in segs:
        col = [f(n, b) for n in ns]
        assert col == sorted(col), b
    for n in ns:
        row = [f(n, b) for b in segs]
        assert row == sorted(row), n
    # room for the offsets of at least one level
    assert f(1000, 37) >= 65 * 1000 + 4 * 38


def test_knob_is_listed_and_out_of_range_means_the_default(dvp):
    v = C.c_longlong(0)
    assert dvp.lib.dvp_tune_get(KNOB, C.byref(v)) == 0
    prev = v.value
    assert 2 <= prev <= 64
    try:
        for val in (2, 3, 64, 0, 1, 65, -7, 1 << 40):
            assert dvp.lib.dvp_tune_set(KNOB, val) == 0
            assert dvp.lib.dvp_tune_get(KNOB, C.byref(v)) == 0 and v.value == val
    finally:
        dvp.lib.dvp_tune_set(KNOB, prev)
    wb = dvp.curve.segments_work_bytes(1 << 12, 5)
    for val in (2, 64, 0, 1, 65, -7):  # in range or not, the size covers it (out of range runs as the default: the GPU tests compare results)
        with dvp._native.tune(DVP_MSM_SEG_PIECE=val):
            assert dvp.curve.segments_work_bytes(1 << 12, 5) == wb
    assert dvp.lib.dvp_tune_get(KNOB, C.byref(v)) == 0 and v.value == prev
