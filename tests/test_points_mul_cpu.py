"""CPU tests of dvp_points_mul: the parts of the ABI that need no device, and the case set of tests/points_mul_cases.py -- its
restated width-w tau-NAF evaluates back to the scalar, and the scalar set reaches every digit value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import points_mul_cases as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ENTRIES = ("dvp_points_mul", "dvp_points_mul_dev", "dvp_points_mul_xsk233")


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(dvp_[a-z0-9_]+)\s*\(", txt))


def test_entries_are_declared_exported_and_bound(nat):
    assert set(ENTRIES) <= _declared("dvpari.h")
    assert "dvp_debug_recode_tnaf" in _declared("dvpari_internal.h")
    lib = C.CDLL(nat.LIB_PATH)
    for s in ENTRIES + ("dvp_debug_recode_tnaf",):
        assert hasattr(lib, s), s
        assert s in nat._SIGS and s in nat.EXPORTED, s


def test_python_mirror_exists(dvp):
    for f in ("point_scalar_mul", "point_scalar_mul_dev", "point_scalar_mul_bytes"):
        assert callable(getattr(dvp.curve, f)), f


def test_empty_call_needs_no_device(dvp):
    assert dvp.lib.dvp_points_mul(None, 0, None, None, 0, None, None) == 0
    assert dvp.lib.dvp_points_mul(None, 1, None, None, 0, None, None) == 0
    assert dvp.lib.dvp_points_mul_xsk233(None, 0, None, 0, None) == 0


def test_invalid_arguments_need_no_device(dvp, nat):
    n = 3
    s = np.ones((n, 4), dtype=np.uint64)
    xy = np.ones((n, 8), dtype=np.uint64)
    oxy = np.full((n, 8), 0x5A, dtype=np.uint64)
    oinf = np.full(n, 0x5A, dtype=np.uint8)
    p = nat.ptr
    f = dvp.lib.dvp_points_mul
    assert f(None, n, p(xy), None, n, p(oxy), p(oinf)) == EINVAL
    assert f(p(s), n, None, None, n, p(oxy), p(oinf)) == EINVAL
    assert f(p(s), n, p(xy), None, n, None, p(oinf)) == EINVAL
    assert f(p(s), n, p(xy), None, n, p(oxy), None) == EINVAL
    for bad_ns in (0, 2, n + 1):
        assert f(p(s), bad_ns, p(xy), None, n, p(oxy), p(oinf)) == EINVAL, bad_ns
    assert (oxy == 0x5A).all() and (oinf == 0x5A).all()
    s32 = np.ones((n, 32), dtype=np.uint8)
    enc = np.zeros((n, 30), dtype=np.uint8)
    out = np.full((n, 30), 0x5A, dtype=np.uint8)
    g = dvp.lib.dvp_points_mul_xsk233
    assert g(None, n, p(enc), n, p(out)) == EINVAL
    assert g(p(s32), n, None, n, p(out)) == EINVAL
    assert g(p(s32), n, p(enc), n, None) == EINVAL
    for bad_ns in (0, 2, n + 1):
        assert g(p(s32), bad_ns, p(enc), n, p(out)) == EINVAL, bad_ns
    assert (out == 0x5A).all()
    # the device flavour: the same decisions, before anything is enqueued
    h = dvp.lib.dvp_points_mul_dev
    assert h(None, n, None, None, n, None, None, None, None) == EINVAL


def test_knob_and_recoder_constants_need_no_device(dvp):
    v = C.c_longlong(0)
    assert dvp.lib.dvp_tune_get(b"DVP_POINTS_MUL_W", C.byref(v)) == 0 and v.value in pm.WIDTHS
    for w in pm.WIDTHS:
        nd = C.c_int(0)
        alpha = np.zeros(2 << (w - 2), dtype=np.int32)
        assert dvp.lib.dvp_debug_recode_tnaf(None, 0, w, None, C.byref(nd), alpha.ctypes.data) == 0
        # the representatives the kernel derives are congruent to u modulo tau^w and of the least norm, as the restated ones are
        mine = pm.alpha_table(w)
        tw = pm.zt_pow_tau(w)
        nw = pm.zt_norm(tw)
        for e, u in enumerate(range(1, 1 << (w - 1), 2)):
            b, g = int(alpha[2 * e]), int(alpha[2 * e + 1])
            d = pm.zt_mul((b - u, g), (tw[0] - tw[1], -tw[1]))  # (alpha - u) conj(tau^w): divisible by N(tau^w) = 2^w
            assert d[0] % nw == 0 and d[1] % nw == 0, (w, u)
            assert pm.zt_norm((b, g)) == pm.zt_norm(mine[u]), (w, u)
        # the proven bound covers what the restated recoder needs on the case set
        assert 233 < nd.value <= 256
        assert max(len(pm.tnaf_w(k, w)) for k in pm.scalar_cases()[:120]) <= nd.value
    for w in (2, 6):
        assert dvp.lib.dvp_debug_recode_tnaf(None, 0, w, None, C.byref(C.c_int(0)), None) == EINVAL


def test_lambda():
    lam = pm.lam()
    assert (lam * lam + lam + 2) % pm.R == 0


@pytest.mark.parametrize("w", pm.WIDTHS)
def test_restated_recoding_evaluates_to_the_scalar(w):
    lam, alpha = pm.lam(), pm.alpha_table(w)
    for k in pm.scalar_cases():
        d = pm.tnaf_w(k, w, alpha)
        assert pm.evaluate(d, alpha, lam) == k, hex(k)
        nz = [j for j, v in enumerate(d) if v]
        assert all(b - a >= w for a, b in zip(nz, nz[1:])), hex(k)
        assert all(v % 2 and abs(v) < 1 << (w - 1) for v in d if v), hex(k)


@pytest.mark.parametrize("w", pm.WIDTHS)
def test_case_set_reaches_every_digit_value(w):
    want = {s * u for u in range(1, 1 << (w - 1), 2) for s in (1, -1)}
    assert pm.digit_values_seen(pm.scalar_cases(), w) == want
