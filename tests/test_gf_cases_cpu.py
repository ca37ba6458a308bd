"""The case sets of gf_cases.py hold what they claim, their combined references agree with pyref's own functions and with the C oracle,
every point case is on the curve, and dvp_debug_gf_op rejects each violated precondition with the right index -- on the host, before
any device call, so all of this runs without a GPU."""
import ctypes as C
import random

import numpy as np
import pytest

import c_oracle as co
import gf_cases as gc
import pyref as o


def test_field_case_tables_hold_what_they_state():
    e = set(gc.edge_values())
    f = set(gc.field_values())
    assert set(gc.basis()) <= f and len(gc.basis()) == 233 and e <= f
    lo = (1 << 117) - 1
    assert {0, 1, gc.MASK, (1 << 232) | 1, lo, gc.MASK ^ lo, 1 << 116, 1 << 117, 1 << 159} <= e
    assert lo & (gc.MASK ^ lo) == 0 and lo | (gc.MASK ^ lo) == gc.MASK
    for v in gc.equal_halves():  # a0 == a1 under the 117-bit split
        assert v & lo == v >> 117 and v >> 117 < 1 << 116
    assert len(gc.equal_halves()) >= 5
    for k in range(1, 8):
        assert {1 << (32 * k - 1), 1 << (32 * k)} <= e
    assert sum(0xC0000000 << (32 * w) for w in range(7)) in e
    # every digit value at every comb position of one word: 10 three-bit positions x 7 values + the 2-bit top digit's 3
    d = gc.digit_values()
    assert len(d) == 73 and set(d) <= e
    sh = 32 * gc.DIGIT_WORD
    assert {(v << (3 * pos)) << sh for pos in range(10) for v in range(1, 8)} | {v << (sh + 30) for v in (1, 2, 3)} == set(d)
    assert (1 << (32 * gc.DIGIT_WORD + 21)) in d  # the bit where gf_k_split cuts
    r = gc.random_values()
    assert len(r) == 2000 and len(set(r)) == 2000 and all(0 <= x <= gc.MASK for x in r)
    assert sum(bin(x).count("1") for x in r) > 2000 * 100  # dense
    assert all(0 <= x <= gc.MASK for x in f)


def test_multiplication_sets():
    bp = gc.mul_basis_pairs()
    assert len(bp) == 233 * 233 == 54289 and len(set(bp)) == 54289
    assert set(bp) == {(1 << i, 1 << j) for i in range(233) for j in range(233)}
    op = gc.mul_other_pairs()
    ne = len(gc.edge_values())
    assert len(op) == ne * ne + 2000
    assert set(op[:ne * ne]) == {(a, b) for a in gc.edge_values() for b in gc.edge_values()}
    # both first operands of MUL2 sweep the whole basis grid
    t = gc.mul2_triples(bp, 97)
    assert {(a1, b) for a1, _, b in t} == set(bp) and {(a2, b) for _, a2, b in t} == set(bp)
    t = gc.mul2_triples(op, 1)
    assert [(a1, b) for a1, _, b in t] == list(op) and [a2 for _, a2, _ in t] == [a for a, _ in op[1:] + op[:1]]
    assert gc.MUL_LEAD[0] & 7 == 0 and gc.MUL_LEAD[0] <= gc.MASK
    # the run lengths put one active lane, quad and row of 16 into the last wave
    assert gc.RUN_LENGTHS == (1, 3, 63, 64, 65, 257)
    ch = gc.chunks(1000)
    assert [ln for _, ln in ch[:6]] == list(gc.RUN_LENGTHS) and sum(ln for _, ln in ch) == 1000
    assert all(a + ln == b for (a, ln), (b, _) in zip(ch, ch[1:]))


def test_table_and_reduce_sets():
    t = gc.tab_entries()
    assert len(t) == 30 * 256 + 300
    assert set(t[:30 * 256]) == {(byte << (8 * pos)) & gc.MASK for pos in range(30) for byte in range(256)}
    assert max(t[29 * 256:30 * 256]) == 1 << 232
    assert set(gc.TABLES) == {"t29", "t58", "t116", "th", "t14", "t7"}
    for top in (14, 15):
        r = gc.reduce_inputs(top)
        bits = 32 * (top + 1)
        assert {1 << i for i in range(bits)} <= set(r) and max(r) < 1 << bits
    assert {0, 1, gc.MASK} <= set(gc.inv_values()) and set(gc.basis()) <= set(gc.inv_values()) and len(gc.inv_values()) >= 500


def test_pyref_and_c_oracle_agree_on_the_multiplication_and_inversion_sets():
    pairs = gc.mul_basis_pairs() + gc.mul_other_pairs()
    want = gc.mul_expected("basis") + gc.mul_expected("other")
    lib = co.lib()
    a = np.frombuffer(gc.pack([p[0] for p in pairs]), dtype="<u8").reshape(-1, 4).copy()
    b = np.frombuffer(gc.pack([p[1] for p in pairs]), dtype="<u8").reshape(-1, 4).copy()
    out = np.zeros_like(a)
    for i in range(len(pairs)):
        lib.dvo_gf_mul(a[i].ctypes.data, b[i].ctypes.data, out[i].ctypes.data)
    assert out.tobytes() == gc.pack(want)
    for v in gc.inv_values():
        if v:
            assert co.gf_inv(v) == gc.inv(v) and o.gf_mul(v, gc.inv(v)) == 1
    assert gc.inv(0) == 0


def test_combined_references_are_pyrefs_own_functions():
    """frob / halftrace / trace combine pyref's values on the basis: the same as pyref's functions on whole operands"""
    rnd = random.Random(5)
    vals = [gc.MASK, (1 << 232) | 1] + [rnd.getrandbits(233) for _ in range(6)] + [1 << 159, 1, 1 << 232]
    for v in vals:
        for k in (1, 7, 14, 29, 58, 116, 232):
            assert gc.frob(v, k) == o.gf_pow2k(v, k)
        assert gc.frob(v, 0) == v and gc.frob(v, 232) == o.gf_sqrt(v)
        assert gc.halftrace(v) == o.gf_halftrace(v)
        assert gc.trace(v) == o.gf_trace_def(v) == o.gf_trace(v)
    assert [i for i in range(233) if gc.trace(1 << i)] == [0, 159]
    for top in (14, 15):
        for c in gc.reduce_inputs(top)[-5:]:
            assert o.gf_reduce(c) == o.gf_mul(o.gf_reduce(c), 1) <= gc.MASK


@pytest.mark.parametrize("op", sorted(gc.POINT_OPS))
def test_point_cases_are_on_the_curve_and_cover_their_classes(op):
    ks = gc.FROB_KS if op == "ld_frob_n" else (0,)
    for k in ks:
        cases = gc.point_cases(op, k)
        classes = {c.cls for c in cases}
        kp, kq, _ = gc.POINT_OPS[op]
        if kq is None:
            assert {"generic", "infinity"} <= classes and (op != "ld_dbl" or "order-2" in classes)
        elif op == "ld_add_aff_aff":
            assert classes == {"generic"}
        elif op == "ld_madd_fast":
            assert classes == {"generic", "P+P", "P-P"}
        elif kq == "aff":
            assert classes == {"generic", "P+P", "P-P", "inf+Q"}
        else:
            assert classes == {"generic", "P+P", "P-P", "inf+Q", "P+inf", "inf+inf"}
        for c in cases:
            assert all(0 <= v <= gc.MASK for v in c.ins)
            assert c.want is None or (o.k233_on_curve(c.want) and c.want[0] != 0)
            pts = gc.case_affine_inputs(op, c)
            for pt in pts:
                assert pt is None or o.k233_on_curve(pt)
            if c.cls == "order-2":
                assert pts[0] == o.N_STD and o.k233_dbl(pts[0]) is None
            elif kq is None:
                want = {"ld_dbl": o.k233_dbl, "lam_dbl": o.k233_dbl}.get(op, lambda p: p)(pts[0])
                if op == "ld_frob_n" and want is not None:
                    want = (o.gf_pow2k(want[0], k), o.gf_pow2k(want[1], k))
                assert c.want == want
            else:
                assert c.want == o.k233_add(pts[0], pts[1])
                if c.cls in ("P+P", "P-P"):  # two different representatives
                    assert pts[0][0] == pts[1][0] and (kq == "aff" or c.ins[2] != c.ins[5])
                    assert (pts[0] == pts[1]) == (c.cls == "P+P")
    # the representatives really use every Z of the list, and the points come from the C oracle's k G
    assert len(set(gc.Z_VALUES)) == 4 and {1, 2, gc.MASK} <= set(gc.Z_VALUES)
    assert gc.points()[0] == o.G_STD and gc.points()[1] == o.k233_dbl(o.G_STD)


# ---- the entry's preconditions: rejected on the host, with the index, without a device call --------------------------------------------
def _call(dvp, name, form, ins, param=0, n=None):
    op, n_in, n_out, flag = dvp.gf.DEBUG_OPS[name]
    n = len(ins[0]) // 32 if n is None else n
    bufs = [np.frombuffer(b, dtype="<u8").copy() for b in ins]
    outs = [np.zeros(4 * max(n, 1) * 16, dtype=np.uint64) for _ in range(4)]
    pin = (C.c_void_p * 6)(*[a.ctypes.data for a in bufs])
    pout = (C.c_void_p * 4)(*[a.ctypes.data for a in outs])
    st = dvp.lib.dvp_debug_gf_op(op, dvp.gf.FORMS[form], pin, n, param, pout)
    return st, dvp.lib.dvp_last_error_index()


def test_binding_matches_the_header(dvp):
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvpari_internal.h")).read()
    ops = re.findall(r"DVP_GFOP_([A-Z0-9_]+)", hdr.split("enum dvp_gf_op")[1].split("};")[0])
    assert [x.lower() for x in ops if x != "COUNT"] == list(dvp.gf.DEBUG_OPS)
    forms = re.findall(r"DVP_GFFORM_([A-Z]+)", hdr.split("enum dvp_gf_form")[1].split("};")[0])
    assert [x.lower() for x in forms if x != "COUNT"] == list(dvp.gf.FORMS)
    assert set(dvp.gf.SQR_TABS) == set(gc.TABLES) and all(dvp.gf.SQR_TABS[t][1] == gc.TABLES[t] for t in gc.TABLES)


def test_operand_out_of_range_is_rejected_with_its_index(dvp):
    good = [1, gc.MASK, 1 << 232, 5, 7, 9, 11]
    for name, (op, n_in, n_out, flag) in dvp.gf.DEBUG_OPS.items():
        if name.startswith("reduce16"):
            continue
        form = dvp.gf.op_forms(name)[-1]
        for k in range(n_in):
            for idx in (0, 3, 6):
                for bad in (1 << 233, 1 << 255, gc.MASK + 1 + 5):
                    ins = [list(good) for _ in range(n_in)]
                    ins[k][idx] = bad
                    assert _call(dvp, name, form, [gc.pack(v) for v in ins]) == (-1, idx), (name, k, idx)


def test_reduce16_word_15_and_params_are_rejected(dvp):
    lo = gc.pack([1, 2, 3])
    hi = [(1 << 224) - 1] * 3
    hi[2] = 1 << 224  # word 15
    assert _call(dvp, "reduce16_14", "reg", [lo, gc.pack(hi)]) == (-1, 2)
    hi[1] = (1 << 256) - 1
    assert _call(dvp, "reduce16_14", "reg", [lo, gc.pack(hi)]) == (-1, 1)
    one = [gc.pack([1])]
    for name in ("sqr_n", "sqr_n_fast"):
        assert _call(dvp, name, "reg", one, 233) == (-1, -1)
        assert _call(dvp, name, "reg", one, 1 << 40) == (-1, -1)
    assert _call(dvp, "ld_frob_n", "reg", one * 3, 233) == (-1, -1)
    # tables: an unknown selector, stray bits, and a table the current DVP_GF_INV_TABS does not provide
    for param in (6, 255, 0x200, 0x106, 1 << 32):
        assert _call(dvp, "sqr_tab", "reg", one, param) == (-1, -1), param
    t14, t7 = dvp.gf.SQR_TABS["t14"][0], dvp.gf.SQR_TABS["t7"][0]
    for tabs, missing in ((0, (t14, t7)), (1, (t7,))):
        with dvp.tune(DVP_GF_INV_TABS=tabs):
            for sel in missing:
                for wide in (0, dvp.gf.SQR_TAB_WIDE):
                    assert _call(dvp, "sqr_tab", "reg", one, sel | wide) == (-1, -1), (tabs, sel)
    v = C.c_longlong(-1)
    assert dvp.lib.dvp_tune_get(b"DVP_GF_INV_TABS", C.byref(v)) == 0 and v.value == 1  # the default provides t14 only
    assert _call(dvp, "sqr_tab", "reg", one, t7) == (-1, -1)


def test_bad_calls_are_rejected(dvp):
    one = gc.pack([1])
    for name in dvp.gf.DEBUG_OPS:
        n_in = dvp.gf.DEBUG_OPS[name][1]
        for form in dvp.gf.FORMS:
            if form not in dvp.gf.op_forms(name):  # a form the function does not exist in
                assert _call(dvp, name, form, [one] * n_in)[0] == -1, (name, form)
            else:  # nothing to do
                assert _call(dvp, name, form, [one] * n_in, n=0)[0] == 0, (name, form)
    lib = dvp.lib
    buf, out = (C.c_void_p * 6)(), (C.c_void_p * 4)()
    assert lib.dvp_debug_gf_op(-1, 0, buf, 0, 0, out) == -1
    assert lib.dvp_debug_gf_op(len(dvp.gf.DEBUG_OPS), 0, buf, 0, 0, out) == -1
    assert lib.dvp_debug_gf_op(0, -1, buf, 0, 0, out) == -1
    assert lib.dvp_debug_gf_op(0, len(dvp.gf.FORMS), buf, 0, 0, out) == -1
    assert lib.dvp_debug_gf_op(0, 0, buf, 1, 0, out) == -1  # null operands
    assert lib.dvp_debug_gf_op(0, 0, None, 1, 0, out) == -1
    a = np.zeros(4, dtype=np.uint64)
    buf[0] = buf[1] = a.ctypes.data
    assert lib.dvp_debug_gf_op(0, 0, buf, 1, 0, out) == -1  # null result
    out[0] = a.ctypes.data
    assert lib.dvp_debug_gf_op(1, 3, buf, 1 << 28, 0, out) == -1  # n x 16 lanes does not fit 31 bits
