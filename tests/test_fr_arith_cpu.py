"""The host build of every Fr function of csrc/fr.cuh (dvp_debug_fr_op, on_device = 0: no HIP call, no GPU) against exact Python
integers on the chosen operands of fr_cases.py; the case set's own branch coverage, judged on the reference alone; the entry's
precondition checks; and the argument checks of dvp_fr_spmv / dvp_fr_vec_dot that return before any device work.
Every assertion is integer (byte) equality."""
import ctypes as C

import numpy as np
import pytest

import fr_cases as fc

P = fc.P


def test_edge_values():
    e = fc.edge_values()
    assert 1300 <= len(e) <= 1800 and all(0 <= x < P for x in e) and len(set(e)) == len(e)
    s = set(e)
    must = [0, 1, 2, 3, P - 1, P - 2, P - 3, (P - 1) // 2, (P + 1) // 2, P // 3, fc.R % P, fc.R ** 2 % P, fc.R ** 3 % P, pow(fc.R, -1, P),
            fc.R30 % P, fc.R30 ** 2 % P, fc.R30 ** 3 % P, pow(fc.R30, -1, P)]
    must += [(1 << k) + d for k in range(1, 231) for d in (-1, 0, 1)] + [P - (1 << k) + d for k in range(1, 231) for d in (-1, 0, 1)]
    must += [(1 << 231) - 1, 1 << 231, (1 << 231) + 1, (1 << 29) - 1, (1 << 30) - 1, (1 << 32) - 1, ((1 << 29) - 1) << 29]
    assert all(x in s for x in must)
    # the GCD's "close" case: values that agree with p in more than 100 top bits
    assert sum(1 for x in e if (x ^ P) >> 131 == 0) >= 300
    assert sum(1 for x in e if x & 0x3FFFFFFF == 0) >= 100 and sum(1 for x in e if x & 0x3FFFFFFF == 0x3FFFFFFF) >= 100
    assert len(fc.pairs()) >= 40 * len(e)
    assert all(len(fc.cases(op)) < 10 ** 5 for op in fc.OPS if not op.startswith("inv"))
    assert len(fc.inversion_inputs()) >= len(e) + (1 << 17)
    # inversion: inputs whose binary GCD finishes in each of the later rounds of 30 steps, the last (steps 451 .. 480) included
    rounds = {(fc.gcd_steps(y) + 29) // 30 for y in e}
    assert rounds >= set(range(9, 17)), sorted(rounds)


def test_branch_coverage():
    """the case set reaches every branch the reference can tell apart.  fr_dot2's second conditional subtraction (T >= 2p) needs
    a0 b0 + a1 b1 within a margin of 2^-116 of its maximum; the near-p cases do not reach it and it is not required here
    (fr_muladd29 shares the double subtraction and reaches it thousands of times)."""
    b = fc.branches("add")
    assert b["sum<p"] > 1000 and b["sum=p"] >= 100 and b["sum>p"] > 1000
    b = fc.branches("sub")
    assert b["borrow"] > 1000 and b["no borrow"] > 1000 and b["a=b"] > 1000
    b = fc.branches("cond_sub_p")
    assert all(b.get(k) for k in ("p-1", "p", "p+1", "2p-1"))
    for op in ("mul", "mul29"):
        b = fc.branches(op)
        assert b["T<p"] > 1000 and b["T>=p"] > 1000
        assert all(b.get(k, 0) >= 48 for k in ("T=p+1", "T=p+2", "T=p-1", "T=p-2")), b
    b = fc.branches("muladd29")
    assert b["0 subtractions"] > 1000 and b["1 subtractions"] > 1000 and b["2 subtractions"] > 1000, b
    b = fc.branches("dot2")
    assert b["0 subtractions"] > 1000 and b["1 subtractions"] > 1000, b
    # lazy products: results on both sides of every power of two a limb-7 mask could cut at
    t = fc.unpack(fc.expected("muladd30")[0])
    assert min(t) == 0 and max(t) >= (1 << 240) - 2 and sum(1 for x in t if x >> 239) > 100 and sum(1 for x in t if x >> 232) > 10000
    t0, t1 = (fc.unpack(b) for b in fc.expected("muladd30_x2"))
    assert sum(1 for x in t1 if x >> 239) > 100 and sum(1 for x, y in zip(t0, t1) if x != y) > len(t0) - 100
    d = fc.unpack(fc.expected("sub_lazy30")[0])
    assert min(d) == 1 and max(d) == (1 << 239) - 1 + 128 * P  # 0 - (128 p - 1) and (2^239 - 1) - 0


@pytest.mark.parametrize("op", fc.OPS)
def test_host_op_vs_integers(dvp, op):
    fc.assert_same(op, fc.run_op(dvp, op, False), fc.expected(op))


def test_zero_inverts_to_zero(dvp):
    for op in ("inv", "inv_gcd_raw", "inv_fermat"):
        assert dvp.fr.debug_op(op, [fc.pack([0, 1, 0])], False)[0][:32] == bytes(32)


# one value just outside every op's precondition, in operand `slot`, with valid company
OUTSIDE = [("add", 0, P), ("add", 1, P), ("sub", 1, P), ("neg", 0, P), ("dbl", 0, P), ("cond_sub_p", 0, 2 * P), ("mul", 0, P), ("mul", 1, P),
           ("sqr", 0, P), ("to_mont", 0, P), ("from_mont", 0, P), ("dot2", 0, P), ("dot2", 3, P), ("muladd29", 2, P), ("mul29", 1, P),
           ("roundtrip29", 0, 1 << 232), ("roundtrip30", 0, 1 << 240), ("const30", 0, P), ("canon30", 0, 2 * P),
           ("sub_lazy30", 0, 1 << 239), ("sub_lazy30", 1, 128 * P), ("muladd30", 0, P), ("muladd30", 1, 1 << 240), ("muladd30", 2, 1 << 240),
           ("muladd30", 2, (1 << 240) - 1), ("muladd30_x2", 3, P), ("muladd30_x2", 5, 1 << 240), ("inv", 0, P), ("inv_gcd_raw", 0, P),
           ("inv_fermat", 0, fc.M256), ("pow_u64", 0, P), ("pow_u64", 1, 1 << 64), ("limbs29", 0, 1 << 232), ("limbs30", 0, 1 << 240)]


@pytest.mark.parametrize("op,slot,value", OUTSIDE)
def test_precondition_is_enforced(dvp, op, slot, value):
    """an operand outside the precondition is DVP_EINVAL with its index, on both flavours, before anything runs (so without a GPU)"""
    n_in = dvp.fr.DEBUG_OPS[op][1]
    vals = [[1, 1, 1, 1, 1] for _ in range(n_in)]
    assert dvp.fr.debug_op(op, [fc.pack(v) for v in vals], False)  # the company is valid
    vals[slot][3] = value
    for on_device in (False, True):
        with pytest.raises(dvp.DvpError) as ei:
            dvp.fr.debug_op(op, [fc.pack(v) for v in vals], on_device)
        assert ei.value.status == -1 and ei.value.index == 3


def test_debug_entry_argument_checks(dvp):
    lib = dvp.lib
    buf = (C.c_void_p * 6)()
    out = (C.c_void_p * 2)()
    assert lib.dvp_debug_fr_op(-1, buf, 0, 0, out) == -1
    assert lib.dvp_debug_fr_op(len(dvp.fr.DEBUG_OPS), buf, 0, 0, out) == -1
    assert lib.dvp_debug_fr_op(0, buf, 1, 0, out) == -1  # null operand
    assert lib.dvp_debug_fr_op(0, buf, 0, 0, out) == 0  # nothing to do
    assert list(dvp.fr.DEBUG_OPS) == list(fc.OPS)


def _spmv_status(dvp, row_ptr, col, cid, n_coeffs=2, n_cols=3):
    rp = np.asarray(row_ptr, dtype=np.uint32)
    col, cid = np.asarray(col, dtype=np.uint32), np.asarray(cid, dtype=np.uint32)
    coeffs, x = np.ones((n_coeffs, 4), dtype=np.uint64), np.ones((n_cols, 4), dtype=np.uint64)
    out = np.zeros((len(rp) - 1, 4), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    st = dvp.lib.dvp_fr_spmv(p(rp), p(col), p(cid), len(rp) - 1, p(coeffs), n_coeffs, p(x), n_cols, p(out))
    return st, dvp.lib.dvp_last_error_index()


def test_spmv_rejects_malformed_rows(dvp):
    """a row_ptr that is not non-decreasing, or that points past row_ptr[n_rows], would send the kernel out of col / coeff_ids: it is
    refused with the row's index before any device call (so this runs without a GPU), like a column or coefficient id out of range"""
    col, cid = [0, 1, 2, 0], [0, 1, 0, 1]
    assert _spmv_status(dvp, [0, 3, 2, 4], col, cid) == (-1, 1)  # row 1 runs backwards
    assert _spmv_status(dvp, [0, 2, 9, 4], col, cid) == (-1, 1)  # row 1 ends past the last offset
    assert _spmv_status(dvp, [5, 5, 5, 4], col, cid) == (-1, 0)  # starts above the end
    assert _spmv_status(dvp, [0, 0xFFFFFFFF, 4], col, cid) == (-1, 0)
    assert _spmv_status(dvp, [0, 2, 4], col, cid, n_cols=2) == (-1, 2)  # col[2] = 2 >= n_cols
    assert _spmv_status(dvp, [0, 2, 4], col, cid, n_coeffs=1) == (-1, 1)
    assert _spmv_status(dvp, [0, 2, 4], [], cid)[0] == -1  # entries, but no column array
    assert _spmv_status(dvp, [0, 2, 4], col, [])[0] == -1


def test_empty_dot_reads_nothing(dvp):
    """<a, b> over no elements is 0 and touches neither operand (null pointers are fine) nor the device"""
    out = np.full(4, 7, dtype=np.uint64)
    assert dvp.lib.dvp_fr_vec_dot(None, None, 0, out.ctypes.data_as(C.c_void_p)) == 0
    assert not out.any()
    assert dvp.lib.dvp_fr_vec_dot(None, None, 0, None) == -1
    assert dvp.lib.dvp_fr_vec_dot(None, out.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == -1
