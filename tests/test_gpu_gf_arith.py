"""The device build of every function of csrc/gf233.cuh and every point formula of csrc/k233.cuh, one function per element
(dvp_debug_gf_op), against oracle/pyref.py on the case sets of gf_cases.py.  Bit-exact: the field is exact, no tolerance anywhere.

The products and the table passes are checked EXHAUSTIVELY for everything that keeps them (bi)linear -- all 233^2 basis pairs in every
multiplier form, all 30 x 256 entries of every table (see gf_cases.py for the argument); edge and random operands, calls of 1, 3, 63, 64,
65 and 257 elements and a lane working through several elements in one LDS region cover what is not linear.  For the quad and row forms
every lane's copy of every result is compared.  The point formulas are checked against the affine group law after normalising the
device's (X, Y, Z), and word for word across the multiplier forms."""
import numpy as np
import pytest

import gf_cases as gc

pytestmark = pytest.mark.gpu

FORMS = ("reg", "lds", "ldsq", "ldsh", "ldsk")
LDS_FORMS = FORMS[1:]


def run(dvp, op, form, cols, param=0):
    """cols: one list of values per operand -> one bytes object per output, the lanes' copies checked equal and folded into one"""
    n = len(cols[0])
    outs = dvp.gf.debug_op(op, form, [gc.pack(c) for c in cols], param)
    g = dvp.gf.LANES[form]
    if g == 1:
        return outs
    folded = []
    for k, buf in enumerate(outs):
        a = np.frombuffer(buf, dtype="<u8").reshape(n, g, 4)
        same = (a == a[:, :1, :]).all(axis=(1, 2))
        assert same.all(), (op, form, "output", k, "element", int(np.argmin(same)), "lanes disagree", a[int(np.argmin(same))].tolist())
        folded.append(a[:, 0, :].tobytes())
    return folded


def run_in_runs(dvp, op, form, cols, param=0, lead=None):
    """the same elements in consecutive calls of gc.RUN_LENGTHS elements, each call led by `lead` where one is given"""
    n = len(cols[0])
    parts = None
    for at, ln in gc.chunks(n):
        sub = [list(c[at:at + ln]) for c in cols]
        if lead is not None:
            ln0 = max(ln - 1, 0)
            sub = [[lv] + s[:ln0] for lv, s in zip(lead, sub)]  # the call keeps its length: the lead takes the last element's place
        outs = run(dvp, op, form, sub, param)
        if lead is not None:
            outs = [b[32:] + bytes(32) for b in outs]
        parts = [p + b for p, b in zip(parts, outs)] if parts else outs
    return parts


def same(what, got: bytes, want_vals, cols=None):
    want = gc.pack(want_vals)
    if got == want:
        return
    g = gc.unpack(got)
    i = next(k for k in range(len(want_vals)) if g[k] != want_vals[k])
    ins = [hex(c[i]) for c in cols] if cols else None
    raise AssertionError(f"{what}: element {i} of {len(want_vals)}: got {g[i]:#x}, want {want_vals[i]:#x}, operands {ins}")


def with_lead(pairs, lead):
    return [[lead[k]] + [p[k] for p in pairs] for k in range(len(lead))]


# ---- products ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ("basis", "other"))
def test_mul_every_basis_pair_edges_and_random(dvp, form, which):
    pairs = gc.mul_basis_pairs() if which == "basis" else gc.mul_other_pairs()
    cols = with_lead(pairs, gc.MUL_LEAD)
    want = [gc.o.gf_mul(*gc.MUL_LEAD)] + list(gc.mul_expected(which))
    same(f"gf_mul[{form}]", run(dvp, "mul", form, cols)[0], want, cols)


@pytest.mark.parametrize("form", LDS_FORMS)
@pytest.mark.parametrize("which", ("basis", "other"))
def test_mul2_every_basis_pair_edges_and_random_in_both_products(dvp, form, which):
    pairs = gc.mul_basis_pairs() if which == "basis" else gc.mul_other_pairs()
    rot = 97 if which == "basis" else 1
    tri = gc.mul2_triples(pairs, rot)
    lead = (gc.MUL_LEAD[0], gc.MUL_LEAD[0] ^ 8, gc.MUL_LEAD[1])
    cols = with_lead(tri, lead)
    exp = gc.mul_expected(which)
    n = len(pairs)
    if which == "basis":  # a2 b = the product of the pair `rot` rows on
        want2 = [exp[((i // gc.M + rot) % gc.M) * gc.M + i % gc.M] for i in range(n)]
    else:
        want2 = [gc.o.gf_mul(a2, b) for _, a2, b in tri]
    r1, r2 = run(dvp, "mul2", form, cols)
    same(f"gf_mul2[{form}] first", r1, [gc.o.gf_mul(lead[0], lead[2])] + list(exp), cols)
    same(f"gf_mul2[{form}] second", r2, [gc.o.gf_mul(lead[1], lead[2])] + want2, cols)


@pytest.mark.parametrize("form", FORMS)
def test_products_in_short_and_ragged_calls(dvp, form):
    """calls of 1, 3, 63, 64, 65 and 257 elements (a lone lane / quad / row in the last wave), each led by an operand whose low comb
    digit is zero; the elements of a call beyond its first 64 / 16 / 4 are a lane's second element in the same LDS region"""
    other, exp = gc.mul_other_pairs(), gc.mul_expected("other")
    idx = list(range(0, len(other), 9))[:2 * sum(gc.RUN_LENGTHS)]
    pairs = [other[i] for i in idx]
    want = [exp[i] for i in idx]
    cols = [[p[0] for p in pairs], [p[1] for p in pairs]]
    got = run_in_runs(dvp, "mul", form, cols, lead=gc.MUL_LEAD)[0]
    # the lead displaced the last element of every call: those are not compared
    keep = [k for at, ln in gc.chunks(len(pairs)) for k in range(at, at + ln - 1)]
    g = gc.unpack(got)
    for k in keep:
        assert g[k] == want[k], (form, k, hex(pairs[k][0]), hex(pairs[k][1]))
    assert len(pairs) == 2 * sum(gc.RUN_LENGTHS) and len(keep) == len(pairs) - 2 * len(gc.RUN_LENGTHS)
    if form != "reg":
        a2 = cols[0][1:] + cols[0][:1]
        r1, r2 = run_in_runs(dvp, "mul2", form, [cols[0], a2, cols[1]])
        same(f"gf_mul2[{form}] runs, first", r1, want)
        same(f"gf_mul2[{form}] runs, second", r2, [gc.o.gf_mul(a, b) for a, b in zip(a2, cols[1])])


# ---- the linear functions ---------------------------------------------------------------------------------------------------------------
def test_add_sqr_sqrt_trace_halftrace(dvp):
    v = list(gc.field_values())
    w = v[7:] + v[:7]
    same("gf_add", run(dvp, "add", "reg", [v, w])[0], [a ^ b for a, b in zip(v, w)])
    same("gf_sqr", run(dvp, "sqr", "reg", [v])[0], [gc.frob(a, 1) for a in v], [v])
    same("gf_sqrt", run(dvp, "sqrt", "reg", [v])[0], [gc.frob(a, 232) for a in v], [v])
    same("gf_trace", run(dvp, "trace", "reg", [v])[0], [gc.trace(a) for a in v], [v])
    same("gf_halftrace", run(dvp, "halftrace", "reg", [v])[0], [gc.halftrace(a) for a in v], [v])
    same("gf_sqr in runs", run_in_runs(dvp, "sqr", "reg", [v])[0], [gc.frob(a, 1) for a in v], [v])


@pytest.mark.parametrize("op", ("sqr_n", "sqr_n_fast"))
def test_repeated_squaring_around_every_table_run(dvp, op):
    v = list(gc.field_values())
    for k in gc.KS:
        same(f"gf_{op}({k})", run(dvp, op, "reg", [v], k)[0], [gc.frob(a, k) for a in v], [v])


@pytest.mark.parametrize("top", (15, 14))
def test_reduce16_every_bit(dvp, top):
    vals = gc.reduce_inputs(top)
    lo, hi = gc.split512(vals)
    same(f"gf_reduce16<{top}>", run(dvp, f"reduce16_{top}", "reg", [lo, hi])[0], [gc.o.gf_reduce(c) for c in vals], [lo, hi])


@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("table", sorted(gc.TABLES))
def test_table_pass_every_entry(dvp, table, wide):
    v = list(gc.tab_entries())
    sel = dvp.gf.SQR_TABS[table][0] | (dvp.gf.SQR_TAB_WIDE if wide else 0)
    with dvp.tune(DVP_GF_INV_TABS=2):
        got = run(dvp, "sqr_tab", "reg", [v], sel)[0]
        runs = run_in_runs(dvp, "sqr_tab", "reg", [v[-600:]], sel)[0]
    want = [gc.table_map(table, a) for a in v]
    same(f"table {table} wide={wide}", got, want, [v])
    same(f"table {table} wide={wide} in runs", runs, want[-600:])


# ---- inversion --------------------------------------------------------------------------------------------------------------------------
def _check_inverse(dvp, what, form, v, got):
    same(what, got, [gc.inv(a) for a in v], [v])
    # and on the device's own output: a inv(a) = 1
    prod = run(dvp, "mul", form, [v, gc.unpack(got)])[0]
    same(what + ": a inv(a)", prod, [1 if a else 0 for a in v], [v])


def test_inv_register_chain(dvp):
    v = list(gc.inv_values())
    _check_inverse(dvp, "gf_inv", "reg", v, run(dvp, "inv", "reg", [v])[0])


@pytest.mark.parametrize("tabs", (0, 1, 2))
@pytest.mark.parametrize("form", LDS_FORMS)
def test_inv_fast_every_form_every_table_setting(dvp, form, tabs):
    v = list(gc.inv_values())
    with dvp.tune(DVP_GF_INV_TABS=tabs):
        got = run(dvp, "inv_fast", form, [v])[0]
        runs = run_in_runs(dvp, "inv_fast", form, [v[:200]])[0]
    _check_inverse(dvp, f"gf_inv_fast[{form}, tabs={tabs}]", form, v, got)
    assert runs == got[:32 * 200]


# ---- point formulas ---------------------------------------------------------------------------------------------------------------------
def _verify(op, cases, outs):
    kinds = gc.POINT_OPS[op]
    cols = [gc.unpack(b) for b in outs]
    for i, c in enumerate(cases):
        tag = (op, i, c.cls)
        if op == "ld_to_aff":
            x, y, flag = cols[0][i], cols[1][i], cols[2][i]
            assert flag == c.flag, tag
            assert (x, y) == (c.want if c.want is not None else (0, 0)), tag
            continue
        X, Y, Z = cols[0][i], cols[1][i], cols[2][i]
        if c.flag is not None:
            assert cols[3][i] == c.flag, tag
        if c.untouched:  # "returns false -- p untouched"
            assert (X, Y, Z) == c.ins[:3], tag
        elif c.want is None:
            assert Z == 0, tag
        else:
            assert Z != 0, tag
            assert (gc.lam_norm if kinds[2] == "lam" else gc.ld_norm)(X, Y, Z) == c.want, tag


def _point_op(dvp, op, k=0):
    cases = gc.point_cases(op, k)
    cols = [[c.ins[j] for c in cases] for j in range(len(cases[0].ins))]
    first = None
    for form in dvp.gf.op_forms(op):
        outs = run(dvp, op, form, cols, k)
        assert run_in_runs(dvp, op, form, cols, k) == outs, (op, form, "calls of other lengths give other words")
        if first is None:
            first, first_form = outs, form
            _verify(op, cases, outs)
            continue
        # the formulas are the same and the field is exact: the same words in every form.  (The register functions return q where the
        # in-place ones keep p for infinity + infinity, and either is an infinity: a register result is compared where it is finite.)
        if first_form == "reg":
            z = gc.unpack(first[2])
            for j, (a, b) in enumerate(zip(first, outs)):
                ua, ub = gc.unpack(a), gc.unpack(b)
                for i in range(len(cases)):
                    assert ua[i] == ub[i] or (j < 2 and z[i] == 0), (op, form, i, cases[i].cls, j)
            _verify(op, cases, outs)
            first, first_form = outs, form
        else:
            assert outs == first, (op, form, "differs from", first_form)


@pytest.mark.parametrize("op", sorted(o for o in gc.POINT_OPS if o != "ld_frob_n"))
def test_point_formula_every_form_every_class(dvp, op):
    _point_op(dvp, op)


def test_frobenius(dvp):
    for k in gc.FROB_KS:
        _point_op(dvp, "ld_frob_n", k)


@pytest.mark.parametrize("form", LDS_FORMS)
def test_add_aff_aff_is_the_mixed_addition_with_z_1_word_for_word(dvp, form):
    cases = gc.point_cases("ld_add_aff_aff")
    px, py, qx, qy = [[c.ins[j] for c in cases] for j in range(4)]
    one = [1] * len(cases)
    assert run(dvp, "ld_add_aff_aff", form, [px, py, qx, qy]) == run(dvp, "ld_madd", form, [px, py, one, qx, qy])
