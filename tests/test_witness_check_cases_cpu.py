"""CPU: the restatement of the witness check (tests/witness_check_cases.py) pinned on the toy circuit by values worked out by hand, and
every case of the GPU test checked to do what it is meant to do -- a case that quietly stops failing breaks HERE, instead of passing
the GPU test with an empty list."""
import pytest

import pyref as o
import witness_check_cases as wcc

P = o.P
# src/dvsnark_test.rs:84-115 -- wires 1=0, o=1, w=2, y=3, z=4, x=5, t=6, s=7; x*x = y, y + z = w, 2z = t, x + t = s, w + s = o
TOY_W = [1, 24, 13, 9, 4, 3, 8, 11]


def toy(w_raw, n_public=2):
    return wcc.restate(o.TOY_ROWS, o.TOY_COEFFS, n_public, 8, w_raw, wcc.domain(3))


def test_toy_witness_satisfies():
    r = toy(TOY_W)
    assert r == {"n_unsat": 0, "first_unsat": -1, "n_noncanonical": 0, "first_noncanonical": -1, "n_suspect_wires": 0,
                 "constant_wire_is_one": True, "rows": [], "wires": []}


def test_toy_with_z_changed_by_hand():
    """z = 5 instead of 4: row 1 reads (y + z) * 1 = 14 against w = 13, row 2 reads 2 z * 1 = 10 against t = 8; rows 0, 3, 4 hold.
    Failing rows touch wires {y, z, 1, w} and {z, 1, t}; the satisfied ones touch {x, y}, {x, t, 1, s}, {w, s, 1, o}: only z is in
    failing rows alone, with two terms."""
    w = list(TOY_W)
    w[4] = 5
    r = toy(w)
    d = wcc.domain(3)
    assert (r["n_unsat"], r["first_unsat"], r["n_noncanonical"], r["first_noncanonical"]) == (2, 1, 0, -1)
    assert [x["row"] for x in r["rows"]] == [1, 2]
    assert [(x["a"], x["b"]) for x in r["rows"]] == [(14, 1), (10, 1)]
    for x, cw in zip(r["rows"], (13, 8)):
        assert x["i"] == (24 + 13 * d[x["row"]]) % P  # pub_0 + pub_1 d_row
        assert (x["c"] + x["i"]) % P == cw and x["a"] * x["b"] % P != cw
    assert r["wires"] == [(4, 2)] and r["n_suspect_wires"] == 1
    # without public inputs i vanishes and c is C w itself
    r0 = toy(w, n_public=0)
    assert [(x["c"], x["i"]) for x in r0["rows"]] == [(13, 0), (8, 0)]


def test_toy_with_x_changed_counts_every_term():
    """x = 4: row 0 (16 != 9) and row 3 (12 != 11) fail.  x lies in failing rows only (3 terms: twice in row 0, once in row 3); y lies
    in row 1, which holds, so it is not suspect; s lies in row 4, which holds."""
    w = list(TOY_W)
    w[5] = 4
    r = toy(w)
    assert [x["row"] for x in r["rows"]] == [0, 3] and r["wires"] == [(5, 3)]


def test_toy_entries_not_below_p():
    w = list(TOY_W)
    w[5] += P          # another representative of x: nothing fails
    w[7] += 3 * P
    r = toy(w)
    assert (r["n_unsat"], r["n_noncanonical"], r["first_noncanonical"], r["constant_wire_is_one"]) == (0, 2, 5, True)
    w[0] = P           # the constant wire reduces to 0: rows 1 .. 4 multiply by it
    r = toy(w)
    assert (r["n_noncanonical"], r["first_noncanonical"], r["constant_wire_is_one"]) == (3, 0, False)
    assert [x["row"] for x in r["rows"]] == [1, 2, 3, 4] and all(x["b"] == 0 for x in r["rows"])


@pytest.mark.parametrize("case", wcc.CASES, ids=repr)
def test_case_does_what_it_is_meant_to(case):
    exp = wcc.expected(case)
    got = [x["row"] for x in exp["rows"]]
    assert got == sorted(got) and exp["n_unsat"] == len(got)
    if case.want_rows is None:
        assert got, "the case no longer fails anywhere"
    else:
        assert got == case.want_rows
    assert all(x["a"] * x["b"] % P != (x["c"] + x["i"]) % P for x in exp["rows"])
    assert all(r < case.inst.n_rows for r in got)  # padding rows are satisfied


def test_cases_cover_the_edges():
    by = wcc.BY_NAME
    sp = by["sparse12-ok"].inst
    assert sp.num_constraints == 4096 and sp.n_rows % 256 != 0 and by["dense8-ok"].inst.num_constraints == 256
    assert by["sparse12-edge-rows"].want_rows == [0, 63, 64, 255, 256, sp.n_rows - 1]
    lo, hi = wcc.DENSE_RANGE
    assert lo % 256 == 0 and hi % 256 == 0 and hi - lo >= 512 and by["sparse12-dense-failure"].want_rows == list(range(lo, hi))
    one = wcc.expected(by["sparse12-one-wire"])
    assert (2000, ) == tuple(w for w, _ in one["wires"])[:1] and one["n_unsat"] > 1  # the changed wire is suspect; it feeds later rows
    p3 = by["dense8-p-and-p3"]
    assert p3.w_raw[2] == P and p3.w_raw[77] == P + 3 and 1 <= 2 <= p3.n_public
    assert wcc.expected(p3)["n_noncanonical"] == 2 and wcc.expected(p3)["first_noncanonical"] == 2
    lifted = wcc.expected(by["sparse12-lifted"])
    assert (lifted["n_unsat"], lifted["n_noncanonical"], lifted["first_noncanonical"]) == (0, 3, 1)
    assert not wcc.expected(by["dense8-zero-constant"])["constant_wire_is_one"]
