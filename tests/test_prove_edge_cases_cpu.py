"""The cases of prove_edge_cases.py against the oracle ALONE (no GPU): each case states what pyref's setup and proof must show -- the
verdict of verify_dl, which commitments are neutral, how many g_m scalars are 0, whether i2 is i(X) on D' -- and the GPU tests
(test_gpu_prove_edges.py) then hold the library to the same oracle values.  A case the oracle cannot run is a wrong case."""
import pytest

import pyref as o
import prove_edge_cases as ec

P = o.P


def test_the_case_list_is_the_one_the_gpu_tests_rely_on():
    names = [c.name for c in ec.CASES]
    assert names == ["m2", "m4-padded", "pub-eq-m-2", "pub-eq-m-4", "pub-gt-m-2", "pub-gt-m-4", "pub-gt-m-32", "pub-48", "pub-49",
                     "all-neutral", "const-rows-2", "const-rows-4", "unused-wires", "coeff-edges", "wrap"]
    shape = {c.name: (c.m, len(c.rows), c.n_public) for c in ec.CASES}
    assert shape["m2"] == (2, 2, 0) and shape["m4-padded"] == (4, 3, 1)
    assert shape["pub-eq-m-2"] == (2, 2, 2) and shape["pub-eq-m-4"] == (4, 4, 4)
    assert shape["pub-gt-m-2"] == (2, 2, 3) and shape["pub-gt-m-4"] == (4, 4, 5) and shape["pub-gt-m-32"] == (32, 32, 33)
    assert shape["pub-48"] == (64, 64, 48) and shape["pub-49"] == (64, 64, 49)
    assert shape["all-neutral"] == (2, 2, 0) and shape["const-rows-2"] == (2, 2, 0) and shape["const-rows-4"] == (4, 4, 0)
    assert shape["unused-wires"][0] == 4 and shape["coeff-edges"][0] == 4 and shape["wrap"][0] == 2


@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_case_is_well_formed(case):
    w = case.witness
    assert len(w) == case.n_wires >= 1 + case.n_public and all(0 <= x < P for x in w)
    assert all(0 <= x < P for x in case.coeffs) and all(0 < x < P for x in case.trapdoor)
    for row in case.rows:
        a, b, c = (o.eval_row(s, case.coeffs, w) for s in row)
        assert a * b % P == c
        assert all(wire < case.n_wires and cid < len(case.coeffs) for s in row for wire, cid in s)
    inst = case.inst()
    assert (inst.n_rows, inst.num_public_inputs) == (len(case.rows), case.n_public)


@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_oracle_meets_the_stated_expectations(case):
    tree, st, pr = ec.oracle(case)
    d, d2 = st["tables"]["D"], st["tables"]["D2"]
    assert case.trapdoor[0] not in d and case.trapdoor[0] not in d2
    ok = o.verify_dl(case.trapdoor, case.public, pr["dl_commit_p"], pr["dl_kzg"], pr["a0"], pr["b0"], pr["alpha"])
    assert ok == case.verifies
    assert (pr["dl_commit_p"] == 0) == case.commit_neutral
    assert (pr["dl_kzg"] == 0) == case.kzg_neutral
    assert sum(1 for x in ec.gm_padded(case, st) if x == 0) == case.gm_zeros
    assert (pr["i2"] == [o.evaluate_monomial_basis_poly(case.public, x) for x in d2]) == case.i2_is_i_on_d2
    assert case.i2_is_i_on_d2 == (case.n_public <= case.m)
    # the interpolant the extend gives is the polynomial of degree < m through i on D, whatever n_public is
    assert pr["i2"] == [o.lagrange_eval(d, pr["i"], x) for x in d2]


def test_what_each_named_case_is_for():
    pr = {c.name: ec.oracle(c)[2] for c in ec.CASES}
    st = {c.name: ec.oracle(c)[1] for c in ec.CASES}
    z = pr["all-neutral"]
    assert (z["a0"], z["b0"], z["dl_commit_p"], z["dl_kzg"]) == (0, 0, 0, 0) and st["all-neutral"]["g_m"][0] == 0
    for n in ("const-rows-2", "const-rows-4"):
        assert (pr[n]["a0"], pr[n]["b0"]) == (1, 1) and pr[n]["dl_commit_p"] != 0 and not any(pr[n]["s_k"])
    u = ec.BY_NAME["unused-wires"]
    gm = ec.gm_padded(u, st["unused-wires"])
    assert [k for k, x in enumerate(gm) if x == 0] == [3, 7] and u.witness[3] and u.witness[7]
    e = ec.BY_NAME["coeff-edges"]
    assert {0, 1, P - 1} <= set(e.coeffs) and len(set(e.coeffs)) < len(e.coeffs)
    assert pr["coeff-edges"]["a"][2] == 0 and pr["coeff-edges"]["c"][2] == (-pr["coeff-edges"]["i"][2]) % P
    assert [k for k, x in enumerate(ec.gm_padded(e, st["coeff-edges"])) if x == 0] == [4] and e.witness[4]
    w = pr["wrap"]
    assert w["a"][0] == w["b"][0] == P - 1 and (w["c"][0], w["a"][1]) == (1, 0) and {0, 1, P - 1} <= set(ec.BY_NAME["wrap"].witness)
