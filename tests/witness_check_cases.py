"""Cases of the witness check (dvp_prover_check_witness*) and its restatement in plain Python: pyref.eval_row over every row, Horner for
i(d_row), integer counters for the suspect rule.  Nothing here touches a device; the domain D comes from the oracle's own tree.

A case is (instance, raw witness [1, public.., private..] of any integers below 2^256, what it is meant to do); expected(case) is the
report the check must give: every failing row as {row, a, b, c, i}, the entries that are not below p, the suspect wires."""
import dataclasses
import functools
import importlib

import pyref as o

P = o.P
EDGE_ROWS = (0, 63, 64, 255, 256)  # lane, wave and workgroup edges; the last real row joins them per instance
DENSE_RANGE = (256, 1024)          # every row of workgroups 1, 2 and 3


def domain(log_m):
    """D of a prover with 2^log_m constraints: the even leaves of the oracle's tree with 2^(log_m + 1) leaves"""
    return _domain(log_m)


@functools.lru_cache(maxsize=None)
def _domain(log_m):
    return tuple(o.FFTree(log_m + 1).both_domains()[0])


def rows_of(inst):
    """an R1CSInstance's real rows as (A_r, B_r, C_r) lists of (wire, coeff_id), and its coefficient table as ints"""
    def side(m, r):
        lo, hi = int(m.row_ptr[r]), int(m.row_ptr[r + 1])
        return list(zip(m.wire[lo:hi].tolist(), m.coeff[lo:hi].tolist()))

    coeffs = [int.from_bytes(inst.coeffs[k].tobytes(), "little") for k in range(inst.coeffs.shape[0])]
    return [(side(inst.l, r), side(inst.r, r), side(inst.o, r)) for r in range(inst.n_rows)], coeffs


def restate(rows, coeffs, n_public, m, w_raw, dom):
    """the report, unabridged: rows = every failing row in row order, wires = every suspect wire in wire order"""
    w = [x % P for x in w_raw]
    big = [k for k, x in enumerate(w_raw) if x >= P]
    failing, good, in_bad = [], set(), {}
    for r in range(m):  # padding rows have no terms: a = b = C w = 0, satisfied
        sides = rows[r] if r < len(rows) else ([], [], [])
        a, b, cw = (o.eval_row(s, coeffs, w) for s in sides)
        fails = a * b % P != cw
        if fails:
            iv = 0
            for j in range(n_public - 1, -1, -1):  # Horner: i = sum_j pub_j d^j
                iv = (iv * dom[r] + w[1 + j]) % P
            failing.append({"row": r, "a": a, "b": b, "c": (cw - iv) % P, "i": iv})
        for s in sides:
            for wire, _ in s:
                if fails:
                    in_bad[wire] = in_bad.get(wire, 0) + 1
                else:
                    good.add(wire)
    wires = sorted((wire, n) for wire, n in in_bad.items() if wire not in good)
    return {"n_unsat": len(failing), "first_unsat": failing[0]["row"] if failing else -1, "n_noncanonical": len(big),
            "first_noncanonical": big[0] if big else -1, "n_suspect_wires": len(wires), "constant_wire_is_one": w[0] == 1,
            "rows": failing, "wires": wires}


@dataclasses.dataclass
class Case:
    name: str
    inst: object       # R1CSInstance
    w_raw: list        # [1, public.., private..], any integers below 2^256
    want_rows: object  # the exact failing set the case is meant to produce (a sorted list), or None: non-empty is all that is asked

    @property
    def log_m(self):
        return self.inst.num_constraints.bit_length() - 1

    @property
    def n_public(self):
        return self.inst.num_public_inputs

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = BY_NAME[name]
    rows, coeffs = rows_of(c.inst)
    return restate(rows, coeffs, c.n_public, c.inst.num_constraints, c.w_raw, domain(c.log_m))


def expected(case):
    """computed once per case and shared: treat it as read-only"""
    return _expected(case.name)


def with_c_coeff(inst, rows, coeff_id):
    """the instance with the coefficient id of C's FIRST term changed in the given rows: what editing those terms in the dump gives"""
    coeff = inst.o.coeff.copy()
    for r in rows:
        assert inst.o.row_ptr[r + 1] > inst.o.row_ptr[r]
        coeff[int(inst.o.row_ptr[r])] = coeff_id
    return dataclasses.replace(inst, o=dataclasses.replace(inst.o, coeff=coeff))


def _build():
    g = importlib.import_module("dv-pari_amd").gnark_r1cs
    dense, d_pub, d_prv = g.synthetic_dense(8)
    sparse, s_pub, s_prv = g.synthetic_sparse(12)
    dw, sw = [1] + list(d_pub) + list(d_prv), [1] + list(s_pub) + list(s_prv)
    assert len(dw) == dense.n_wires and len(sw) == sparse.n_wires and sparse.n_rows < sparse.num_constraints == 4096
    cases = [Case("dense8-ok", dense, dw, []), Case("sparse12-ok", sparse, sw, [])]
    # one private wire changed: an output wire in the middle of the circuit, read by later rows
    bad = list(sw)
    bad[2000] = (bad[2000] + 1) % P
    cases.append(Case("sparse12-one-wire", sparse, bad, None))
    bad = list(dw)
    bad[100] = (bad[100] + 1) % P
    cases.append(Case("dense8-one-wire", dense, bad, None))
    # C's term edited in chosen rows (coefficient 1 -> coefficient id 1, another value): exactly these rows fail
    edges = sorted(EDGE_ROWS + (sparse.n_rows - 1,))
    cases.append(Case("sparse12-edge-rows", with_c_coeff(sparse, edges, 1), sw, edges))
    whole = list(range(*DENSE_RANGE))
    cases.append(Case("sparse12-dense-failure", with_c_coeff(sparse, whole, 1), sw, whole))
    # entries that are not below p.  The literal values p and p + 3 (they reduce to 0 and 3, so rows fail), one of them a public wire
    bad = list(dw)
    bad[2], bad[77] = P, P + 3
    cases.append(Case("dense8-p-and-p3", dense, bad, None))
    # other representatives of the SAME witness: nothing fails, three entries are counted
    lifted = list(sw)
    for k, mult in ((1, 1), (300, 3), (sparse.n_wires - 1, 2**24 - 1)):
        lifted[k] += mult * P
    cases.append(Case("sparse12-lifted", sparse, lifted, []))
    # the constant wire zeroed (only the be32 and device flavours can present it)
    bad = list(dw)
    bad[0] = 0
    cases.append(Case("dense8-zero-constant", dense, bad, None))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
