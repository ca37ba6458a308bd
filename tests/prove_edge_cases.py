"""Hand-built circuits at the edges of Proof::prove, each with what the ORACLE (oracle/pyref.py) must say about it.  Nothing here touches
a device; of the product only gnark_r1cs is used, to hold a case's rows as the R1CSInstance the prover takes.

A case is (rows, coeffs, n_public, n_wires, public, private, trapdoor) plus its expectations:
  verifies          the value of pyref.verify_dl on the oracle's own proof
  commit_neutral    dl_commit_p == 0 (commit_p is the neutral element)
  kzg_neutral       dl_kzg == 0
  gm_zeros          how many of the n_wires g_m scalars are 0 (SRS bases at infinity: wires that no row reads)
  i2_is_i_on_d2     i2 == [i(x) for x in D']: true up to n_public == m, false beyond, where the extend of m evaluations gives the
                    interpolant of degree < m (src/proving.rs:369-376, 415) and the reference's own verifier rejects the proof

Rows are (A, B, C) lists of (wire, coeff_id); a row is satisfied when (A w)(B w) = C w: the public-input polynomial enters through the
Vandermonde terms the setup adds to C (pyref.r1cs_with_vandermonde), so the public wires need not be read by any row."""
import dataclasses
import functools
import importlib
import random

import pyref as o

P = o.P


@dataclasses.dataclass
class Case:
    name: str
    rows: list
    coeffs: list
    n_public: int
    n_wires: int
    public: list
    private: list
    trapdoor: tuple
    verifies: bool = True
    commit_neutral: bool = False
    kzg_neutral: bool = False
    gm_zeros: int = 0
    i2_is_i_on_d2: bool = True

    @property
    def m(self):
        m = 2  # the smallest prover has two rows
        while m < len(self.rows):
            m *= 2
        return m

    @property
    def log_m(self):
        return self.m.bit_length() - 1

    @property
    def witness(self):
        return [1] + list(self.public) + list(self.private)

    def inst(self):
        g = importlib.import_module("dv-pari_amd").gnark_r1cs
        inst = g.R1CSInstance.from_rows(self.rows, self.coeffs, self.n_public, self.n_wires)
        assert inst.num_constraints == self.m and inst.n_wires == self.n_wires == len(self.witness)
        return inst

    def __repr__(self):
        return self.name


def _trapdoor(name):
    rnd = random.Random("trapdoor " + name)
    return tuple(rnd.randrange(1, P) for _ in range(3))


def chain(name, n_rows, n_public, **expect):
    """rows (1 + pub_(r mod n_public) + x_r) * x_r = x_(r+1) over the coefficient table [1] ((1 + x_r) * x_r = x_(r+1) without public
    inputs): wires [1 | public | x_0 .. x_n_rows], the constant and every private wire read, the public ones as far as the rows reach"""
    rnd = random.Random("chain " + name)
    pub = [rnd.randrange(P) for _ in range(n_public)]
    x = [rnd.randrange(1, P)]
    rows = []
    for r in range(n_rows):
        xr = 1 + n_public + r
        a = [(0, 0), (xr, 0)]
        av = (1 + x[r]) % P
        if n_public:
            a.insert(1, (1 + r % n_public, 0))
            av = (av + pub[r % n_public]) % P
        rows.append((a, [(xr, 0)], [(xr + 1, 0)]))
        x.append(av * x[r] % P)
    return Case(name, rows, [1], n_public, 1 + n_public + n_rows + 1, pub, x, _trapdoor(name), **expect)


def _build():
    cases = []
    # wires 0 = 1, 1 = x, 2 = y, 3 = z:  x x = y,  y 1 = z
    cases.append(Case("m2", [([(1, 0)], [(1, 0)], [(2, 0)]), ([(2, 0)], [(0, 0)], [(3, 0)])], [1], 0, 4, [], [3, 9, 9], _trapdoor("m2")))
    # wires 0 = 1, 1 = out (public), 2 = x, 3 = y, 4 = z:  x x = y,  y x = z,  (z + x) 1 = out;  the fourth row is padding
    cases.append(Case("m4-padded", [([(2, 0)], [(2, 0)], [(3, 0)]), ([(3, 0)], [(2, 0)], [(4, 0)]), ([(4, 0), (2, 0)], [(0, 0)], [(1, 0)])],
                      [1], 1, 5, [30], [3, 9, 27], _trapdoor("m4-padded")))
    cases.append(chain("pub-eq-m-2", 2, 2))
    cases.append(chain("pub-eq-m-4", 4, 4))
    beyond = dict(verifies=False, i2_is_i_on_d2=False)
    cases.append(chain("pub-gt-m-2", 2, 3, **beyond))
    cases.append(chain("pub-gt-m-4", 4, 5, **beyond))
    cases.append(chain("pub-gt-m-32", 32, 33, **beyond))
    cases.append(chain("pub-48", 64, 48))
    cases.append(chain("pub-49", 64, 49))
    # wire 0 is read by no row and every other wire is 0: w = [1, 0, 0, 0] meets g_m = [0, ..], every evaluation vector is 0
    cases.append(Case("all-neutral", [([(1, 0)], [(1, 0)], [(2, 0)]), ([(2, 0)], [(1, 0)], [(3, 0)])], [1], 0, 4, [], [0, 0, 0],
                      _trapdoor("all-neutral"), commit_neutral=True, kzg_neutral=True, gm_zeros=1))
    # every row 1 * 1 = 1 on the constant wire alone: a = b = 1 on D, so a0 = b0 = 1 and every K scalar is 0
    one = ([(0, 0)], [(0, 0)], [(0, 0)])
    cases.append(Case("const-rows-2", [one] * 2, [1], 0, 1, [], [], _trapdoor("const-rows-2"), kzg_neutral=True))
    cases.append(Case("const-rows-4", [one] * 4, [1], 0, 1, [], [], _trapdoor("const-rows-4"), kzg_neutral=True))
    # wires 0 = 1, 1 = x, 2 = y, 3 = UNUSED, 4 = z, 5 = t, 6 = u, 7 = UNUSED (beyond the last wire any row reads)
    cases.append(Case("unused-wires", [([(1, 0)], [(1, 0)], [(2, 0)]), ([(2, 0)], [(1, 0)], [(4, 0)]), ([(4, 0)], [(0, 0)], [(5, 0)]),
                                       ([(5, 0)], [(5, 0)], [(6, 0)])],
                      [1], 0, 8, [], [3, 9, 0x1234567, 27, 27, 729, P - 2], _trapdoor("unused-wires"), gm_zeros=2))
    # coefficient table with 0, 1, p - 1 and a repeated value; wires 0 = 1, 1 = pub, 2 = x, 3 = y, 4 = z, 5 = t, 6 = u
    #   row 0  (x + 5 x) 1 = y          the same wire twice in one row
    #   row 1  (y + 0 z) (-x) = t       a term with coefficient 0: z is read by that term alone, so its base is at infinity
    #   row 2  () (5 t) = ()            an empty A and an empty C: a = 0 = c
    #   row 3  (-t + 1) pub = 5 u + 5 u
    x, pub, z = 7, 11, 0xabcdef
    y = 6 * x % P
    t = (-x * y) % P
    u = (1 - t) * pub % P * pow(10, P - 2, P) % P
    cases.append(Case("coeff-edges", [([(2, 1), (2, 3)], [(0, 1)], [(3, 1)]), ([(3, 1), (4, 0)], [(2, 2)], [(5, 1)]), ([], [(5, 4)], []),
                                      ([(5, 2), (0, 1)], [(1, 1)], [(6, 3), (6, 4)])],
                      [0, 1, P - 1, 5, 5], 1, 7, [pub], [x, y, z, t, u], _trapdoor("coeff-edges"), gm_zeros=1))
    # wires 0 = 1, 1 = x = p - 1, 2 = y = 1, 3 = z = 0:  x x = y  ((p - 1)^2 = 1),  (x + y) x = z  (the sum wraps to 0); no row reads
    # the constant wire, so its base is at infinity under the scalar 1
    cases.append(Case("wrap", [([(1, 0)], [(1, 0)], [(2, 0)]), ([(1, 0), (2, 0)], [(1, 0)], [(3, 0)])], [1], 0, 4, [], [P - 1, 1, 0],
                      _trapdoor("wrap"), gm_zeros=1))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def alpha_of(case):
    """the Fiat-Shamir challenge as the reference forms it: the transcript over commit_p's 30 bytes (C oracle) and the public inputs"""
    import c_oracle as co

    return lambda dl: o.transcript_challenge(co.xsk233_encode(co.k233_mulgen(dl)), case.public)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = BY_NAME[name]
    tree = o.FFTree(c.log_m + 1)
    st = o.setup_srs_scalars(tree, c.rows, c.coeffs, c.n_public, c.trapdoor)
    return tree, st, o.prove_scalars(tree, st, c.public, c.private, alpha_of(c))


def oracle(case):
    """(tree, setup, proof scalars) of the case from pyref, computed once and shared: treat it as read-only"""
    return _oracle(case.name)


def gm_padded(case, st):
    """g_m over all n_wires wires: pyref stops at the last wire a row reads"""
    return st["g_m"] + [0] * (case.n_wires - len(st["g_m"]))
