"""The Fr vector entries of the C ABI (dvp_fr_vec_mul / _scale / _axpy / _scalar_sub / _dot, dvp_fr_spmv, dvp_fr_batch_inverse,
dvp_barycentric_eval: what srs.py and gnark_r1cs.py build the SRS and the witness with) against Python integers, at the lengths
where their kernels change shape -- empty, one element, one workgroup of 256 and one element either side of it, the stride loop of
the capped dot-product grid, one thread's 16 elements and one workgroup's 4096 of the barycentric sum -- with elements and scalars
drawn from the carry-boundary values of fr_cases.py as well as at random.  Integer equality only."""
import random

import numpy as np
import pytest

import fr_cases as fc
import pyref as o
from util import from_limbs, np_dot_mod_fast, rand_fr_np, to_limbs

pytestmark = pytest.mark.gpu
P = fc.P
LENGTHS = (0, 1, 255, 256, 257, 1000)
SCALARS = (0, 1, 2, P - 1, (P + 1) // 2, fc.R % P, (1 << 231) - 1, 0x1234567 * 7919)


def mixed(n, seed, nonzero=False):
    """n canonical values: edge values and uniform ones in turn"""
    rnd = random.Random(seed)
    e = fc.edge_values()
    out = [e[rnd.randrange(len(e))] if rnd.random() < 0.5 else rnd.randrange(P) for _ in range(n)]
    return [x or 1 for x in out] if nonzero else out


@pytest.mark.parametrize("n", LENGTHS)
def test_pointwise_ops(dvp, n):
    a, b = mixed(n, 100 + n), mixed(n, 200 + n)
    va, vb = dvp.fr.vec(a), dvp.fr.vec(b)
    assert dvp.fr.to_ints(dvp.fr.mul(va, vb)) == [x * y % P for x, y in zip(a, b)]
    for s in SCALARS + tuple(mixed(4, 300 + n)):
        assert dvp.fr.to_ints(dvp.fr.scale(va, s)) == [s * x % P for x in a], hex(s)
        assert dvp.fr.to_ints(dvp.fr.axpy(va, s, vb)) == [(x + s * y) % P for x, y in zip(a, b)], hex(s)
        assert dvp.fr.to_ints(dvp.fr.scalar_sub(s, va)) == [(s - x) % P for x in a], hex(s)
    assert dvp.fr.dot(va, vb) == sum(x * y for x, y in zip(a, b)) % P


def test_pointwise_ops_reject_noncanonical_scalar(dvp, nat):
    va = dvp.fr.vec([1, 2, 3])
    out = np.zeros_like(va)
    s = to_limbs([P])
    assert dvp.lib.dvp_fr_vec_scale(nat.ptr(va), nat.ptr(s), 3, nat.ptr(out)) == -1
    assert dvp.lib.dvp_fr_vec_axpy(nat.ptr(va), nat.ptr(s), nat.ptr(va), 3, nat.ptr(out)) == -1
    assert dvp.lib.dvp_fr_vec_scalar_sub(nat.ptr(s), nat.ptr(va), 3, nat.ptr(out)) == -1


def test_dot_stride_loop(dvp):
    """2^18 + 257 elements: the grid is capped at 1024 workgroups of 256, so 257 threads take a second element.  Extremes ride at
    both ends of the vector and around the wrap."""
    n = (1 << 18) + 257
    a, b = rand_fr_np(n, 41), rand_fr_np(n, 42)
    spots = [0, 1, 255, 256, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 18) + 255, n - 2, n - 1]
    a[spots] = to_limbs([P - 1] * len(spots))
    b[spots] = to_limbs(mixed(len(spots), 43, nonzero=True))
    assert dvp.fr.dot(a, b) == np_dot_mod_fast(a, b)
    # a single non-zero product in the part only the second trip of the loop reaches
    z = np.zeros((n, 4), dtype=np.uint64)
    for i in ((1 << 18), (1 << 18) + 256, n - 1):
        z[:] = 0
        z[i] = to_limbs([P - 2])[0]
        assert dvp.fr.dot(z, z) == 4, i


@pytest.mark.parametrize("n", LENGTHS + (4097,))
def test_batch_inverse(dvp, n):
    vals = mixed(n, 500 + n)
    for i in (0, 7, 255, 256, n - 1):
        if 0 <= i < n and n > 1:
            vals[i] = 0
    got = dvp.fr.to_ints(dvp.fr.batch_inverse(dvp.fr.vec(vals)))
    assert got == [pow(x, -1, P) if x else 0 for x in vals]


def test_batch_inverse_every_edge_value(dvp):
    e = list(fc.edge_values())
    assert dvp.fr.to_ints(dvp.fr.batch_inverse(dvp.fr.vec(e))) == [pow(x, -1, P) if x else 0 for x in e]


def _spmv_case(dvp, rows, n_cols, n_coeffs, seed):
    """rows: list of lists of (col, coeff id)"""
    coeffs, x = mixed(n_coeffs, seed), mixed(n_cols, seed + 1)
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    col = np.array([c for r in rows for c, _ in r], dtype=np.uint32)
    cid = np.array([k for r in rows for _, k in r], dtype=np.uint32)
    got = dvp.fr.to_ints(dvp.fr.spmv(row_ptr, col, cid, dvp.fr.vec(coeffs), dvp.fr.vec(x)))
    assert got == [sum(coeffs[k] * x[c] for c, k in r) % P for r in rows]


def test_spmv(dvp):
    rnd = random.Random(77)
    n_cols, n_coeffs = 301, 17
    ent = lambda: (rnd.randrange(n_cols), rnd.randrange(n_coeffs))
    rows = [[ent() for _ in range(rnd.randrange(6))] for _ in range(257)]
    rows[0], rows[1], rows[2] = [], [ent()], [(c, c % n_coeffs) for c in range(300)]  # empty, one entry, 300 entries
    rows[3] = [(5, 1)] * 9 + [(5, 2), (6, 1)]  # repeated columns
    rows[255], rows[256] = [], [ent(), ent()]  # the last row of workgroup 0 and the lone row of workgroup 1
    _spmv_case(dvp, rows, n_cols, n_coeffs, 600)
    _spmv_case(dvp, [[(0, 0), (2, 1), (0, 0)]], 3, 2, 610)  # one row
    _spmv_case(dvp, [[(c % 3, 0) for c in range(300)]], 3, 1, 620)
    _spmv_case(dvp, [[] for _ in range(5)], 3, 2, 630)  # no entry at all
    _spmv_case(dvp, [[]], 1, 1, 640)
    assert dvp.fr.spmv(np.zeros(1, dtype=np.uint32), [], [], dvp.fr.vec([1]), dvp.fr.vec([1])).shape == (0, 4)  # no row


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097])
def test_barycentric_eval(dvp, nat, n):
    """one thread owns 16 elements and one workgroup 4096: a length either side of both.  The entry computes
    z * sum_i y_i w_i / (alpha - s_i) for whatever tables it is given, so a random distinct domain with random weights exercises it
    exactly as a real one does"""
    rnd = random.Random(900 + n)
    e = fc.edge_values()
    alphas = (P - 1, (1 << 231) + 1, rnd.randrange(P))  # kept out of the domain: alpha - s_i must be invertible
    dom = set()
    while len(dom) < n:
        dom.add(e[rnd.randrange(len(e))] if len(dom) < min(n // 2, 600) else rnd.randrange(P))
        dom -= set(alphas)
    dom = list(dom)
    rnd.shuffle(dom)
    wts, ev = mixed(n, 910 + n), mixed(n, 920 + n)
    assert len(dom) == n and not set(dom) & set(alphas)
    for alpha, z in zip(alphas, (P - 1, rnd.randrange(P), 1)):
        out = np.zeros(4, dtype=np.uint64)
        dvp.check(dvp.lib.dvp_barycentric_eval(nat.ptr(to_limbs(dom)), nat.ptr(to_limbs(wts)), nat.ptr(to_limbs([z])),
                                               nat.ptr(to_limbs(ev)), n, nat.ptr(to_limbs([alpha])), nat.ptr(out)))
        assert from_limbs(out[None])[0] == o.barycentric_eval(dom, wts, z, ev, alpha), hex(alpha)
