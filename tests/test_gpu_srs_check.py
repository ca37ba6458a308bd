"""GPU tests (-m gpu) of dvp_srs_check_cache_dir: the audit of the five SRS vectors of a cache_dir against a trapdoor, on the
instances test_gpu_cache_dir.py::test_setup_cache_dir_entry_scalars sets up (toy, sparse7, sparse12 -- the last two with two public
inputs, so the Vandermonde fold is in g_m).  What a foreign trapdoor or public-input count must flag is predicted from the discrete
logs dvp_setup_cache_dir_ex reports under both settings: exactly the vectors whose scalars differ, at the first index they differ."""
import os
import random
import shutil
import struct

import numpy as np
import pytest

import pyref as o
from util import from_limbs

pytestmark = pytest.mark.gpu
SHAPES = ["toy", "sparse7", "sparse12"]
EINVAL = -1


class Case:
    pass


def py_dump(rows, coeffs):
    """rows of (L, R, O) term lists in the gnark dump format (src/gnark_r1cs.rs:84-91,121-185)"""
    out = [struct.pack("<I", len(coeffs))] + [int(c).to_bytes(32, "big") for c in coeffs] + [struct.pack("<I", len(rows))]
    for l, r, oo in rows:
        out.append(struct.pack("<III", len(l), len(r), len(oo)))
        for part in (l, r, oo):
            for w, k in part:
                out.append(struct.pack("<II", w, k))
    return b"".join(out)


@pytest.fixture(scope="module")
def cases(dvp, tmp_path_factory):
    """shape -> the directory after dvp_setup_cache_dir, its trapdoor, its scalars; set up once, never written to again"""
    made = {}

    def get(shape):
        if shape in made:
            return made[shape]
        A, g = dvp.artifacts, dvp.gnark_r1cs
        c = Case()
        c.dir = tmp_path_factory.mktemp(shape)
        if shape == "toy":
            (c.dir / A.R1CS_CONSTRAINTS_FILE).write_bytes(py_dump(g.TOY_ROWS, g.TOY_COEFFS))
            c.pub, c.prv = g.TOY_PUBLIC, g.TOY_PRIVATE
        else:
            inst0, c.pub, c.prv = g.synthetic_sparse(int(shape[6:]))
            inst0.write_dump_file(c.dir / A.R1CS_CONSTRAINTS_FILE)
        c.n_pub = len(c.pub)
        rnd = random.Random(len(shape))
        c.trap = (rnd.randrange(1, o.P - 1), rnd.randrange(1, o.P - 1), rnd.randrange(1, o.P - 1))
        c.td = dvp.srs.Trapdoor(*c.trap)
        c.inst, pv, c.scalars = dvp.srs.verifier_runs_setup_cache_dir(c.td, c.dir, c.n_pub, write_precomputes=False, return_scalars=True)
        pv.close()
        c.counts = [c.inst.n_wires] + [c.inst.num_constraints] * 3 + [2 * c.inst.num_constraints]
        made[shape] = c
        return c

    return get


def flat(scalars):
    g_m, g_q, g_k = scalars
    return [g_m, g_q, g_k[0], g_k[1], g_k[2]]


def scalars_under(dvp, c, tmp_path, td, n_pub):
    """the discrete logs dvp_setup_cache_dir_ex reports for c's dump under another trapdoor / public-input count"""
    d = tmp_path / f"other{len(os.listdir(tmp_path))}"
    d.mkdir()
    shutil.copy(c.dir / dvp.artifacts.R1CS_CONSTRAINTS_FILE, d)
    _, pv, sc = dvp.srs.verifier_runs_setup_cache_dir(td, d, n_pub, write_precomputes=False, return_scalars=True)
    pv.close()
    return flat(sc)


def predicted(mine, theirs):
    """per vector: the first index at which two scalar vectors differ, or None"""
    out = []
    for a, b in zip(mine, theirs):
        diff = np.nonzero((a != b).any(axis=1))[0]
        out.append(int(diff[0]) if diff.size else None)
    return out


def assert_report(dvp, rep, c, first, exact=False, status=None):
    """first[v] = None for a clean vector, else its first offending index; status[v] overrides SRS_VEC_WRONG"""
    S, C = dvp.srs, dvp.curve
    bad = 0
    for v, vec in enumerate(rep.vectors):
        want = 0 if first[v] is None else (status or {}).get(v, S.SRS_VEC_WRONG)
        assert (vec.name, vec.status, vec.first_bad, vec.count) == (S.SRS_VECTORS[v], want, first[v] if first[v] != -1 else None, c.counts[v]), (v, vec)
        if want in (0, S.SRS_VEC_WRONG):
            assert vec.path == (C.DLOG_PATH_EXACT if exact else C.DLOG_PATH_LOCATED if want else C.DLOG_PATH_COMBINED), (v, vec)
        else:
            assert vec.path == 0, (v, vec)
        bad |= (want != 0) << v
    assert rep.bad_vectors == bad and rep.verdict == (1 if bad else 0) and rep.ok == (not bad)


CLEAN = [None] * 5


@pytest.mark.parametrize("shape", SHAPES)
def test_the_setups_own_directory_is_clean(dvp, cases, shape):
    c = cases(shape)
    before = {n: (c.dir / n).read_bytes() for n in os.listdir(c.dir)}
    for seed, exact in ((None, False), (bytes(range(32)), False), (None, True)):
        assert_report(dvp, dvp.srs.check_cache_dir(c.td, c.dir, c.n_pub, seed=seed, exact=exact), c, CLEAN, exact)
    assert {n: (c.dir / n).read_bytes() for n in os.listdir(c.dir)} == before  # nothing written, nothing added


@pytest.mark.parametrize("which", ["tau", "delta", "epsilon"])
@pytest.mark.parametrize("shape", SHAPES)
def test_a_foreign_trapdoor_flags_what_its_scalars_change(dvp, cases, tmp_path, shape, which):
    c = cases(shape)
    k = ["tau", "delta", "epsilon"].index(which)
    trap = tuple(x + 1 if j == k else x for j, x in enumerate(c.trap))
    td = dvp.srs.Trapdoor(*trap)
    first = predicted(flat(c.scalars), scalars_under(dvp, c, tmp_path, td, c.n_pub))
    changed = {"tau": [0, 1, 2, 3, 4], "delta": [0, 1, 3, 4], "epsilon": [0, 1]}[which]  # src/srs.rs:126-160
    assert [v for v in range(5) if first[v] is not None] == changed
    for exact in (False, True):
        assert_report(dvp, dvp.srs.check_cache_dir(td, c.dir, c.n_pub, exact=exact), c, first, exact)


@pytest.mark.parametrize("shape", SHAPES)
def test_another_public_input_count_flags_g_m_only(dvp, cases, tmp_path, shape):
    c = cases(shape)
    n_pub = c.n_pub - 1
    first = predicted(flat(c.scalars), scalars_under(dvp, c, tmp_path, c.td, n_pub))
    assert first[0] == 1 + n_pub and first[1:] == [None] * 4  # the wire whose Vandermonde column is no longer folded in
    for exact in (False, True):
        assert_report(dvp, dvp.srs.check_cache_dir(c.td, c.dir, n_pub, exact=exact), c, first, exact)


def damaged(c, tmp_path):
    d = tmp_path / "damaged"
    shutil.copytree(c.dir, d)
    return d


@pytest.mark.parametrize("shape", SHAPES)
def test_damaged_files(dvp, cases, tmp_path, shape):
    A, io, S = dvp.artifacts, dvp.io_utils, dvp.srs
    c = cases(shape)
    d = damaged(c, tmp_path)
    m = c.inst.num_constraints
    # one entry of g_k_2 is another scalar's multiple
    enc = io.read_point_vec_payload(d / A.SRS_G_K_2)
    good_k2 = enc.copy()
    at = 2 * m - 3
    enc[at] = dvp.curve.point_scalar_mul_gen_batch_bytes(dvp.fr.vec([12345]))[0]
    io.write_point_vec_to_file(d / A.SRS_G_K_2, enc)
    for exact in (False, True):
        assert_report(dvp, S.check_cache_dir(c.td, d, c.n_pub, exact=exact), c, [None, None, None, None, at], exact)
    io.write_point_vec_to_file(d / A.SRS_G_K_2, good_k2)
    # g_q one entry short
    gq = io.read_point_vec_payload(d / A.SRS_G_Q)
    io.write_point_vec_to_file(d / A.SRS_G_Q, gq[:-1])
    # an encoding the decoder rejects in g_k_0 (under the rule in force: shown first)
    k0 = io.read_point_vec_payload(d / A.SRS_G_K_0)
    k0[5 % m] = 0xFF
    with pytest.raises(dvp.DvpError) as e:
        dvp.curve.from_bytes(k0)
    assert (e.value.status, e.value.index) == (-2, 5 % m)
    io.write_point_vec_to_file(d / A.SRS_G_K_0, k0)
    # g_k_1 is gone
    os.remove(d / A.SRS_G_K_1)
    status = {1: S.SRS_VEC_LENGTH, 2: S.SRS_VEC_DECODE, 3: S.SRS_VEC_MISSING}
    for exact in (False, True):
        assert_report(dvp, S.check_cache_dir(c.td, d, c.n_pub, exact=exact), c, [None, m - 1, 5 % m, -1, None], exact, status)
    # a file that ends before its count says, and one without a count
    raw = (d / A.SRS_G_K_2).read_bytes()
    (d / A.SRS_G_K_2).write_bytes(raw[:-1])
    (d / A.SRS_G_M).write_bytes(b"\x01\x02\x03")
    status.update({0: S.SRS_VEC_LENGTH, 4: S.SRS_VEC_LENGTH})
    assert_report(dvp, S.check_cache_dir(c.td, d, c.n_pub), c, [0, m - 1, 5 % m, -1, 2 * m - 1], False, status)


def test_calls_that_fail(dvp, cases, tmp_path):
    c = cases("toy")
    for k in range(3):
        trap = [0 if j == k else x for j, x in enumerate(c.trap)]
        with pytest.raises(dvp.DvpError) as e:
            dvp.srs.check_cache_dir(dvp.srs.Trapdoor(*trap), c.dir, c.n_pub)
        assert e.value.status == EINVAL
    with pytest.raises(dvp.DvpError) as e:  # not below p
        dvp.srs.check_cache_dir(dvp.srs.Trapdoor(o.P, c.trap[1], c.trap[2]), c.dir, c.n_pub)
    assert e.value.status == EINVAL
    tree = dvp.ec_fft.FFTree(2 * c.inst.num_constraints)
    for dom in tree.get_both_domains():  # tau in D, tau in D'
        with pytest.raises(dvp.DvpError) as e:
            dvp.srs.check_cache_dir(dvp.srs.Trapdoor(from_limbs(dom)[3], c.trap[1], c.trap[2]), c.dir, c.n_pub)
        assert e.value.status == EINVAL
    tree.close()
    with pytest.raises(dvp.DvpError) as e:  # no dump
        dvp.srs.check_cache_dir(c.td, tmp_path, c.n_pub)
    assert e.value.status == -6
    with pytest.raises(dvp.DvpError) as e:  # more public inputs than wires
        dvp.srs.check_cache_dir(c.td, c.dir, 1000)
    assert e.value.status == EINVAL


@pytest.mark.parametrize("shape", ["toy", "sparse12"])
def test_the_directory_still_proves_and_verifies(dvp, cases, shape):
    c = cases(shape)
    assert dvp.srs.check_cache_dir(c.td, c.dir, c.n_pub).ok
    n_wires = struct.unpack("<Q", (c.dir / dvp.artifacts.SRS_G_M).read_bytes()[:8])[0]
    proof = dvp.proving.Proof.prove(c.dir, c.pub, c.prv[: n_wires - 1 - c.n_pub])
    dvp.proving.release_cache_dir(c.dir)
    assert dvp.srs.verify_device(c.td, c.pub, proof)
    assert dvp.srs.check_cache_dir(c.td, c.dir, c.n_pub).ok
