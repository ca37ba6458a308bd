"""GPU tests (-m gpu) of dvp_verify_trace_batch (csrc/simulate.hip: k_verify_trace, srs.verify_trace): for simulated proofs of every
case the record's scalars equal big-int arithmetic and its points equal fixed-base multiples of the known discrete logs; for
tampered proofs of every kind the verdict is dvp_verify_batch's, a validity bit zeroes the record, the EQUATION bit follows the
points; v0 K is checked against the C oracle's variable-base multiplication; the CLI's --trace output parses back to the record."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import c_oracle as co
import pyref as o
import simulate_cases as sc
import verify_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = (0x3D9F1A77 * 104729 % o.P, 0xC0FFEE1234567 % o.P, 0xDEADBEEF987654321 % o.P)
SEED = bytes(range(40, 72))
FIELDS = ("alpha", "i0", "r0", "u0", "v0")
POINTS = ("p", "k", "vk", "ug", "sum")


def simulated(dvp, n, n_public=2, seed=SEED):
    rng = random.Random(n)
    S = dvp.srs
    pubs = [[rng.randrange(o.P) for _ in range(n_public)] for _ in range(n)]
    cases = [(j + n) % 7 for j in range(n)]
    proofs, status, dlogs = S.simulate_batch(S.Trapdoor(*TD), pubs, seed=seed, cases=cases, return_dlogs=True)
    assert not status.any()
    return pubs, cases, proofs, [dvp.fr.to_ints(d) for d in dlogs]


def mulgen(dvp, dlogs):
    """(xy, inf) of dlog G, infinity with zero coordinates as the trace writes it"""
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(dvp.fr.vec(dlogs))
    xy[inf != 0] = 0
    return xy, inf


def assert_points(tr, name, xy, inf, rows=None):
    rows = range(len(tr)) if rows is None else rows
    got_xy, got_inf = tr[name + "_xy"][rows], tr[name + "_inf"][rows]
    assert (got_inf == inf).all(), (name, np.nonzero(got_inf != inf)[0][:10])
    assert (got_xy == xy).all(), (name, np.nonzero((got_xy != xy).any(axis=1))[0][:10])


def is_zero_elsewhere(rec):
    return not any(np.asarray(rec[f]).any() for f in rec.dtype.names if f != "verdict")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_valid_proofs_of_every_case(dvp, n):
    S = dvp.srs
    td = S.Trapdoor(*TD)
    pubs, cases, proofs, dlogs = simulated(dvp, n)
    tr = S.verify_trace(td, pubs, proofs)
    assert tr.shape == (n,) and not tr["verdict"].any() and not tr["pad"].any()
    assert (tr["verdict"] == S.verify_batch(td, pubs, proofs)).all()
    want = {f: [] for f in FIELDS}
    d_vk, d_ug, d_sum = [], [], []
    for j in range(n):
        pb = proofs[j].tobytes()
        alpha = dvp.proving.transcript_challenge(pb[:30], pubs[j])
        i0, r0, u0, v0 = sc.trace_scalars(TD, pubs[j], pb, alpha)
        for f, v in zip(FIELDS, (alpha, i0, r0, u0, v0)):
            want[f].append(v)
        p, k = dlogs[j]
        vk, ug, sm = sc.trace_dlogs(k, u0, v0)
        assert sm == p, (j, cases[j])  # v0 K + u0 G = (p - t) G + t G
        d_vk.append(vk)
        d_ug.append(ug)
        d_sum.append(p)
    for f in FIELDS:
        assert dvp.fr.to_ints(tr[f]) == want[f], f
    for name, lo in (("p", 0), ("k", 30)):
        xy, inf = dvp.curve.from_bytes(proofs[:, lo:lo + 30])
        xy[inf != 0] = 0
        assert_points(tr, name, xy, inf)
    for name, dl in (("vk", d_vk), ("ug", d_ug), ("sum", d_sum)):
        assert_points(tr, name, *mulgen(dvp, dl))
    if n >= 7:  # the cases did reach their flags
        by = {c: j for j, c in enumerate(cases)}
        assert tr["p_inf"][by[sc.P_ZERO]] and tr["sum_inf"][by[sc.P_ZERO]] and not tr["vk_inf"][by[sc.P_ZERO]]
        assert tr["k_inf"][by[sc.K_ZERO]] and tr["vk_inf"][by[sc.K_ZERO]]
        assert tr["ug_inf"][by[sc.U0_ZERO]]
        j = by[sc.T_HALF]
        assert (tr["vk_xy"][j] == tr["ug_xy"][j]).all() and not tr["sum_inf"][j]  # the final addition was a doubling


@pytest.fixture(scope="module")
def tampered(dvp):
    """three tampered proofs of every kind among valid ones, in one batch per trapdoor: rows of (bytes, pub, kind, K's discrete log)"""
    rng = random.Random(99)
    pubs, cases, proofs, dlogs = simulated(dvp, 70, seed=bytes(32))
    base = [dict(proof=proofs[j].tobytes(), td=TD, pub=pubs[j], a0=int.from_bytes(proofs[j, 60:89].tobytes(), "little")) for j in range(70)]
    rows = {TD: [(b["proof"], b["pub"], "valid", dlogs[j][1]) for j, b in enumerate(base)]}
    pos = rng.sample(range(70), 3 * (len(vc.TAMPER) - 1))
    it = iter(pos)
    for kind in vc.TAMPER:
        for r in range(3):
            if kind == "wrong_trapdoor":
                j = 7 * r  # a generic proof: with K = O (K_ZERO) another tau changes nothing
                assert cases[j] == sc.GENERIC
                b, td, pub = vc.tamper(base[j], kind, rng)
                rows.setdefault(td, []).append((b, pub, kind, dlogs[j][1]))
            else:
                j = next(it)
                b, td, pub = vc.tamper(base[j], kind, rng)
                rows[TD][j] = (b, pub, kind, dlogs[j][1])
    return rows


def test_tampered_proofs(dvp, tampered):
    S = dvp.srs
    seen = set()
    for tdv, rows in tampered.items():
        td = S.Trapdoor(*tdv)
        pubs, proofs = [r[1] for r in rows], [r[0] for r in rows]
        tr = S.verify_trace(td, pubs, proofs)
        v = S.verify_batch(td, pubs, proofs)
        assert (tr["verdict"] == v).all(), np.nonzero(tr["verdict"] != v)[0]
        known, d_vk, d_ug = [], [], []
        for j, (b, pub, kind, k) in enumerate(rows):
            rec, verdict = tr[j], int(tr["verdict"][j])
            seen.add(kind)
            if kind == "valid":
                assert verdict == 0
            if verdict & ~S.VERIFY_EQUATION:
                assert is_zero_elsewhere(rec), (j, kind)
                continue
            same = rec["sum_inf"] == rec["p_inf"] and (rec["sum_xy"] == rec["p_xy"]).all()
            assert bool(verdict & S.VERIFY_EQUATION) == (not same), (j, kind)
            if kind in ("a0_plus_1", "wrong_public", "wrong_trapdoor"):  # K's discrete log is still known
                assert verdict == S.VERIFY_EQUATION, (j, kind)
                alpha = dvp.proving.transcript_challenge(b[:30], pub)
                i0, r0, u0, v0 = sc.trace_scalars(tdv, pub, b, alpha)
                assert [dvp.fr.to_int(rec[f]) for f in FIELDS] == [alpha, i0, r0, u0, v0], (j, kind)
                vk, ug, _ = sc.trace_dlogs(k, u0, v0)
                known.append(j)
                d_vk.append(vk)
                d_ug.append(ug)
        if known:
            assert_points(tr, "vk", *mulgen(dvp, d_vk), rows=known)
            assert_points(tr, "ug", *mulgen(dvp, d_ug), rows=known)
    assert seen == set(vc.TAMPER) | {"valid"}


def test_vk_against_the_oracles_variable_base_multiplication(dvp):
    S = dvp.srs
    pubs, cases, proofs, dlogs = simulated(dvp, 4, n_public=1)
    tr = S.verify_trace(S.Trapdoor(*TD), pubs, proofs)
    for j in range(4):
        pt_k, ok = co.xsk233_decode(proofs[j, 30:60].tobytes())
        assert ok
        want = co.k233_mul(dvp.fr.to_int(tr["v0"][j]), pt_k) if pt_k else None
        got = None if tr["vk_inf"][j] else (dvp.fr.to_int(tr["vk_xy"][j][:4]), dvp.fr.to_int(tr["vk_xy"][j][4:]))
        assert got == want, (j, cases[j])


def test_format_and_parse_round_trip(dvp):
    S = dvp.srs
    pubs, cases, proofs, dlogs = simulated(dvp, 7)
    for rec in S.verify_trace(S.Trapdoor(*TD), pubs, proofs):
        assert S.parse_verify_trace(S.format_verify_trace(rec)) == rec


def test_cli_trace(dvp, tmp_path):
    """examples/dvp_verify_cli --trace prints the record of its proof after the verdict line; the exit status stays 0 / 2"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this box")
    S = dvp.srs
    libdir = os.path.join(ROOT, "dv-pari_amd")
    exe = tmp_path / "dvp_verify_cli"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "dvp_verify_cli.cpp"), "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir,
                           "-pthread", "-o", str(exe)])
    pubs, cases, proofs, dlogs = simulated(dvp, 1)
    good = proofs[0].tobytes()
    bad = bytearray(good)
    bad[60] ^= 0x01
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")
    args = [hex(x) for x in TD] + [hex(x) for x in pubs[0]]
    for name, b, code, word in (("good.bin", good, 0, "accepted"), ("bad.bin", bytes(bad), 2, "rejected")):
        pf = tmp_path / name
        pf.write_bytes(b)
        out = subprocess.run([str(exe), str(pf)] + args + ["--trace"], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == code and out.stdout.splitlines()[0].startswith(word), (out.returncode, out.stdout, out.stderr)
        want = S.verify_trace(S.Trapdoor(*TD), pubs, [b])[0]
        assert S.parse_verify_trace(out.stdout) == want, out.stdout
        assert out.stdout.splitlines()[1:] == S.format_verify_trace(want).splitlines()
        plain = subprocess.run([str(exe), str(pf)] + args, capture_output=True, text=True, env=env, timeout=300)
        assert plain.returncode == code and plain.stdout == out.stdout.splitlines()[0] + "\n"
