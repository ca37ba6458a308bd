"""GPU tests (-m gpu) of the cache-directory form of prove_multi: three toy directories written by verifier_runs_setup_cache_dir from
three trapdoors; the reference for bytes is Proof.prove on each directory alone."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import pyref as o

pytestmark = pytest.mark.gpu
EINVAL, EIO = -1, -6


def py_dump(rows, coeffs):
    """rows of (L, R, O) term lists in the gnark dump format (src/gnark_r1cs.rs:84-91,121-185)"""
    out = [struct.pack("<I", len(coeffs))] + [int(c).to_bytes(32, "big") for c in coeffs] + [struct.pack("<I", len(rows))]
    for l, r, oo in rows:
        out.append(struct.pack("<III", len(l), len(r), len(oo)))
        for part in (l, r, oo):
            for w, k in part:
                out.append(struct.pack("<II", w, k))
    return b"".join(out)


def make_dir(dvp, path, trap, coeffs=None, witness=True):
    A, g = dvp.artifacts, dvp.gnark_r1cs
    path.mkdir()
    (path / A.R1CS_CONSTRAINTS_FILE).write_bytes(py_dump(g.TOY_ROWS, g.TOY_COEFFS if coeffs is None else coeffs))
    _, pv = dvp.srs.verifier_runs_setup_cache_dir(dvp.srs.Trapdoor(*trap), path, 2, write_precomputes=False)
    pv.close()
    if witness:
        g.write_witness_to_file(path / A.R1CS_WITNESS_FILE, [1] + list(g.TOY_PUBLIC) + list(g.TOY_PRIVATE))
    return path


@pytest.fixture()
def dirs(dvp, tmp_path):
    rnd = random.Random(2024)
    traps = [[rnd.randrange(1, o.P) for _ in range(3)] for _ in range(3)]
    paths = [make_dir(dvp, tmp_path / name, trap) for name, trap in zip("ABC", traps)]
    yield paths, traps
    dvp.proving.release_cache_dir()


def single_proofs(dvp, paths):
    """Proof.prove on each directory alone, each released again"""
    g, out = dvp.gnark_r1cs, []
    for d in paths:
        out.append(dvp.proving.Proof.prove(d, g.TOY_PUBLIC, g.TOY_PRIVATE))
        dvp.proving.release_cache_dir(d)
    return out


def test_prove_multi_over_directories(dvp, dirs, tmp_path):
    (a, b, c), traps = dirs
    g, P = dvp.gnark_r1cs, dvp.proving
    ref = single_proofs(dvp, [a, b, c])
    assert len({p.to_bytes() for p in ref}) == 3
    assert P.Proof.prove_multi([a, b, c], g.TOY_PUBLIC, g.TOY_PRIVATE) == ref
    assert P.add_srs_dir(a, 2, b) == 1 and P.add_srs_dir(a, 2, c) == 2 and P.add_srs_dir(a, 2, b) == 1  # added once
    assert P.Prover.of_cache_dir(a, 2, 8).srs_slots() == [0, 1, 2]
    assert P.Proof.prove_multi([a, c], g.TOY_PUBLIC, g.TOY_PRIVATE) == [ref[0], ref[2]]
    assert P.Proof.prove(a, g.TOY_PUBLIC, g.TOY_PRIVATE) == ref[0]  # the single entry still proves for the directory's own SRS
    for td, proof in zip(traps, ref):
        assert dvp.srs.verify(dvp.srs.Trapdoor(*td), g.TOY_PUBLIC, proof)
    # the witness-file form
    got, pub = P.Proof.prove_multi_witness_file([a, b, c], 2)
    assert got == ref and [int.from_bytes(pub[k].tobytes(), "little") for k in range(2)] == list(g.TOY_PUBLIC)
    got, _ = P.Proof.prove_multi_witness_file([a, b], 2, witness_path=c / dvp.artifacts.R1CS_WITNESS_FILE)
    assert got == ref[:2]
    # the binding of one slot: slot 1 bound to its own SRS hash, the others untouched
    P.set_cache_dir_slot_binding(a, 2, 1, bind_srs=True)
    got = P.Proof.prove_multi([a, b, c], g.TOY_PUBLIC, g.TOY_PRIVATE)
    assert got[0] == ref[0] and got[2] == ref[2] and got[1].commit_p == ref[1].commit_p and got[1] != ref[1]
    pv = P.Prover.of_cache_dir(a, 2, 8)
    pv.select_srs(1)
    h1 = pv.srs_hash()
    pv.select_srs(0)
    try:
        dvp.srs.set_verify_binding(h1, None)
        assert dvp.srs.verify(dvp.srs.Trapdoor(*traps[1]), g.TOY_PUBLIC, got[1])
    finally:
        dvp.srs.set_verify_binding(None, None)
    P.set_cache_dir_slot_binding(a, 2, 1)
    assert P.Proof.prove_multi([a, b, c], g.TOY_PUBLIC, g.TOY_PRIVATE) == ref
    with pytest.raises(dvp.DvpError) as e:
        P.set_cache_dir_slot_binding(a, 2, 5)
    assert e.value.status == EINVAL


def test_directories_that_do_not_fit(dvp, dirs, tmp_path):
    (a, b, c), traps = dirs
    g, P = dvp.gnark_r1cs, dvp.proving
    # another circuit: same shape, another coefficient table
    coeffs = list(g.TOY_COEFFS)
    coeffs[-1] = (coeffs[-1] + 1) % o.P
    other = make_dir(dvp, tmp_path / "other", traps[1], coeffs=coeffs)
    assert P.circuit_hash_cache_dir(other, 2) != P.circuit_hash_cache_dir(a, 2)
    with pytest.raises(dvp.DvpError) as e:
        P.add_srs_dir(a, 2, other)
    assert e.value.status == EINVAL
    # g_q cut short
    short = tmp_path / "short"
    shutil.copytree(b, short)
    raw = (short / dvp.artifacts.SRS_FILES[1]).read_bytes()
    (short / dvp.artifacts.SRS_FILES[1]).write_bytes(raw[:-7])
    with pytest.raises(dvp.DvpError) as e:
        P.add_srs_dir(a, 2, short)
    assert e.value.status == EIO
    # a point file of another length (the count is right for its own length)
    wrong = tmp_path / "wrong"
    shutil.copytree(b, wrong)
    raw = (wrong / dvp.artifacts.SRS_FILES[1]).read_bytes()
    (wrong / dvp.artifacts.SRS_FILES[1]).write_bytes(struct.pack("<Q", 7) + raw[8:8 + 30 * 7])
    with pytest.raises(dvp.DvpError) as e:
        P.add_srs_dir(a, 2, wrong)
    assert e.value.status == EINVAL
    with pytest.raises(dvp.DvpError) as e:
        P.add_srs_dir(a, 2, tmp_path / "nowhere")
    assert e.value.status == EIO
    # none of them left a slot behind, and an SRS directory without a dump is taken as it is
    assert P.Prover.of_cache_dir(a, 2, 8).srs_slots() == [0]
    bare = tmp_path / "bare"
    bare.mkdir()
    for name in dvp.artifacts.SRS_FILES:
        shutil.copy(c / name, bare)
    assert P.add_srs_dir(a, 2, bare) == 1
    ref_c = single_proofs(dvp, [c])[0]
    assert P.Proof.prove_multi([a, bare], g.TOY_PUBLIC, g.TOY_PRIVATE)[1] == ref_c
    with pytest.raises(TypeError):
        P.Proof.prove_multi(str(a), g.TOY_PUBLIC, g.TOY_PRIVATE)


def test_prove_cli_also(dvp, dirs, tmp_path):
    """dvp_prove_cli <A> 2 --also <B> --also <C>: three lines, each accepted by dvp_verify_cli under its directory's trapdoor"""
    (a, b, c), traps = dirs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx is not None, "the compiled host needs g++"
    libdir = os.path.join(root, "dv-pari_amd")
    exes = {}
    for name in ("dvp_prove_cli", "dvp_verify_cli"):
        exes[name] = tmp_path / name
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", name + ".cpp"),
                               "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-pthread", "-o", str(exes[name])])
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")
    ref = single_proofs(dvp, [a, b, c])
    for flags in ([], ["--trace"]):
        out = subprocess.run([str(exes["dvp_prove_cli"]), str(a), "2", "--also", str(b), "--also", str(c)] + flags, capture_output=True, text=True,
                             env=env, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert [ln.split() for ln in lines[:3]] == [[str(d), p.to_bytes().hex()] for d, p in zip((a, b, c), ref)]
        if flags:  # the trace is the first proof's
            rec = dvp.proving.parse_prove_trace("\n".join(lines[3:]))
            assert rec["commit_p"]["enc"] == ref[0].commit_p and rec["kzg_k"]["enc"] == ref[0].kzg_k
        else:
            assert len(lines) == 3
    pub = [hex(x) for x in dvp.gnark_r1cs.TOY_PUBLIC]
    for k, (trap, proof) in enumerate(zip(traps, ref)):
        f = tmp_path / f"proof{k}.bin"
        f.write_bytes(proof.to_bytes())
        for j, other in enumerate(traps):
            out = subprocess.run([str(exes["dvp_verify_cli"]), str(f)] + [hex(x) for x in other] + pub, capture_output=True, text=True, env=env,
                                 timeout=300)
            assert out.returncode == (0 if j == k else 2), (k, j, out.stdout, out.stderr)
    out = subprocess.run([str(exes["dvp_prove_cli"]), str(a), "2", "--also", str(b), "--also", str(tmp_path / "nowhere")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert out.returncode != 0 and not out.stdout.strip()
    out = subprocess.run([str(exes["dvp_prove_cli"]), str(a), "2", "--also", str(b), "--host-witness"], capture_output=True, text=True, env=env,
                         timeout=300)
    assert out.returncode == 2
