"""GPU test (-m gpu): examples/dvp_setup_cli.cpp -- a compiled host that sees only include/dvpari.h -- sets the toy circuit up from
its dump, audits the directory it wrote (exit 0), and names the vector a one-entry overwrite spoils (exit 2), by the combined check
and by --exact alike.  Every run is a fresh child process."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import pyref as o

pytestmark = pytest.mark.gpu


def py_dump(rows, coeffs):
    """rows of (L, R, O) term lists in the gnark dump format (src/gnark_r1cs.rs:84-91,121-185)"""
    out = [struct.pack("<I", len(coeffs))] + [int(c).to_bytes(32, "big") for c in coeffs] + [struct.pack("<I", len(rows))]
    for l, r, oo in rows:
        out.append(struct.pack("<III", len(l), len(r), len(oo)))
        for part in (l, r, oo):
            for w, k in part:
                out.append(struct.pack("<II", w, k))
    return b"".join(out)


def test_setup_cli_sets_up_and_audits(dvp, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx is not None, "the compiled host needs g++"
    exe = tmp_path / "dvp_setup_cli"
    libdir = os.path.join(root, "dv-pari_amd")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "dvp_setup_cli.cpp"),
                           "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    A, g = dvp.artifacts, dvp.gnark_r1cs
    cache = tmp_path / "cache"
    cache.mkdir()
    (cache / A.R1CS_CONSTRAINTS_FILE).write_bytes(py_dump(g.TOY_ROWS, g.TOY_COEFFS))
    rnd = random.Random(41)
    trap = [rnd.randrange(1, o.P) for _ in range(3)]
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")

    def cli(*flags, trapdoor=trap, where=cache):
        return subprocess.run([str(exe), str(where), "2"] + [hex(x) for x in trapdoor] + list(flags), capture_output=True, text=True, env=env, timeout=300)

    out = cli()
    assert out.returncode == 0, out.stderr
    # the files are the ones the library's own setup writes
    ref = tmp_path / "ref"
    ref.mkdir()
    shutil.copy(cache / A.R1CS_CONSTRAINTS_FILE, ref)
    _, pv = dvp.srs.verifier_runs_setup_cache_dir(dvp.srs.Trapdoor(*trap), ref, 2, write_precomputes=False)
    pv.close()
    for name in A.SRS_FILES:
        assert (cache / name).read_bytes() == (ref / name).read_bytes(), name
    assert not (cache / A.Z_POLY).exists()
    for flags in (["--check"], ["--check", "--exact"]):
        out = cli(*flags)
        assert out.returncode == 0 and out.stdout.strip().endswith("accepted"), (out.stdout, out.stderr)
        lines = out.stdout.splitlines()
        assert [ln.split()[0] for ln in lines[:5]] == list(A.SRS_FILES) and all(ln.split()[1] == "ok" for ln in lines[:5])
        assert all(ln.split()[2] == ("exact" if "--exact" in flags else "combined") for ln in lines[:5])
    # one entry of g_k_1 becomes another scalar's multiple
    enc = dvp.io_utils.read_point_vec_payload(cache / A.SRS_G_K_1)
    enc[6] = dvp.curve.point_scalar_mul_gen_batch_bytes(dvp.fr.vec([77]))[0]
    dvp.io_utils.write_point_vec_to_file(cache / A.SRS_G_K_1, enc)
    for flags in (["--check"], ["--check", "--exact"]):
        out = cli(*flags)
        assert out.returncode == 2, (out.stdout, out.stderr)
        lines = out.stdout.splitlines()
        bad = [ln for ln in lines[:5] if ln.split()[1] != "ok"]
        assert len(bad) == 1 and bad[0].split()[:2] == ["g_k_1", "wrong"] and bad[0].endswith("first_bad 6"), out.stdout
        assert bad[0].split()[2] == ("exact" if "--exact" in flags else "located")
        assert lines[5] == "rejected 0x08"
    # another trapdoor: every vector; a zero trapdoor element, a missing directory, a bad command line: exit 1
    out = cli("--check", trapdoor=[trap[0] + 1, trap[1], trap[2]])
    assert out.returncode == 2 and out.stdout.splitlines()[5] == "rejected 0x1f"
    assert cli("--check", trapdoor=[0, trap[1], trap[2]]).returncode == 1
    out = cli("--check", where=tmp_path / "nowhere")
    assert out.returncode == 1 and ("i/o" in out.stderr.lower() or "io error" in out.stderr.lower()), out.stderr
    assert cli("--exact").returncode == 1
    # --precomputes writes the six domain files too
    pre = tmp_path / "pre"
    pre.mkdir()
    shutil.copy(ref / A.R1CS_CONSTRAINTS_FILE, pre)
    assert cli("--precomputes", where=pre).returncode == 0
    for name in (A.Z_POLY, A.Z_POLYD, A.BAR_WTS, A.BAR_WTSD, A.Z_VALS2_INV, A.Z_VALS2D_INV):
        assert (pre / name).exists(), name
