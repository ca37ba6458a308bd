"""GPU tests (-m gpu) of the verifier (csrc/verify.hip: dvp_verify, dvp_verify_batch, dvp_verify_batch_dev, srs.verify_batch):
synthetic valid proofs of every exceptional shape are accepted, tampered ones get the reference's verdict index for index,
real proofs of the GPU prover are accepted, the flavours agree, and a compiled host verifies over the header alone."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import c_oracle as co
import pyref as o
import verify_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_vectors.json")))
TD = (0x3D9F1A77 * 104729 % o.P, 0xC0FFEE1234567 % o.P, 0xDEADBEEF987654321 % o.P)


def gpu_encode_many(dvp):
    def enc(dlogs):
        s = np.zeros((len(dlogs), 4), dtype=np.uint64)
        if dlogs:
            s[:] = np.frombuffer(b"".join(int(k % o.P).to_bytes(32, "little") for k in dlogs), dtype="<u8").reshape(-1, 4)
        out = np.zeros((len(dlogs), 30), dtype=np.uint8)
        dvp.check(dvp.lib.dvp_mulgen_batch(dvp._native.ptr(s), len(dlogs), dvp._native.ptr(out)), "dvp_mulgen_batch")
        return [out[i].tobytes() for i in range(len(dlogs))]
    return enc


def bulk(dvp, td, pubs, cases, seed):
    return vc.build(td, pubs, cases, seed=seed, encode_many=gpu_encode_many(dvp), challenge=dvp.proving.transcript_challenge)


def run_batch(dvp, rows):
    """rows: (proof bytes, trapdoor, pub) with ONE trapdoor and one public-input count per call -> verdicts"""
    td = dvp.srs.Trapdoor(*rows[0][1])
    assert all(r[1] == rows[0][1] for r in rows)
    return dvp.srs.verify_batch(td, [r[2] for r in rows], [r[0] for r in rows])


@pytest.mark.parametrize("n_public", [0, 1, 2, 35, 36, 100])
def test_accepts_valid_synthetic_proofs(dvp, n_public):
    """thousands of valid proofs (and every exceptional case, twice) at each public-input count: all verdicts 0.  36 and 100 public
    inputs take the multi-chunk BLAKE3 of the public-input hash"""
    rng = random.Random(n_public)
    n = 1500 if n_public <= 35 else 300
    cases = [None] * n + [c for c in vc.CASES if c != "v0_zero"] * 2
    rng.shuffle(cases)
    pubs = [[rng.randrange(o.P) for _ in range(n_public)] for _ in cases]
    built = bulk(dvp, TD, pubs, cases, seed=100 + n_public)
    v = run_batch(dvp, [(c["proof"], c["td"], c["pub"]) for c in built])
    bad = [(i, built[i]["case"], int(v[i])) for i in np.nonzero(v)[0]]
    assert not bad, bad[:10]
    # v0 = 0: the trapdoor is tau = alpha of each proof, so one call per proof
    for c in vc.build(TD, pubs[:3], ["v0_zero"] * 3, seed=7 + n_public):
        assert dvp.srs.verify_device(dvp.srs.Trapdoor(*c["td"]), c["pub"], c["proof"]), n_public
    # the oracle agrees on a sample (the bulk encodings and challenges came from the library itself)
    for c in built[:: max(1, len(built) // 12)]:
        assert vc.oracle_verdict(c["td"], c["pub"], c["proof"]), c["case"]


def test_rejects_tampered_proofs_index_for_index(dvp):
    """2^16 + 37 proofs, tampered ones of every kind at random positions: each verdict is 0 exactly when the reference's
    boolean (oracle_verdict, on the C oracle) is true, the validity bits name the bad field, EQUATION only with valid inputs"""
    rng = random.Random(2024)
    n = (1 << 16) + 37
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in range(n)]
    cases = [None] * n
    built = bulk(dvp, TD, pubs, cases, seed=77)
    rows = [(c["proof"], c["td"], c["pub"]) for c in built]
    expect = {}
    pos = rng.sample(range(n), 4 * len(vc.TAMPER) + 3 * len(vc.CASES))
    k = 0
    for kind in vc.TAMPER:
        for _ in range(4):
            i = pos[k]
            k += 1
            b, td, pub = vc.tamper(built[i], kind, rng)
            if kind == "wrong_trapdoor":  # one trapdoor per batch: the equation breaks the same way with another tau on this proof
                b, td = built[i]["proof"][:60] + ((built[i]["a0"] + 7) % o.P).to_bytes(29, "little") + b[89:], TD
            rows[i] = (b, TD, pub)
            expect[i] = (kind, vc.oracle_verdict(TD, pub, b))
    # exceptional valid cases in the same batch (v0 = 0 needs its own trapdoor: test_accepts_valid_synthetic_proofs)
    exc = bulk(dvp, TD, [pubs[pos[k + j]] for j in range(3 * len(vc.CASES))],
               [c for c in vc.CASES for _ in range(3)], seed=78)
    for j, c in enumerate(exc):
        i = pos[k + j]
        if c["case"] == "v0_zero":
            continue
        rows[i] = (c["proof"], TD, c["pub"])
        expect[i] = (c["case"], True)
    v = run_batch(dvp, rows)
    S = dvp.srs
    for i, (kind, ok) in expect.items():
        assert (v[i] == 0) == ok, (i, kind, int(v[i]))
        if kind in ("a0_ge_p",):
            assert v[i] & S.VERIFY_BAD_A0 and not v[i] & S.VERIFY_EQUATION
        if kind in ("b0_ge_p",):
            assert v[i] & S.VERIFY_BAD_B0 and not v[i] & S.VERIFY_EQUATION
        if kind in ("bad_commit", "spare_commit"):
            assert v[i] & S.VERIFY_BAD_COMMIT_P and not v[i] & S.VERIFY_EQUATION
        if kind in ("bad_kzg", "spare_kzg"):
            assert v[i] & S.VERIFY_BAD_KZG_K and not v[i] & S.VERIFY_EQUATION
        if kind in ("a0_plus_1", "wrong_public", "wrong_trapdoor"):
            assert v[i] == S.VERIFY_EQUATION
    rest = np.ones(n, dtype=bool)
    rest[list(expect)] = False
    assert not v[rest].any(), np.nonzero(v * rest)[0][:10]
    # srs.verify (the Python check every other test uses) agrees on a sample of the tampered cases
    for i in list(expect)[:: 6]:
        b, td, pub = rows[i]
        assert S.verify(S.Trapdoor(*td), pub, b) == (v[i] == 0), (i, expect[i])


def _toy(dvp):
    toy = VEC["toy"]
    H = lambda x: int(x, 16)  # noqa: E731
    td = dvp.srs.Trapdoor(*(H(x) for x in toy["trapdoor"]))
    proof = bytes.fromhex(toy["commit_p"]) + bytes.fromhex(toy["kzg_k"]) + H(toy["a0"]).to_bytes(29, "little") + H(toy["b0"]).to_bytes(29, "little")
    return td, list(o.TOY_PUBLIC), proof


def _agree_on_real_proof(dvp, td, pub, proof):
    S = dvp.srs
    assert S.verify(td, pub, proof)
    assert S.verify_device(td, pub, proof)
    assert S.verify_batch(td, [pub], [proof])[0] == 0
    rng = random.Random(len(pub))
    case = dict(proof=proof, td=(td.tau, td.delta, td.epsilon), pub=pub, a0=int.from_bytes(proof[60:89], "little"))
    rows = [vc.tamper(case, kind, rng) for kind in vc.TAMPER]
    for b, t, p in rows:
        tdx = S.Trapdoor(*t)
        ref = S.verify(tdx, p, b)
        assert S.verify_device(tdx, p, b) == ref
        if len(p) == len(pub) and t == case["td"]:
            assert (S.verify_batch(tdx, [p], [b])[0] == 0) == ref
        assert not ref


def test_golden_toy_proof(dvp):
    """the reference-shaped toy proof and trapdoor of the golden vectors (src/dvsnark_test.rs:131-180)"""
    _agree_on_real_proof(dvp, *_toy(dvp))


def test_gpu_proof_of_sparse_cache_dir(dvp, tmp_path):
    """a GPU proof of the 2^12 sparse circuit, set up and proved through the cache_dir entries"""
    A, g = dvp.artifacts, dvp.gnark_r1cs
    inst0, pub, prv = g.synthetic_sparse(12)
    cache = tmp_path / "cache"
    cache.mkdir()
    inst0.write_dump_file(cache / A.R1CS_CONSTRAINTS_FILE)
    rnd = random.Random(41)
    td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
    _, pv = dvp.srs.verifier_runs_setup_cache_dir(td, cache, len(pub), write_precomputes=False)
    proof = pv.prove(pub, prv).to_bytes()
    pv.close()
    _agree_on_real_proof(dvp, td, list(pub), proof)


def test_dev_flavour_on_a_stream_matches_host(dvp):
    """dvp_verify_batch_dev on torch tensors and a non-default stream: the same bytes as the host flavour; a non-canonical public
    input is the BAD_PUBLIC verdict of its proof there"""
    import ctypes as C

    import torch

    rng = random.Random(3)
    n = 3000
    pubs = [[rng.randrange(o.P) for _ in range(3)] for _ in range(n)]
    built = bulk(dvp, TD, pubs, [None] * n, seed=5)
    rows = [(c["proof"], TD, c["pub"]) for c in built]
    for i in range(0, n, 97):
        rows[i] = vc.tamper(built[i], vc.TAMPER[i % 11], rng)[:1] + (TD, pubs[i])
    host = run_batch(dvp, rows)
    pa = np.frombuffer(b"".join(r[0] for r in rows), dtype=np.uint8).reshape(n, 118)
    pub = dvp.srs._public_array([r[2] for r in rows], n)
    pub[5, 1] = np.frombuffer(o.P.to_bytes(32, "little"), dtype="<u8")  # non-canonical
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(pa.copy()).to(dev)
    tpub = torch.from_numpy(pub.view(np.int64).copy()).to(dev)
    tv = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    keep, (t, d, e) = dvp.srs._trapdoor_args(dvp.srs.Trapdoor(*TD))
    with torch.cuda.stream(s):
        rc = dvp.lib.dvp_verify_batch_dev(t, d, e, C.c_void_p(tpub.data_ptr()), 3, C.c_void_p(tp.data_ptr()), n, C.c_void_p(tv.data_ptr()),
                                          C.c_void_p(s.cuda_stream))
    assert rc == 0
    s.synchronize()
    got = tv.cpu().numpy()
    exp = host.copy()
    exp[5] = dvp.srs.VERIFY_BAD_PUBLIC | (host[5] & ~np.uint8(dvp.srs.VERIFY_EQUATION))
    assert (got == exp).all(), np.nonzero(got != exp)[0][:10]


def test_second_codec_rule(dvp):
    """under another dvp_codec_set_rule value, proofs encoded by that rule are accepted; read back under rule 0 they are not"""
    S = dvp.srs
    rule = 1
    enc = lambda dl: vc.oracle_encode_many(dl, rule=rule)  # noqa: E731
    rng = random.Random(8)
    pubs = [[rng.randrange(o.P)] for _ in range(20)]
    cases = [None] * 13 + [c for c in vc.CASES if c != "v0_zero"]
    dvp.check(dvp.lib.dvp_codec_set_rule(rule))
    try:
        built = vc.build(TD, pubs, cases, seed=9, encode_many=enc)
        v = S.verify_batch(S.Trapdoor(*TD), [c["pub"] for c in built], [c["proof"] for c in built])
        assert not v.any(), v
        for c in built[:3]:
            assert S.verify(S.Trapdoor(*TD), c["pub"], c["proof"])
    finally:
        dvp.check(dvp.lib.dvp_codec_set_rule(0))
    v0 = S.verify_batch(S.Trapdoor(*TD), [c["pub"] for c in built], [c["proof"] for c in built])
    # rule 1 holds w + 1 = w(-Q): read under rule 0 the bytes are -P and -K with the same transcript, so the equation holds
    # exactly when u0 G = -u0 G, i.e. u0 = 0
    for c, v in zip(built, v0):
        assert (v == 0) == (c["case"] == "u0_zero" or (c["p"] == 0 and c["k"] == 0)), (c["case"], int(v))


def test_cpp_verify_cli(dvp, tmp_path):
    """examples/dvp_verify_cli.cpp (plain g++ over include/dvpari.h) accepts a proof written by dvp_prove_cli (exit 0) and rejects
    it after one byte of a0 changed (exit 2)"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this box")
    libdir = os.path.join(ROOT, "dv-pari_amd")
    exes = {}
    for name in ("dvp_prove_cli", "dvp_verify_cli"):
        exes[name] = tmp_path / name
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", name + ".cpp"), "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir,
                               "-pthread", "-o", str(exes[name])])
    A, g = dvp.artifacts, dvp.gnark_r1cs
    inst0, pub, prv = g.synthetic_sparse(10)
    cache = tmp_path / "cache"
    cache.mkdir()
    inst0.write_dump_file(cache / A.R1CS_CONSTRAINTS_FILE)
    g.write_witness_to_file(cache / A.R1CS_WITNESS_FILE, [1] + pub + prv)
    rnd = random.Random(31)
    td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
    dvp.srs.verifier_runs_setup_cache_dir(td, cache, len(pub), write_precomputes=False)[1].close()
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")
    pf = tmp_path / "proof.bin"
    out = subprocess.run([str(exes["dvp_prove_cli"]), str(cache), str(len(pub)), str(pf)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    args = [hex(x) for x in (td.tau, td.delta, td.epsilon)] + [hex(x) for x in pub]
    out = subprocess.run([str(exes["dvp_verify_cli"]), str(pf)] + args, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "accepted" in out.stdout, (out.returncode, out.stdout, out.stderr)
    b = bytearray(pf.read_bytes())
    b[60] ^= 0x01
    bad = tmp_path / "bad.bin"
    bad.write_bytes(bytes(b))
    out = subprocess.run([str(exes["dvp_verify_cli"]), str(bad)] + args, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 2 and "rejected" in out.stdout and "equation" in out.stdout, (out.returncode, out.stdout, out.stderr)
    out = subprocess.run([str(exes["dvp_verify_cli"]), str(pf), "zz", "1", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 1
