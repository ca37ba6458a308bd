"""GPU tests (-m gpu) of the circuit hash: dvp_prover_circuit_hash against BLAKE3 of the oracle's stream (tests/circuit_hash_cases.py:
built from pyref.r1cs_with_vandermonde, never from the library) on every case at the default window and at windows of 1, 2 and 3
chunks; the cache-dir entry; the errors; the launch census of the generator; the binding end to end through prover, verifier and
the compiled host."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pyref as o
import circuit_hash_cases as cc
import msm_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_vectors.json")))
EINVAL, EIO = -1, -6
KNOB = "DVP_CIRCUIT_HASH_WINDOW"
ROWS, COEFFS, LEAVES = "circuit_hash.hip:k_ch_rows", "circuit_hash.hip:k_ch_coeffs", "blake3_tree.hip:k_b3_leaves"
STARTS = "circuit_hash.hip:k_ch_row_starts"  # the row search of k_ch_rows' workgroups: one launch in front of each of its launches


def csr(rows):
    rp = np.zeros(len(rows) + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    flat = [t for r in rows for t in r]
    return rp, np.array([t[0] for t in flat] or [0], dtype=np.uint32), np.array([t[1] for t in flat] or [0], dtype=np.uint32)


def bare_prover(dvp, case, matrices=(0, 1, 2)):
    """a prover without SRS holding the case's coefficients and the listed matrices, each under its OWN n_rows"""
    lib, ptr = dvp.lib, dvp._native.ptr
    pv = dvp.proving.Prover.__new__(dvp.proving.Prover)
    pv.inst, pv.m, pv.log_m = None, case.m, case.log_m
    h = C.c_void_p()
    dvp.check(lib.dvp_prover_create(case.log_m, case.k, case.n_wires, C.byref(h)), "dvp_prover_create")
    pv._h = h
    dvp.check(lib.dvp_prover_set_coeffs(h, ptr(dvp.fr.vec(case.coeffs)), len(case.coeffs)), "dvp_prover_set_coeffs")
    for which in matrices:
        rp, wi, ci = csr(case.mats[which])
        dvp.check(lib.dvp_prover_set_matrix(h, which, len(case.mats[which]), ptr(rp), ptr(wi), ptr(ci)), "dvp_prover_set_matrix")
    return pv


def window(dvp, w):
    return dvp.tune(**({} if w is None else {KNOB: w}))


@pytest.mark.parametrize("case", cc.CASES, ids=repr)
def test_circuit_hash_vs_oracle_stream(dvp, case):
    s, _ = cc.stream(case)
    want = cc.digest(case)
    if len(s) > 4096:
        assert dvp.proving.blake3(s) == want  # the host flavour agrees with the oracle's on the longer streams
    pv = bare_prover(dvp, case)
    try:
        assert from_ints(pv.domains()[0]) == list(cc.domain(case.log_m))  # the prover's D is the oracle's
        for w in cc.WINDOWS:
            with window(dvp, w):
                assert pv.circuit_hash() == want, (case, w)
    finally:
        pv.close()


def from_ints(limbs):
    return [int.from_bytes(limbs[i].tobytes(), "little") for i in range(limbs.shape[0])]


def test_generator_launches(dvp):
    """both generator kernels and k_b3_leaves run; at window = 1 chunk the leaves run once per chunk, the row kernel once per window
    that holds row dwords and the coefficient kernel once per window that holds coefficient dwords; a single-chunk stream takes the
    ROOT flavour of the leaves kernel alone (no tree)"""
    case = cc.BY_NAME["sparse-8"]
    s, row_bytes = cc.stream(case)
    nchunks = -(-len(s) // 1024)
    pv = bare_prover(dvp, case)
    try:
        dvp.lib.dvp_profile_reset()
        assert pv.circuit_hash() == cc.digest(case)
        assert (mc.launches(dvp, STARTS), mc.launches(dvp, ROWS), mc.launches(dvp, COEFFS), mc.launches(dvp, LEAVES)) == (1, 1, 1, 1)
        assert mc.launches(dvp, "circuit_hash.hip:k_ch_find_minus_one") == 1 and mc.launches(dvp, "blake3_tree.hip:k_b3_tree") == 1
        for w in (1, 2, 3):
            dvp.lib.dvp_profile_reset()
            with window(dvp, w):
                assert pv.circuit_hash() == cc.digest(case)
            nwin = -(-nchunks // w)
            assert mc.launches(dvp, LEAVES) == nwin
            assert mc.launches(dvp, ROWS) == -(-row_bytes // (1024 * w))  # row_bytes is no multiple of 1024: the last of them is shared
            assert mc.launches(dvp, COEFFS) == nwin - row_bytes // (1024 * w)
            assert mc.launches(dvp, STARTS) == mc.launches(dvp, ROWS)
            assert mc.launches(dvp, ROWS) + mc.launches(dvp, COEFFS) == nwin + 1  # one window holds the end of one part and the head of the other
    finally:
        pv.close()
    small = cc.BY_NAME["toy-k1"]
    pv = bare_prover(dvp, small)
    try:
        dvp.lib.dvp_profile_reset()
        assert pv.circuit_hash() == cc.digest(small)
        assert mc.launches(dvp, LEAVES) == 1 and mc.launches(dvp, "blake3_tree.hip:k_b3_tree") == 0
    finally:
        pv.close()


def test_incomplete_prover_is_einval(dvp):
    case = cc.BY_NAME["toy-k2"]
    for have in ((), (0, 1), (1, 2)):
        pv = bare_prover(dvp, case, have)
        with pytest.raises(dvp.DvpError) as e:
            pv.circuit_hash()
        assert e.value.status == EINVAL
        pv.close()
    # matrices but no coefficients
    pv = dvp.proving.Prover.__new__(dvp.proving.Prover)
    pv.inst, pv.m, pv.log_m = None, case.m, case.log_m
    h = C.c_void_p()
    dvp.check(dvp.lib.dvp_prover_create(case.log_m, case.k, case.n_wires, C.byref(h)))
    pv._h = h
    for which in range(3):
        rp, wi, ci = csr(case.mats[which])
        dvp.check(dvp.lib.dvp_prover_set_matrix(h, which, len(case.mats[which]), dvp._native.ptr(rp), dvp._native.ptr(wi), dvp._native.ptr(ci)))
    with pytest.raises(dvp.DvpError) as e:
        pv.circuit_hash()
    assert e.value.status == EINVAL
    # a coefficient table shorter than the ids the matrices hold (set afterwards): what dvp_prove answers too
    dvp.check(dvp.lib.dvp_prover_set_coeffs(h, dvp._native.ptr(dvp.fr.vec([5])), 1))
    with pytest.raises(dvp.DvpError) as e:
        pv.circuit_hash()
    assert e.value.status == EINVAL
    dvp.check(dvp.lib.dvp_prover_set_coeffs(h, dvp._native.ptr(dvp.fr.vec(case.coeffs)), len(case.coeffs)))
    assert pv.circuit_hash() == cc.digest(case)
    pv.close()


@pytest.fixture(scope="module")
def toy_dir(dvp, tmp_path_factory):
    """the toy cache directory: dump, witness file, SRS files written by the setup; the prover the setup returns"""
    A, g = dvp.artifacts, dvp.gnark_r1cs
    cache = tmp_path_factory.mktemp("toy_cache")
    (cache / A.R1CS_CONSTRAINTS_FILE).write_bytes(cc.py_dump(g.TOY_ROWS, g.TOY_COEFFS))
    g.write_witness_to_file(cache / A.R1CS_WITNESS_FILE, [1] + g.TOY_PUBLIC + g.TOY_PRIVATE)
    td = dvp.srs.Trapdoor(*(int(x, 16) for x in VEC["toy"]["trapdoor"]))
    inst, pv = dvp.srs.verifier_runs_setup_cache_dir(td, cache, 2)
    yield cache, td, pv
    dvp.proving.release_cache_dir(cache)
    pv.close()


def test_cache_dir_entry(dvp, toy_dir, tmp_path):
    """from the dump alone (no prover open), through the directory's open prover, after its release, under another public-input
    count, and at a small window: always the oracle's digest; a missing dump is DVP_EIO"""
    cache, td, pv = toy_dir
    P, g = dvp.proving, dvp.gnark_r1cs
    want = cc.digest(cc.BY_NAME["toy-k2"])
    P.release_cache_dir(cache)
    assert P.circuit_hash_cache_dir(cache, 2) == want  # a temporary prover without SRS
    assert pv.circuit_hash() == want
    golden = P.Proof.prove(cache, g.TOY_PUBLIC, g.TOY_PRIVATE)  # opens the directory's prover
    dvp.lib.dvp_profile_reset()
    assert P.circuit_hash_cache_dir(cache, 2) == want
    assert mc.launches(dvp, "prove.hip:k_domain_tables") == 0 and mc.launches(dvp, ROWS) == 1  # the open prover was used: none was built
    assert P.Prover.of_cache_dir(cache, 2, 8).circuit_hash() == want
    P.release_cache_dir(cache)
    dvp.lib.dvp_profile_reset()
    with window(dvp, 1):
        assert P.circuit_hash_cache_dir(cache, 2) == want
    assert mc.launches(dvp, "prove.hip:k_domain_tables") == 1  # released: built from the dump again
    assert P.circuit_hash_cache_dir(cache, 5) == cc.digest(cc.BY_NAME["toy-k5"])
    assert P.circuit_hash_cache_dir(cache, 0) == cc.digest(cc.BY_NAME["toy-k0"])
    assert golden.commit_p.hex() == VEC["toy"]["commit_p"] and golden.kzg_k.hex() == VEC["toy"]["kzg_k"]
    with pytest.raises(dvp.DvpError) as e:
        P.circuit_hash_cache_dir(tmp_path, 2)
    assert e.value.status == EIO
    P.release_cache_dir(cache)


def test_binding_end_to_end(dvp, toy_dir):
    """prover bound to (srs_hash(), circuit_hash()); the verifier, who has only the directory, accepts under (srs hash,
    circuit_hash_cache_dir) and rejects with DVP_VERIFY_EQUATION under the hash of the circuit with one coeff_id changed and under no
    binding; with no binding anywhere the proof is the toy golden"""
    cache, td, pv = toy_dir
    S, P, g = dvp.srs, dvp.proving, dvp.gnark_r1cs
    pub, prv = g.TOY_PUBLIC, g.TOY_PRIVATE
    s, c = pv.srs_hash(), pv.circuit_hash()
    assert c == cc.digest(cc.BY_NAME["toy-k2"])
    pv.set_transcript_binding(s, c)
    try:
        proof = pv.prove(pub, prv)
    finally:
        pv.set_transcript_binding(None, None)
    unbound = pv.prove(pub, prv)
    assert unbound.commit_p.hex() == VEC["toy"]["commit_p"] and unbound.kzg_k.hex() == VEC["toy"]["kzg_k"]  # the parent commit's bytes
    assert proof.commit_p == unbound.commit_p and proof != unbound
    P.release_cache_dir(cache)
    other = o.blake3(cc.stream_of(*cc.oracle_instance(cc.toy_with_changed_coeff_id(2)))[0])
    assert other != c
    try:
        S.set_verify_binding(s, P.circuit_hash_cache_dir(cache, 2))
        assert int(S.verify_batch(td, [pub], [proof])[0]) == 0
        assert S.verify(td, pub, proof)
        assert int(S.verify_batch(td, [pub], [unbound])[0]) == S.VERIFY_EQUATION
        S.set_verify_binding(s, other)
        assert int(S.verify_batch(td, [pub], [proof])[0]) == S.VERIFY_EQUATION
        S.set_verify_binding(s, None)
        assert int(S.verify_batch(td, [pub], [proof])[0]) == S.VERIFY_EQUATION
    finally:
        S.set_verify_binding(None, None)
    assert int(S.verify_batch(td, [pub], [proof])[0]) == S.VERIFY_EQUATION  # no binding
    assert int(S.verify_batch(td, [pub], [unbound])[0]) == 0
    # the device computes the changed circuit's hash as the oracle does
    q = bare_prover(dvp, cc.toy_with_changed_coeff_id(2))
    assert q.circuit_hash() == other
    q.close()


def test_compiled_host_binds_the_circuit(dvp, toy_dir, tmp_path):
    """dvp_prove_cli --bind-srs --bind-circuit on the toy directory, both flavours: the two hashes on stderr are the prover's, and
    the verifier accepts the printed proof under them; together with --circuit-hash it is a usage error"""
    cache, td, pv = toy_dir
    S, g = dvp.srs, dvp.gnark_r1cs
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this box")
    exe = tmp_path / "dvp_prove_cli"
    libdir = os.path.join(ROOT, "dv-pari_amd")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "dvp_prove_cli.cpp"),
                           "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-pthread", "-o", str(exe)])
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")
    want_s, want_c = pv.srs_hash(), pv.circuit_hash()
    for extra in ([], ["--host-witness"]):
        out = subprocess.run([str(exe), str(cache), "2", "--bind-srs", "--bind-circuit"] + extra, capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr
        s = bytes.fromhex(re.search(r"^srs hash: ([0-9a-f]{64})$", out.stderr, re.M).group(1))
        c = bytes.fromhex(re.search(r"^circuit hash: ([0-9a-f]{64})$", out.stderr, re.M).group(1))
        assert (s, c) == (want_s, want_c)
        proof = bytes.fromhex(out.stdout.strip())
        try:
            S.set_verify_binding(s, c)
            assert int(S.verify_batch(td, [g.TOY_PUBLIC], [proof])[0]) == 0
        finally:
            S.set_verify_binding(None, None)
        assert int(S.verify_batch(td, [g.TOY_PUBLIC], [proof])[0]) == S.VERIFY_EQUATION
    out = subprocess.run([str(exe), str(cache), "2", "--bind-circuit", "--circuit-hash", "00" * 32], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 2 and "usage:" in out.stderr
