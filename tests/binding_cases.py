"""Shared by the transcript-binding tests (test_binding_cpu.py, test_gpu_binding.py): the oracle's transcript with the two
compile-time hashes as parameters, the verifier's verdict under a binding, and the long BLAKE3 fixture."""
import json
import os

import c_oracle as co
import pyref as o

P = o.P
B3_LONG = {int(n): h for n, h in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "blake3_long.json"))).items()}


def b3_input(n):
    """the published BLAKE3 test input: byte i = i mod 251"""
    return bytes(i % 251 for i in range(n))


def bound_challenge(commit_p_bytes: bytes, public_inputs, srs_hash=None, circuit_hash=None) -> int:
    """Transcript::output, src/proving.rs:164-197, restated like pyref.transcript_challenge with srs_hash / circuit_hash as
    parameters (None = BLAKE3(b""), the buffers the reference leaves empty, :86-105,113-132)"""
    srs_hash = o.blake3(b"") if srs_hash is None else bytes(srs_hash)
    circuit_hash = o.blake3(b"") if circuit_hash is None else bytes(circuit_hash)
    assert len(srs_hash) == 32 and len(circuit_hash) == 32
    wc_hash = o.blake3(commit_p_bytes)  # :137-146
    pi_hash = o.blake3(b"".join((x % P).to_bytes(29, "little") for x in public_inputs))  # :149-161
    compile_hash = o.blake3(srs_hash + circuit_hash)
    runtime_hash = o.blake3(wc_hash + pi_hash)
    root = bytearray(o.blake3(compile_hash + runtime_hash))
    root[28:] = b"\0\0\0\0"  # :190
    return int.from_bytes(root, "little") % P


def challenge_fn(srs_hash, circuit_hash):
    return lambda commit_p, pub: bound_challenge(commit_p, pub, srs_hash, circuit_hash)


def oracle_verdict_bound(td, pub, proof: bytes, srs_hash, circuit_hash) -> bool:
    """verify_cases.oracle_verdict (SRS::verify, src/srs.rs:374-428, on the C oracle) with the bound transcript"""
    tau, delta, eps = td
    pt_p, ok_p = co.xsk233_decode(proof[0:30])
    pt_k, ok_k = co.xsk233_decode(proof[30:60])
    a0, b0 = int.from_bytes(proof[60:89], "little"), int.from_bytes(proof[89:118], "little")
    ok_a, ok_b = a0 < P, b0 < P
    a0, b0 = (a0 if ok_a else 0), (b0 if ok_b else 0)
    enc_p = co.xsk233_encode(pt_p) if ok_p else bytes(30)
    alpha = bound_challenge(enc_p, pub, srs_hash, circuit_hash)
    i0 = o.evaluate_monomial_basis_poly(pub, alpha)
    r0 = (a0 * b0 - i0) % P
    u0 = (a0 + delta * b0 + delta * delta % P * r0) % P * eps % P
    v0 = (tau - alpha) * eps % P
    lhs = o.k233_add(co.k233_mul(v0, pt_k) if (ok_k and v0) else None, co.k233_mulgen(u0) if u0 else None)
    return (lhs == (pt_p if ok_p else None)) and ok_p and ok_k and ok_a and ok_b


def srs_stream(st, n_wires, rule=0):
    """the bytes Transcript::srs_hash would hash (src/proving.rs:91-101): to_bytes() of g_k[0], g_k[1], g_k[2], g_q, g_m, from the
    oracle's setup scalars `st` (pyref.setup_srs_scalars); g_m zero-padded to n_wires like the prover's"""
    scalars = st["g_k"][0] + st["g_k"][1] + st["g_k"][2] + st["g_q"] + st["g_m"] + [0] * (n_wires - len(st["g_m"]))
    out = []
    for k in scalars:
        pt = co.k233_mulgen(k % P) if k % P else None
        out.append(co.xsk233_encode(pt) if rule == 0 else o.xsk233_encode(pt, rule))
    return b"".join(out)
