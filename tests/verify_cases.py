"""Synthetic designated-verifier proofs for the verify tests, built WITHOUT a prover: choose the discrete logs and solve the
verifier's equation (src/srs.rs:374-428) for them.

    P = p G,  alpha = H(enc(P), pub),  i0 = sum pub_j alpha^j,  pick b0 and a target t for u0:
    u0 = (a0 + delta b0 + delta^2 (a0 b0 - i0)) eps = t   =>   a0 = (t / eps - delta b0 + delta^2 i0) / (1 + delta^2 b0)
    v0 = (tau - alpha) eps,  K = ((p - t) / v0) G   =>   v0 K + u0 G = (p - t) G + t G = P.

The same construction reaches the exceptional cases of the addition chain (v0 K = +-u0 G, u0 = 0, v0 = 0, K = +-G, K = O, P = O).
Encodings and challenges come from callables so that the CPU tests use the oracle (pyref / c_oracle) and the GPU tests can build
tens of thousands of proofs with the library's batched multiplication; oracle_verdict is the reference's boolean, restated on the
C oracle's decode / k233_mul / k233_mulgen."""
import random

import c_oracle as co
import pyref as o

P = o.P
CASES = ("t_half", "p_zero", "u0_zero", "v0_zero", "k_plus_g", "k_minus_g", "k_zero")


def inv(x):
    return pow(x % P, P - 2, P)


def oracle_encode_many(dlogs, rule=0):
    out = []
    for k in dlogs:
        pt = co.k233_mulgen(k % P) if k % P else None
        out.append(co.xsk233_encode(pt) if rule == 0 else o.xsk233_encode(pt, rule))
    return out


def solve_a0(td, b0, t, i0):
    tau, delta, eps = td
    d2 = delta * delta % P
    den = (1 + d2 * b0) % P
    assert den, "b0 = -1/delta^2: pick another b0"
    return (t * inv(eps) - delta * b0 + d2 * i0) % P * inv(den) % P


def plan(td, pub, rng, case=None):
    """(p, b0, t) for one proof; the K discrete log follows from alpha (finish)."""
    p = rng.randrange(1, P)
    b0 = rng.randrange(P)
    t = rng.randrange(P)
    if case == "t_half":
        t = p * inv(2) % P  # v0 K = u0 G
    elif case == "p_zero":
        p = 0  # P = O, v0 K = -u0 G
    elif case == "u0_zero":
        t = 0
    elif case == "k_zero":
        t = p  # K = O
    return dict(p=p, b0=b0, t=t, case=case)


def finish(td, pub, pl, alpha):
    """the K discrete log, a0 and (for v0 = 0) the trapdoor this proof is to be checked against"""
    tau, delta, eps = td
    p, b0, t, case = pl["p"], pl["b0"], pl["t"], pl["case"]
    if case == "v0_zero":
        td = (alpha, delta, eps)  # tau = alpha after the proof exists: v0 = 0
        t = p
        k = (pl["b0"] ^ 0x5A5A5A) % P or 1  # any K
    v0 = (td[0] - alpha) * td[2] % P
    if case in ("k_plus_g", "k_minus_g"):
        t = (p - (v0 if case == "k_plus_g" else -v0)) % P
    if case != "v0_zero":
        k = (p - t) * inv(v0) % P if v0 else 0
    i0 = o.evaluate_monomial_basis_poly(pub, alpha)
    a0 = solve_a0(td, b0, t, i0)
    return dict(k=k, a0=a0, b0=b0, td=td, p=p, alpha=alpha)


def build(td, pubs, cases, seed=1, encode_many=oracle_encode_many, challenge=o.transcript_challenge):
    """one proof per (pub row, case): list of dicts with bytes, trapdoor, public inputs and discrete logs"""
    rng = random.Random(seed)
    plans = [plan(td, pub, rng, c) for pub, c in zip(pubs, cases)]
    enc_p = encode_many([pl["p"] for pl in plans])
    fins = [finish(td, pub, pl, challenge(e, pub)) for pub, pl, e in zip(pubs, plans, enc_p)]
    enc_k = encode_many([f["k"] for f in fins])
    out = []
    for pub, pl, f, ep, ek in zip(pubs, plans, fins, enc_p, enc_k):
        proof = ep + ek + f["a0"].to_bytes(29, "little") + f["b0"].to_bytes(29, "little")
        out.append(dict(proof=proof, td=f["td"], pub=list(pub), p=f["p"], k=f["k"], a0=f["a0"], b0=f["b0"], alpha=f["alpha"],
                        case=pl["case"]))
    return out


def tamper(case, kind, rng, other=None):
    """a rejected (or re-judged) variant of a valid case: returns (proof bytes, trapdoor, public inputs)"""
    b = bytearray(case["proof"])
    td, pub = case["td"], list(case["pub"])
    if kind.startswith("flip_"):
        lo, hi = dict(flip_commit=(0, 30), flip_kzg=(30, 60), flip_a0=(60, 89), flip_b0=(89, 118))[kind]
        pos = rng.randrange(lo * 8, hi * 8)
        b[pos // 8] ^= 1 << (pos % 8)
    elif kind == "a0_plus_1":
        b[60:89] = ((case["a0"] + 1) % P).to_bytes(29, "little")
    elif kind == "a0_ge_p":
        b[60:89] = (P + rng.randrange(0, 1 << 200)).to_bytes(29, "little")
    elif kind == "b0_ge_p":
        b[89:118] = (P + rng.randrange(0, 1 << 200)).to_bytes(29, "little")
    elif kind in ("bad_commit", "bad_kzg"):
        off = 0 if kind == "bad_commit" else 30
        while True:  # a 233-bit value that is no encoding
            w = rng.randrange(1, 1 << 233).to_bytes(30, "little")
            if not co.xsk233_decode(w)[1]:
                break
        b[off:off + 30] = w
    elif kind in ("spare_commit", "spare_kzg"):
        off = 29 if kind == "spare_commit" else 59
        b[off] |= 1 << rng.randrange(1, 8)
    elif kind == "wrong_public":
        if pub:
            pub[0] = (pub[0] + 1) % P
        else:
            pub = [1]
    elif kind == "swap":
        b[0:30], b[30:60] = case["proof"][30:60], case["proof"][0:30]
    elif kind == "wrong_trapdoor":
        td = ((td[0] + 1) % P, td[1], td[2])
    else:
        raise ValueError(kind)
    return bytes(b), td, pub


TAMPER = ("flip_commit", "flip_kzg", "flip_a0", "flip_b0", "a0_plus_1", "a0_ge_p", "b0_ge_p", "bad_commit", "bad_kzg", "spare_commit",
          "spare_kzg", "wrong_public", "swap", "wrong_trapdoor")


def oracle_verdict(td, pub, proof: bytes) -> bool:
    """SRS::verify, src/srs.rs:374-428, on the C oracle (codec rule 0): decode both points, FrBits validity, the transcript over the
    RE-ENCODED commitment (witness_commitment_hash), v0 K + u0 G == P"""
    tau, delta, eps = td
    pt_p, ok_p = co.xsk233_decode(proof[0:30])
    pt_k, ok_k = co.xsk233_decode(proof[30:60])
    a0, b0 = int.from_bytes(proof[60:89], "little"), int.from_bytes(proof[89:118], "little")
    ok_a, ok_b = a0 < P, b0 < P
    a0, b0 = (a0 if ok_a else 0), (b0 if ok_b else 0)
    enc_p = co.xsk233_encode(pt_p) if ok_p else bytes(30)
    alpha = o.transcript_challenge(enc_p, pub)
    i0 = o.evaluate_monomial_basis_poly(pub, alpha)
    r0 = (a0 * b0 - i0) % P
    u0 = (a0 + delta * b0 + delta * delta % P * r0) % P * eps % P
    v0 = (tau - alpha) * eps % P
    lhs = o.k233_add(co.k233_mul(v0, pt_k) if (ok_k and v0) else None, co.k233_mulgen(u0) if u0 else None)
    return (lhs == (pt_p if ok_p else None)) and ok_p and ok_k and ok_a and ok_b
