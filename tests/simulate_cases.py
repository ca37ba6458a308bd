"""Plain-Python restatement of dvp_simulate_batch (include/dvpari.h) and of the fields of dvp_verify_trace, for the tests of
csrc/simulate.hip.  simulate() is verify_cases.build made deterministic: the scalars are drawn from BLAKE3(key || LE64(index) || tag)
instead of a random.Random, the cases are the DVP_SIM_* bytes, and v0 = 0 is a status instead of a change of trapdoor.  Encodings and
challenges come from callables as there: the CPU tests pass the oracle's, the GPU tests dvp_mulgen_batch and
proving.transcript_challenge.  trace_expect() computes the trace's points from discrete logs."""
import pyref as o
import verify_cases as vc

P = o.P
GENERIC, T_HALF, P_ZERO, U0_ZERO, K_PLUS_G, K_MINUS_G, K_ZERO = range(7)
CASES = (GENERIC, T_HALF, P_ZERO, U0_ZERO, K_PLUS_G, K_MINUS_G, K_ZERO)
OK, V0_ZERO = 0x00, 0x01
KEY_TAG = b"dv-pari simulate v1"


def default_key(td) -> bytes:
    return o.blake3(KEY_TAG + b"".join(int(x).to_bytes(32, "little") for x in td))


def draw(key: bytes, index: int, tag: int) -> int:
    h = o.blake3(key + (index % (1 << 64)).to_bytes(8, "little") + bytes([tag]))
    return int.from_bytes(h[:29], "little") & ((1 << 230) - 1)


def simulate(td, pubs, seed=None, index_base=0, cases=None, b0=None, encode_many=vc.oracle_encode_many, challenge=o.transcript_challenge):
    """one dict per row of pubs: proof (118 bytes), status, the discrete logs p and k, and t, a0, b0, alpha, v0 for the trace;
    status != 0: proof = 118 zero bytes, p = k = 0"""
    tau, delta, eps = td
    assert eps % P
    key = seed if seed is not None else default_key(td)
    n = len(pubs)
    cases = [GENERIC] * n if cases is None else list(cases)
    pre = []
    for j in range(n):
        p = draw(key, index_base + j, 1) or 1
        bj = draw(key, index_base + j, 2) if b0 is None else b0[j]
        t = draw(key, index_base + j, 3)
        if cases[j] == P_ZERO:
            p = 0
        if cases[j] == T_HALF:
            t = p * vc.inv(2) % P
        if cases[j] == U0_ZERO:
            t = 0
        if cases[j] == K_ZERO:
            t = p
        pre.append((p, bj, t))
    enc_p = encode_many([p for p, _, _ in pre])
    mid = []
    for j, (p, bj, t) in enumerate(pre):
        alpha = challenge(enc_p[j], pubs[j])
        v0 = (tau - alpha) * eps % P
        if v0 == 0:
            mid.append(None)
            continue
        if cases[j] == K_PLUS_G:
            t = (p - v0) % P
        if cases[j] == K_MINUS_G:
            t = (p + v0) % P
        k = (p - t) * vc.inv(v0) % P
        i0 = o.evaluate_monomial_basis_poly(pubs[j], alpha)
        d2 = delta * delta % P
        if (1 + d2 * bj) % P == 0:
            bj = (bj + 1) % P
        a0 = (t * vc.inv(eps) - delta * bj + d2 * i0) % P * vc.inv(1 + d2 * bj) % P
        mid.append(dict(p=p, k=k, t=t, a0=a0, b0=bj, alpha=alpha, v0=v0, i0=i0))
    enc_k = encode_many([m["k"] if m else 0 for m in mid])
    out = []
    for j, m in enumerate(mid):
        if m is None:
            out.append(dict(proof=bytes(118), status=V0_ZERO, p=0, k=0, pub=list(pubs[j]), case=cases[j]))
        else:
            proof = enc_p[j] + enc_k[j] + m["a0"].to_bytes(29, "little") + m["b0"].to_bytes(29, "little")
            out.append(dict(m, proof=proof, status=OK, pub=list(pubs[j]), case=cases[j]))
    return out


def trace_scalars(td, pub, proof: bytes, alpha: int):
    """alpha -> (i0, r0, u0, v0) as SRS::verify computes them from the proof's a0, b0 (src/srs.rs:411-417)"""
    tau, delta, eps = td
    a0, b0 = int.from_bytes(proof[60:89], "little"), int.from_bytes(proof[89:118], "little")
    i0 = o.evaluate_monomial_basis_poly(pub, alpha)
    r0 = (a0 * b0 - i0) % P
    u0 = (a0 + delta * b0 + delta * delta % P * r0) % P * eps % P
    v0 = (tau - alpha) * eps % P
    return i0, r0, u0, v0


def trace_dlogs(k: int, u0: int, v0: int):
    """the discrete logs of the trace's three points for a proof whose K = k G: vk = (v0 k) G, ug = u0 G, sum = (v0 k + u0) G"""
    vk = v0 * k % P
    return vk, u0 % P, (vk + u0) % P
