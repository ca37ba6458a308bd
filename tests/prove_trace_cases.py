"""Restatements for the prove trace and the Fr-vector digest, from the reference's formats and the oracle alone (never from the library):
the byte stream of Vec<Fr>::serialize_uncompressed, the lengths at which the packer and the hash tree change shape, and the record
dvp_prover_trace_last must deliver for a proof the oracle has restated (pyref.prove_scalars)."""
import functools
import random

import pyref as o
import c_oracle as co

P = o.P
R_MONT = 1 << 232  # the library's Montgomery radix (csrc/fr.cuh)

# n -> what it exercises (stream bytes = 8 + 29 n)
LENGTHS = {
    0: "count bytes only (8)",
    1: "single short block (37)",
    2: "two blocks (66)",
    24: "11 full blocks (704)",
    35: "one chunk, one byte short (1023)",
    36: "second chunk of 28 B (1052)",
    600: "exactly 17 chunks (17408), odd count",
    601: "18 chunks, 29 B in the last (17437)",
}


def fr_stream(vals) -> bytes:
    """Vec<Fr>::serialize_uncompressed: the count as u64 LE, then 29 bytes LE per entry (its low 232 bits)"""
    return len(vals).to_bytes(8, "little") + b"".join((int(v) & ((1 << 232) - 1)).to_bytes(29, "little") for v in vals)


def chunks_of(n: int) -> int:
    return max(1, -(-(8 + 29 * n) // 1024))


def length_for_chunks(k: int) -> int:
    """the largest n whose stream has exactly k chunks"""
    n = (1024 * k - 8) // 29
    assert chunks_of(n) == k
    return n


@functools.lru_cache(maxsize=None)
def values(n: int, seed: int = 0):
    rnd = random.Random(1000 * seed + n)
    v = [rnd.randrange(P) for _ in range(n)]
    for k, edge in enumerate((0, 1, P - 1, (1 << 231) - 1, 1 << 231)):  # < p: p = 2^231 + ...
        if k < n:
            v[(7 * k + 3) % n] = edge
    return tuple(v)


@functools.lru_cache(maxsize=None)
def digest_of_values(n: int, seed: int = 0) -> bytes:
    return o.blake3(fr_stream(values(n, seed)))


def digest(vals) -> bytes:
    return o.blake3(fr_stream(vals))


def to_mont(vals):
    return [v * R_MONT % P for v in vals]


# ---- the record of a restated proof ------------------------------------------------------------------------------------------
DIGEST_NAMES = ("assignment", "evals.a", "evals.b", "evals.c", "evals.i", "evals2.a", "evals2.b", "evals2.c", "evals2.i", "r_vals2", "q_vals2",
                "denom_invs", "denom_invs2", "k_scalar_a", "k_scalar_b", "k_scalar_r")
SCALAR_NAMES = ("alpha", "z_alpha", "a0", "b0", "i0", "r0")
POINT_NAMES = ("msm_gm", "msm_q", "commit_p", "kzg_a", "kzg_b", "kzg_r", "kzg_k")


def dot(a, b):
    assert len(a) == len(b)
    return sum(x * y for x, y in zip(a, b)) % P


def expected_scalars(pr):
    return {k: pr[k] for k in SCALAR_NAMES}


def expected_vectors(pr, tables, n_wires):
    """the sixteen vectors under src/proving.rs's names; denom_invs / denom_invs2 as pyref.prove_scalars computes its dinv / dinv2"""
    d, d2, alpha = tables["D"], tables["D2"], pr["alpha"]
    dinv = o.fr_batch_inverse([(x - alpha) % P for x in d])
    dinv2 = o.fr_batch_inverse([(x - alpha) % P for x in d2])
    w = list(pr["w"]) + [0] * (n_wires - len(pr["w"]))
    return {"assignment": w, "evals.a": pr["a"], "evals.b": pr["b"], "evals.c": pr["c"], "evals.i": pr["i"], "evals2.a": pr["a2"],
            "evals2.b": pr["b2"], "evals2.c": pr["c2"], "evals2.i": pr["i2"], "r_vals2": pr["r2"], "q_vals2": pr["q2"], "denom_invs": dinv,
            "denom_invs2": dinv2, "k_scalar_a": pr["ka"], "k_scalar_b": pr["kb"], "k_scalar_r": pr["kr"]}


def expected_dlogs(pr, setup):
    """the discrete log of every point of the record, summed from the oracle's vectors and the setup's base scalars"""
    g_m = list(setup["g_m"])
    dl = {"msm_gm": dot(pr["w"][:len(g_m)], g_m[:len(pr["w"])]), "msm_q": dot(pr["q2"], setup["g_q"]), "kzg_a": dot(pr["ka"], setup["g_k"][0]),
          "kzg_b": dot(pr["kb"], setup["g_k"][1]), "kzg_r": dot(pr["kr"], setup["g_k"][2])}
    dl["commit_p"] = (dl["msm_gm"] + dl["msm_q"]) % P
    dl["kzg_k"] = (dl["kzg_a"] + dl["kzg_b"] + dl["kzg_r"]) % P
    assert dl["commit_p"] == pr["dl_commit_p"] and dl["kzg_k"] == pr["dl_kzg"]
    return dl


def expected_point(dl: int):
    """dl G by the C oracle, as the record holds a point"""
    pt = co.k233_mulgen(dl)
    if pt is None:
        return {"x": 0, "y": 0, "inf": 1, "enc": co.xsk233_encode(None)}
    return {"x": pt[0], "y": pt[1], "inf": 0, "enc": co.xsk233_encode(pt)}


def sample_record():
    """a record with every field distinct, for the text round trip (no proof behind it)"""
    rnd = random.Random(5)
    rec = {"log2_m": 8, "n_wires": 771, "n_public": 2, "codec_rule": 0, "parts": 7, "mismatch": 2}
    for f in SCALAR_NAMES:
        rec[f] = rnd.randrange(P)
    for k, f in enumerate(POINT_NAMES):
        rec[f] = {"x": rnd.randrange(1 << 233), "y": rnd.randrange(1 << 233), "inf": k & 1, "enc": bytes(rnd.randrange(256) for _ in range(30))}
    for f in DIGEST_NAMES:
        rec[f] = bytes(rnd.randrange(256) for _ in range(32))
    return rec
