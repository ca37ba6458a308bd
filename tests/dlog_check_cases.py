"""dvp_points_check_dlog restated in plain Python (include/dvpari.h states the derivation), and the cases its tests share.

    h   = BLAKE3(xy bytes || infinity bytes)           the points as given; no infinity mask hashes as n zero bytes
    key = seed, or BLAKE3("dv-pari dlog check v1")
    k   = BLAKE3(key || h)
    r_i = (first 16 bytes of BLAKE3(k || LE64(i)), little-endian) | 2^127

The combined check asks whether sum_i r_i (P_i - s_i G) is O.  On discrete logs, with P_i = t_i G, that is
sum_i r_i (t_i - s_i) == 0 mod p: combined_sum below.  BLAKE3 is pyref's, written from the specification.  Nothing here touches a
device."""
import random

import numpy as np

import pyref as o

TAG = b"dv-pari dlog check v1"
SRS_TAG = b"dv-pari srs check v1"
BLOCK_LENGTHS = (1, 2, 255, 256, 257)  # one lane, two, a block less one, a block, a block and one lane


def points_hash(xy, inf=None) -> bytes:
    xy = np.ascontiguousarray(xy, dtype="<u8").reshape(-1, 8)
    n = xy.shape[0]
    tail = bytes(n) if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).reshape(n).tobytes()
    return o.blake3(xy.tobytes() + tail)


def coefficients(h: bytes, n: int, seed=None):
    key = o.blake3(TAG) if seed is None else bytes(seed)
    assert len(key) == 32 and len(h) == 32
    k = o.blake3(key + h)
    return [int.from_bytes(o.blake3(k + i.to_bytes(8, "little"))[:16], "little") | (1 << 127) for i in range(n)]


def srs_key(trapdoor, v: int, seed=None) -> bytes:
    """the key dvp_srs_check_cache_dir checks vector v under"""
    head = SRS_TAG + b"".join(int(x).to_bytes(32, "little") for x in trapdoor) if seed is None else bytes(seed)
    return o.blake3(head + v.to_bytes(4, "little"))


def combined_sum(r, s, t) -> int:
    """sum r_i (t_i - s_i) mod p for the claimed logs s and the points' logs t"""
    return sum(ri * (ti - si) for ri, si, ti in zip(r, s, t)) % o.P


def fr_sum_constants():
    """(lanes, blocks) of the two-level block sums, read from csrc/fr_block.cuh"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dv-pari_amd", "csrc", "fr_block.cuh")).read()
    lanes = int(re.search(r"constexpr uint32_t FR_SUM_LANES = (\d+);", src).group(1))
    blocks = int(re.search(r"constexpr uint32_t FR_SUM_BLOCKS = (\d+);", src).group(1))
    return lanes, blocks


def tampers(n: int, seed: int):
    """[(name, {index: what is added to that point's discrete log}, first wrong index)] for a vector of n entries"""
    rnd = random.Random(seed)
    t = rnd.randrange(1, o.P)
    out = [("first", {0: 1}, 0), ("last", {n - 1: 1}, n - 1)]
    if n >= 3:
        out.append(("middle", {n // 2: 1}, n // 2))
    if n >= 2:
        i, j = sorted(rnd.sample(range(n), 2))
        out.append(("pair", {i: t, j: o.P - t}, i))  # compensating: the unweighted sum of the logs does not move
        a, b = sorted(rnd.sample(range(n), 2))
        out.append(("two", {a: rnd.randrange(1, o.P), b: rnd.randrange(1, o.P)}, a))
    return out


def apply_tamper(logs, delta):
    out = list(logs)
    for i, d in delta.items():
        out[i] = (out[i] + d) % o.P
    return out
