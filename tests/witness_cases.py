"""The value list of the witness-wire tests (tests/test_witness_wire_cpu.py, tests/test_gpu_witness_wire.py): 256-bit integers at
every boundary of the reduction x -> x mod p that csrc/fr_wire.cuh performs (p = 2^231 + c; the quotient x >> 231 runs up to 2^25 - 1,
the largest multiple of p below 2^256 is 33554431 p), then 4096 seeded random ones.  The expected values are Python's x % P."""
import random

P = 3450873173395281893717377931138512760570940988862252126328087024741343
BN254_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # the field a gnark witness is written in
K_MAX = (2**256 - 1) // P
assert K_MAX == 33554431 and P >> 231 == 1


def values():
    v = [0, 1, P - 1, P, P + 1, 2**231 - 1, 2**231, 2**232 - 1, 2**232, 2**256 - 1, BN254_R - 1]
    for k in (1, 2, 3, 2**10, 2**24 - 1, 2**24, K_MAX):
        for d in (-1, 0, 1):
            if k * P + d < 2**256:
                v.append(k * P + d)
    rnd = random.Random(0x5EED0BE32)
    v += [rnd.getrandbits(256) for _ in range(4096)]
    assert all(0 <= x < 2**256 for x in v)
    return v


VALUES = values()
EXPECTED = [x % P for x in VALUES]


def be32(vals) -> bytes:
    """the file's element encoding: 32 bytes big-endian each"""
    return b"".join(int(x).to_bytes(32, "big") for x in vals)


def witness_file_bytes(vals) -> bytes:
    """u32-BE count || count x 32 bytes big-endian (src/gnark_r1cs.rs:58-77,188-198), values written as they are (not reduced)"""
    return len(vals).to_bytes(4, "big") + be32(vals)
