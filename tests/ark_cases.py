"""The value list of the arkworks-form tests (tests/test_fr_ark_cpu.py, tests/test_gpu_fr_ark.py).  Everything here is Python integers:

    from_ark(x) = (x % P) * 2^-256 % P        to_ark(a) = (a % P) * 2^256 % P

for any 256-bit x, a (csrc/fr_ark.cuh: a reduction mod p, then one Montgomery product by a constant).  The values sit at the
boundaries of both steps: the reduction's (witness_cases.VALUES, around p, 2^231, 2^232, 2^256), every 32-bit limb boundary, and the
preimages under both maps of 0, 1 and p - 1, which put the product's result on either side of its last conditional subtraction."""
import random

import witness_cases as wc

P = wc.P
R = 2**256 % P  # arkworks' one
R_INV = pow(2, -256, P)


def from_ark(x: int) -> int:
    return (x % P) * R_INV % P


def to_ark(a: int) -> int:
    return (a % P) * 2**256 % P


def values():
    v = list(wc.VALUES)
    v += [0, 1, R, R * R % P, P - 1, P, P + 1, 2 * P - 1, 2**231 - 1, 2**231 + 1, 2**232 - 1, 2**232 + 1, 2**256 - 1]
    for k in range(1, 8):
        v += [2**(32 * k) - 1, 2**(32 * k)]
    for y in (0, 1, P - 1):
        v += [to_ark(y), from_ark(y)]  # from_ark(to_ark(y)) = y and to_ark(from_ark(y)) = y: the preimages under both maps
    rnd = random.Random(0xA4C)
    v += [rnd.randrange(P) for _ in range(200)]
    v += [rnd.getrandbits(256) for _ in range(56)]
    assert all(0 <= x < 2**256 for x in v)
    return v


VALUES = values()
FROM_ARK = [from_ark(x) for x in VALUES]
TO_ARK = [to_ark(x) for x in VALUES]
assert from_ark(R) == 1 and to_ark(1) == R and all(from_ark(to_ark(x)) == x % P == to_ark(from_ark(x)) for x in VALUES[-300:])


def limbs_bytes(ints) -> bytes:
    """32 bytes little-endian each: four LE u64, the memory of a [u64; 4]"""
    return b"".join(int(x).to_bytes(32, "little") for x in ints)
