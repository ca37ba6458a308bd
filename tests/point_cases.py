"""Affine points of every class dvp_points_check names, with the class each must get BY DEFINITION -- never by the trace shortcut
the kernel uses:
    on the curve   pyref.k233_on_curve (the curve equation)
    in E[r]        r P = O by double-and-add (pyref.k233_in_prime_subgroup)
    COSET_N        P + N in E[r], N = (0,1)
    ORDER4         on the curve and neither of the two
The generator is deterministic.  A big-int scalar multiplication of pyref takes seconds, so the list and its classes by pyref's
definition are RECORDED in tests/golden/point_cases.json (`python tests/point_cases.py` rewrites it, minutes); the tests load
the record, and tests/test_points_check_cpu.py regenerates the list and re-derives every class from the definition with the C
oracle's integer double-and-add (c_oracle.k233_mul(.., frob=False)), and one with pyref itself."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyref as o  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "point_cases.json")
OK, UNREDUCED, OFF_CURVE, ORDER4, COSET_N = 0, 0x01, 0x02, 0x04, 0x08
CLASS_NAMES = {OK: "ok", UNREDUCED: "UNREDUCED", OFF_CURVE: "OFF_CURVE", ORDER4: "ORDER4", COSET_N: "COSET_N"}
G_MULTIPLES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 255, 256, 1000, 4095, 17, 63, 64, 65, 127, 1 << 20, (1 << 64) - 1, 1 << 64, 1 << 128, 1 << 230, o.P - 1, o.P - 2, (o.P + 1) // 2, 0xC0FFEE1234567 * 0xDEADBEEF987654321 % o.P]
N_RANDOM_X = 76


def pyref_mul(k, pt):
    return o.k233_mul(k, pt)


def class_by_definition(x: int, y: int, inf: int, mul=pyref_mul) -> int:
    """the class of one point from the definitions alone; mul(k, pt) = a scalar multiplication valid on the whole curve"""
    if inf:
        return OK
    if (x >> 233) or (y >> 233):
        return UNREDUCED
    if not o.k233_on_curve((x, y)):
        return OFF_CURVE
    if mul(o.K233_ORDER, (x, y)) is None:
        return OK
    pn = o.k233_add((x, y), o.N_STD)
    if pn is None or mul(o.K233_ORDER, pn) is None:
        return COSET_N
    return ORDER4


def class_by_trace(x: int, y: int, inf: int) -> int:
    """the same partition the way the kernel takes it: two trace tests and one half (pyref.k233_in_prime_subgroup_fast's route)"""
    if inf:
        return OK
    if (x >> 233) or (y >> 233):
        return UNREDUCED
    if not o.k233_on_curve((x, y)):
        return OFF_CURVE
    if x == 0:
        return COSET_N
    if o.gf_trace(x):
        return ORDER4
    return OK if o.k233_in_prime_subgroup_fast((x, y)) else COSET_N


def _random_curve_point(rng):
    """a curve point over a random x: y = x z with z^2 + z = x + 1 / x^2 (half of all x have one)"""
    while True:
        x = rng.getrandbits(233)
        if x == 0:
            continue
        z = o.gf_solve_quadratic(x ^ o.gf_sqr(o.gf_inv(x)))
        if z is None:
            continue
        y = o.gf_mul(z ^ rng.getrandbits(1), x)
        assert o.k233_on_curve((x, y))
        return x, y


def generate(mul=pyref_mul):
    """[(label, x, y, inf)]: about 200 points; mul is used for the multiples of G only"""
    rng = random.Random(233)
    out = []
    mults = [mul(k, o.G_STD) for k in G_MULTIPLES]
    for k, p in zip(G_MULTIPLES, mults):
        out.append((f"{k % 10**6}G", p[0], p[1], 0))
    for k, p in zip(G_MULTIPLES, mults):
        q = o.k233_add(p, o.N_STD)
        out.append((f"{k % 10**6}G+N", q[0], q[1], 0))
    for j in range(N_RANDOM_X):
        x, y = _random_curve_point(rng)
        out.append((f"random_x_{j}", x, y, 0))
    out.append(("N", 0, 1, 0))
    out.append(("(0,0)", 0, 0, 0))
    for j in range(8):
        out.append((f"(0,y!=1)_{j}", 0, [2, 3, 1 << 232, (1 << 233) - 1][j] if j < 4 else rng.getrandbits(233) | 2, 0))
    for j in range(10):
        x, y = mults[j]
        out.append((f"y_bit_flipped_{j}", x, y ^ (1 << [0, 1, 31, 32, 63, 64, 127, 200, 231, 232][j]), 0))
    for j, bit in enumerate((233, 255, 224 + 31)):  # bit 233, bit 255, the top bit of 32-bit word 7 (= bit 255 again, by its other name)
        for c in range(2):
            x, y = mults[3 + 2 * j + c]
            out.append((f"x_bit_{bit}_{c}", x | (1 << bit), y, 0))
            out.append((f"y_bit_{bit}_{c}", x, y | (1 << bit), 0))
    for j in range(3):  # further spare bits, and both coordinates at once
        x, y = mults[9 + j]
        out.append((f"xy_spare_bits_{j}", x | (1 << (234 + 7 * j)), y | (1 << (254 - 5 * j)), 0))
    for j in range(8):
        x, y = mults[j]
        out.append((f"valid_inf_{j}", x, y, 1))
    for j in range(10):
        bits = 256 if j % 2 else 233
        out.append((f"garbage_inf_{j}", rng.getrandbits(bits) | ((1 << 255) if j % 2 else 0), rng.getrandbits(bits), 1 + 254 * (j % 3 == 0)))
    return out


def _definition_classes(points, procs=8):
    from multiprocessing import Pool

    with Pool(procs) as pool:
        return pool.starmap(class_by_definition, [(x, y, inf) for _, x, y, inf in points])


def load():
    """the recorded list: [dict(label, x, y, inf, cls)]"""
    rec = json.load(open(GOLDEN))
    return [dict(label=r["label"], x=int(r["x"], 16), y=int(r["y"], 16), inf=r["inf"], cls=r["cls"]) for r in rec["points"]]


def arrays(cases):
    """(xy uint64 [n, 8], inf uint8 [n], expected uint8 [n]) of a list of cases"""
    import numpy as np

    xy = np.frombuffer(b"".join(c["x"].to_bytes(32, "little") + c["y"].to_bytes(32, "little") for c in cases), dtype="<u8").reshape(-1, 8).copy()
    inf = np.array([c["inf"] for c in cases], dtype=np.uint8)
    cls = np.array([c["cls"] for c in cases], dtype=np.uint8)
    return xy, inf, cls


if __name__ == "__main__":
    pts = generate()
    cls = _definition_classes(pts)
    rec = dict(note="tests/point_cases.py: generate() and class_by_definition() with pyref's own double-and-add",
               points=[dict(label=l, x=hex(x), y=hex(y), inf=inf, cls=c) for (l, x, y, inf), c in zip(pts, cls)])
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
    hist = {CLASS_NAMES[k]: cls.count(k) for k in CLASS_NAMES}
    print(len(pts), "points", hist)
