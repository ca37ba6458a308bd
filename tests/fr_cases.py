"""Case sets and the exact integer reference for the Fr arithmetic of dv-pari_amd/csrc/fr.cuh (dvp_debug_fr_op, one function per
element).  Python integers only; no code is shared with the library.

Random operands exercise a carry boundary of these functions about once in 2^29 .. 2^116 tries, so the operands here are CHOSEN:
powers of two and p minus powers of two with their neighbours, all-ones limbs at the three limb widths (29, 30, 32 bits), the
Montgomery constants, long-Euclid inputs for the GCD inversion, values that agree with p in more than 100 top bits, and operand pairs
constructed so that the value before the final conditional subtraction lands next to p.  classify() names the branch a case takes
ON THE REFERENCE ALONE, so a test can assert that the set reaches every branch without consulting the code under test."""
import functools
import random

P = (1 << 231) + 0x69D5BB915BCD46EFB1AD5F173ABDF
R_BITS, R30_BITS = 232, 240
R, R30 = 1 << R_BITS, 1 << R30_BITS
R_INV = pow(R, -1, P)
_NEG_P_INV = {R_BITS: (-pow(P, -1, R)) % R, R30_BITS: (-pow(P, -1, R30)) % R30}
M256 = (1 << 256) - 1


def pack(vals) -> bytes:
    return b"".join([v.to_bytes(32, "little") for v in vals])


def unpack(buf: bytes) -> list:
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


# ---- values ---------------------------------------------------------------------------------------------------------------------
def _fib_ratios():
    out, a, b = [], 1, 2
    k = 0
    while b < (P << 4):
        if k % 8 == 0:
            out.append(P * a // b)  # p F_k / F_(k+1): the quotients of Euclid on (p, this) are all 1 for ~k steps
        a, b = b, a + b
        k += 1
    return out


@functools.lru_cache(None)
def edge_values() -> tuple:
    """about 1.5 k canonical values (< p), sorted"""
    v = {0, 1, 2, 3, P - 1, P - 2, P - 3, (P + 1) // 2, (P - 1) // 2, P // 3}
    for rad in (R, R30):
        v |= {rad % P, rad * rad % P, rad ** 3 % P, pow(rad, -1, P)}
    for k in range(232):
        for d in (-1, 0, 1):
            v |= {(1 << k) + d, P - (1 << k) + d}
    for w in (29, 30, 32):  # all-ones limbs, one at a time, all but one, all together; clipped below p
        ones = (1 << w) - 1
        full = (1 << 232) - 1
        for i in range(8):
            v |= {(ones << (w * i)) & full, full & ~(ones << (w * i))}
        v.add(full)
    v |= {P >> k for k in (1, 2, 3, 7, 8, 9, 28, 29, 30, 31, 32, 33, 58, 59, 60, 61, 62, 115, 116, 117, 200, 229, 230, 231)}
    v |= set(_fib_ratios())
    # c 2^k, c small and odd: the binary GCD halves a for k steps, swaps, and then wears p down against b = c one bit per step, so
    # b reaches 1 only in the last of its 16 rounds of 30 steps (gcd_steps)
    v |= {c << k for c in (3, 5, 7, 9, 11) for k in range(214, 230) if c << k < P}
    rnd = random.Random(2330)
    for x in [P - 1, P // 3, R % P] + [rnd.randrange(P) for _ in range(8)]:  # low 30 bits all zero / all one
        v |= {(x >> 30) << 30, x | 0x3FFFFFFF}
    out = set()
    for x in v:
        if x >= P:
            x &= (1 << 231) - 1  # clip: drop bit 231 and above
        if 0 <= x < P:
            out.add(x)
    return tuple(sorted(out))


@functools.lru_cache(None)
def key_values() -> tuple:
    """the partners every edge value meets"""
    return (0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, R % P, R * R % P, R30 % P, pow(R, -1, P), (1 << 231) - 1, 1 << 231,
            (1 << 231) + 1, P - (1 << 230), (1 << 29) - 1, 1 << 29, (1 << 30) - 1, 1 << 30, (1 << 32) - 1, 1 << 32, (1 << 116) - 1,
            1 << 116, P // 3)


@functools.lru_cache(None)
def pairs() -> tuple:
    """every edge value with the key values, 16 other edge values and itself; near-p pairs; pairs whose Montgomery product lands
    next to p before the conditional subtraction"""
    e = edge_values()
    rnd = random.Random(29)
    out = []
    for a in e:
        out += [(a, b) for b in key_values()]
        out += [(a, e[rnd.randrange(len(e))]) for _ in range(16)]
        out.append((a, a))
    out += [(P - 1 - rnd.randrange(1 << 20), P - 1 - rnd.randrange(1 << 20)) for _ in range(4096)]
    for a in [rnd.randrange(1, P) for _ in range(48)] + [e[rnd.randrange(1, len(e))] for _ in range(48)]:
        for t in (1, 2, P - 1, P - 2):
            out.append((a, t * R * pow(a, -1, P) % P))  # a b / R = t (mod p)
    out += [(a, P - a) for a in e[1:200]] + [(a, P - a - 1) for a in e[:100]] + [(a, P - a + 1) for a in e[2:100]]  # sums around p
    return tuple(out)


@functools.lru_cache(None)
def triples() -> tuple:
    """(a, b, c) for a b / R + c: the pairs with an addend that walks the key values, and near-p operands with c = p - 1 - j"""
    rnd = random.Random(31)
    k = key_values()
    out = [(a, b, k[i % len(k)]) for i, (a, b) in enumerate(pairs()[::2])]
    out += [(P - 1 - rnd.randrange(1 << 20), P - 1 - rnd.randrange(1 << 20), P - 1 - (rnd.randrange(1 << 20) if i % 2 else 0))
            for i in range(8192)]
    out += [(rnd.randrange(1 << 200), rnd.randrange(1 << 200), rnd.randrange(1 << 100)) for _ in range(64)]
    return tuple(out)


@functools.lru_cache(None)
def quads() -> tuple:
    """(a0, b0, a1, b1) for the fused two-term product"""
    rnd = random.Random(37)
    p = pairs()
    out = [p[i] + p[(i * 7 + 3) % len(p)] for i in range(0, len(p), 2)]
    out += [tuple(P - 1 - rnd.randrange(1 << 20) for _ in range(4)) for _ in range(8192)]
    out += [(P - 1,) * 4, (0,) * 4, (1, 1, 1, 1), (P - 1, 1, 1, P - 1), (P - 1, P - 1, 0, 0)]
    return tuple(out)


@functools.lru_cache(None)
def lazy_values() -> tuple:
    """k p + e, the shape of a value inside an extend (congruent to e, a few dozen p large); all below 192 p < 2^239"""
    e = edge_values()
    rnd = random.Random(41)
    es = [0, 1, P - 1, P - 2, (P - 1) // 2, (1 << 231) - 1, 1 << 231, (1 << 30) - 1, 1 << 30, (1 << 210) - 1, 1 << 210]
    es += [e[rnd.randrange(len(e))] for _ in range(24)]
    out = {k * P + x for k in (0, 1, 2, 31, 63, 127, 191) for x in es}
    out |= {(1 << 238) - 1, 64 * P - 1, 192 * P - 1, 128 * P - 1, 1 << 238, (1 << 238) + 1}
    return tuple(sorted(out))


@functools.lru_cache(None)
def lazy_pairs() -> tuple:
    """(e0, e1) for e0 - e1 + 128 p: e0 < 2^239, e1 < 128 p"""
    lz = lazy_values()
    e1s = [x for x in lz if x < 128 * P]
    rnd = random.Random(43)
    out = [(a, b) for a in lz for b in e1s[::3]] + [(a, a) for a in e1s]
    out += [((1 << 239) - 1, b) for b in e1s] + [(0, b) for b in e1s] + [(a, 128 * P - 1) for a in lz] + [(a, 0) for a in lz]
    # every 30-bit limb of e0 at 0 against an all-ones limb of e1, and the other way round: the lent 2^30 is what covers it
    ones = (1 << 30) - 1
    for i in range(8):
        lo = ones << (30 * i) if i < 7 else (127 * P >> 210) << 210
        out += [(0, lo), (lo, 0), ((1 << 239) - 1 - lo, lo), (lo, lo), (1 << (30 * i), lo)]
    out += [(rnd.randrange(1 << 239), rnd.randrange(128 * P)) for _ in range(2048)]
    return tuple(out)


@functools.lru_cache(None)
def lazy_triples() -> tuple:
    """(a, b, c): a constant below p times a lazy b, plus a lazy c; the exact result stays below 2 p + 192 p < 2^240.  Operands near
    2^240 ride along where the result allows them (b up to 2^240 - 1 with a small c, c up to 2^240 - 2 p - 1)."""
    e = edge_values()
    lz = lazy_values()
    rnd = random.Random(47)
    out = []
    for a in e:
        out += [(a, lz[rnd.randrange(len(lz))], lz[rnd.randrange(len(lz))]) for _ in range(18)]
        out += [(a, R30 - 1, 0), (a, (1 << 239) + rnd.randrange(1 << 239), rnd.randrange(1 << 238))]
    top_c = R30 - 2 * P - 1
    out += [(P - 1, R30 - 1, top_c), (P - 1, P - 1, top_c), (1, 1, top_c), (0, 0, top_c), (0, 0, R30 - 1), (1, R30 - 1, R30 - 1 - P - 1)]
    out += [(rnd.randrange(P), rnd.randrange(R30), rnd.randrange(R30 - 2 * P)) for _ in range(2048)]
    return tuple(out)


@functools.lru_cache(None)
def below_2p() -> tuple:
    e = edge_values()
    return tuple(e) + tuple(P + x for x in e)


@functools.lru_cache(None)
def any_256() -> tuple:
    rnd = random.Random(53)
    out = list(below_2p()) + [2 * P, 2 * P + 1, M256, 1 << 255, (1 << 255) - 1, 1 << 232, (1 << 232) - 1, 1 << 233]
    for i in range(8):  # equal to p above 32-bit limb i, below / above it there
        hi = (P >> (32 * i)) << (32 * i)
        out += [hi, hi - 1, hi + (1 << (32 * i)), (hi + (1 << (32 * i)) - 1) & M256]
        out += [P ^ (1 << (32 * i)), (P + (1 << (32 * i + 31))) & M256, P | (0xFFFFFFFF << (32 * i))]
    out += [rnd.randrange(1 << 256) for _ in range(256)]
    return tuple(out)


@functools.lru_cache(None)
def below_2_232() -> tuple:
    e = edge_values()
    full = (1 << 232) - 1
    out = list(e) + [x | (1 << 231) for x in e[::3]] + [full, full - 1, 1 << 231, P, P + 1]
    for w in (29, 30, 32):
        out += [((1 << w) - 1) << (w * i) & full for i in range(8)] + [full & ~(((1 << w) - 1) << (w * i)) for i in range(8)]
    out += [(1 << k) - 1 for k in range(1, 233)] + [1 << k for k in range(232)]
    return tuple(out)


@functools.lru_cache(None)
def below_2_240() -> tuple:
    full = (1 << 240) - 1
    out = list(lazy_values()) + list(below_2_232()[::2]) + [full, full - 1, 1 << 239, (1 << 239) - 1, (1 << 239) + 1]
    for w in (29, 30, 32):
        out += [((1 << w) - 1) << (w * i) & full for i in range(9)] + [full & ~(((1 << w) - 1) << (w * i)) for i in range(9)]
    out += [(1 << k) - 1 for k in range(232, 241)] + [1 << k for k in range(232, 240)] + [x | (1 << 239) for x in lazy_values()[::4]]
    return tuple(out)


@functools.lru_cache(None)
def inversion_inputs() -> tuple:
    """every edge value and 2^17 random ones"""
    rnd = random.Random(59)
    return edge_values() + tuple(rnd.randrange(P) for _ in range(1 << 17))


@functools.lru_cache(None)
def pow_cases() -> tuple:
    rnd = random.Random(61)
    es = [0, 1, 2, 3, 1 << 63, (1 << 64) - 1, P & ((1 << 64) - 1), 0x5555555555555555, (1 << 32) - 1, 1 << 32]
    e = edge_values()
    return tuple((a, es[i % len(es)]) for i, a in enumerate(e)) + tuple((rnd.randrange(P), rnd.randrange(1 << 64)) for _ in range(256)) \
        + tuple((P - 1, x) for x in es) + tuple((0, x) for x in es)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def mont_t(terms, c=0, bits=R_BITS) -> int:
    """the value a Montgomery product holds BEFORE any conditional subtraction: (sum a_i b_i + m p) / 2^bits + c with
    m = -sum / p mod 2^bits (the limb-wise m_i of the column loop add up to exactly this m)"""
    s = sum(a * b for a, b in terms)
    m = (s * _NEG_P_INV[bits]) % (1 << bits)
    t = s + m * P
    assert t % (1 << bits) == 0
    return (t >> bits) + c


def _mul_ref(a, b):
    t = mont_t([(a, b)])
    # (a b + m p) / R < (p^2 + R p) / R = p (1 + p / R) < 3 R / 4 + 2^117: one conditional subtraction, and the single product never
    # reaches bit 232 (the fused forms below do: their addend or second product takes them up to 3 p)
    assert t < 2 * P and t < R
    return t % P


def _limbs(x, w):
    return sum((((x >> (w * i)) & ((1 << w) - 1)) if i < 7 else (x >> (w * 7))) << (32 * i) for i in range(8))


def _muladd30_ref(a, b, c):
    t = mont_t([(a, b)], c, R30_BITS)
    assert t < R30, "case outside the precondition"
    return t


def _const30_ref(a):
    t = mont_t([(a, R30 % P)])  # fr_mul(a, 2^8 R mod p): the constant is 2^240 mod p
    assert t < 2 * P and a < P  # the operand goes through fr_mul's 29-bit slicing: bit 232 would be dropped
    return t % P


def _inv(y):
    return pow(y, -1, P) if y else 0


# name -> (case set, function of one case tuple -> tuple of outputs)
def _ops():
    one = lambda xs: tuple((x,) for x in xs)
    e = edge_values()
    return {
        "add": (pairs, lambda a, b: ((a + b) % P,)),
        "sub": (pairs, lambda a, b: ((a - b) % P,)),
        "neg": (lambda: one(e), lambda a: (-a % P,)),
        "dbl": (lambda: one(e), lambda a: (2 * a % P,)),
        "cond_sub_p": (lambda: one(below_2p()), lambda a: (a - P if a >= P else a,)),
        "is_canonical": (lambda: one(any_256()), lambda a: (int(a < P),)),
        "mul": (pairs, lambda a, b: (_mul_ref(a, b),)),
        "sqr": (lambda: one(e), lambda a: (_mul_ref(a, a),)),
        "to_mont": (lambda: one(e), lambda a: (_mul_ref(a, R * R % P),)),
        "from_mont": (lambda: one(e), lambda a: (_mul_ref(a, 1),)),
        "dot2": (quads, lambda a0, b0, a1, b1: (mont_t([(a0, b0), (a1, b1)]) % P,)),
        "muladd29": (triples, lambda a, b, c: (mont_t([(a, b)], c) % P,)),
        "mul29": (pairs, lambda a, b: (_mul_ref(a, b),)),
        "roundtrip29": (lambda: one(below_2_232()), lambda a: (a,)),
        "roundtrip30": (lambda: one(below_2_240()), lambda a: (a,)),
        "const30": (lambda: one(e), lambda a: (_const30_ref(a),)),
        "canon30": (lambda: one(below_2p()), lambda a: (a % P,)),
        "sub_lazy30": (lazy_pairs, lambda e0, e1: (e0 - e1 + 128 * P,)),
        "muladd30": (lazy_triples, lambda a, b, c: (_muladd30_ref(a, b, c),)),
        "muladd30_x2": (lazy_sextuples, lambda a0, b0, c0, a1, b1, c1: (_muladd30_ref(a0, b0, c0), _muladd30_ref(a1, b1, c1))),
        "inv": (lambda: one(inversion_inputs()), lambda a: (_inv(a) * R * R % P,)),
        "inv_gcd_raw": (lambda: one(inversion_inputs()), lambda a: (_inv(a),)),
        "inv_fermat": (lambda: one(inversion_inputs()), lambda a: (_inv(a) * R * R % P,)),
        "pow_u64": (pow_cases, lambda a, x: (pow(a * R_INV % P, x, P) * R % P,)),
        "limbs29": (lambda: one(below_2_232()), lambda a: (_limbs(a, 29),)),
        "limbs30": (lambda: one(below_2_240()), lambda a: (_limbs(a, 30),)),
    }


@functools.lru_cache(None)
def lazy_sextuples() -> tuple:
    """the two chains of the paired product get DIFFERENT operands: triple i with triple 5 i + 11"""
    t = lazy_triples()
    return tuple(t[i] + t[(5 * i + 11) % len(t)] for i in range(len(t)))


OPS = tuple(_ops())


@functools.lru_cache(None)
def cases(op: str) -> tuple:
    """the op's case tuples; never a multiple of 256, so that the last workgroup of the device flavour is ragged"""
    cs = tuple(_ops()[op][0]())
    return cs + cs[:1] if len(cs) % 256 == 0 else cs


@functools.lru_cache(None)
def inputs(op: str) -> tuple:
    """one packed buffer (n x 32 bytes) per operand"""
    cs = cases(op)
    return tuple(pack([c[k] for c in cs]) for k in range(len(cs[0])))


@functools.lru_cache(None)
def expected(op: str) -> tuple:
    """one packed buffer per output"""
    f = _ops()[op][1]
    outs = [f(*c) for c in cases(op)]
    return tuple(pack([o[k] for o in outs]) for k in range(len(outs[0])))


def gcd_steps(y: int) -> int:
    """steps of the plain binary extended GCD on (a, b) = (y, p) -- a odd and below b: swap; a odd: a -= b; then a /= 2 -- until
    b = 1, which is when its cofactor v is the inverse.  fr_inv_gcd_raw runs 16 rounds of 30 of these steps on approximations."""
    a, b, n = y, P, 0
    while b != 1 and a:
        if a & 1:
            if a < b:
                a, b = b, a
            a -= b
        a >>= 1
        n += 1
    return n


# ---- which branch a case takes, on the reference alone ----------------------------------------------------------------------------
def classify(op: str, case) -> str:
    if op == "add":
        s = case[0] + case[1]
        return "sum<p" if s < P else "sum=p" if s == P else "sum>p"
    if op == "sub":
        return "a=b" if case[0] == case[1] else "borrow" if case[0] < case[1] else "no borrow"
    if op == "cond_sub_p":
        return {P - 1: "p-1", P: "p", P + 1: "p+1", 2 * P - 1: "2p-1"}.get(case[0], "other")
    if op in ("mul", "mul29"):
        t = mont_t([case])
        return {1: "T=p+1", 2: "T=p+2", -1: "T=p-1", -2: "T=p-2"}.get(t - P, "T>=p" if t >= P else "T<p")
    if op == "muladd29":
        return f"{mont_t([case[:2]], case[2]) // P} subtractions"
    if op == "dot2":
        return f"{mont_t([case[:2], case[2:]]) // P} subtractions"
    raise KeyError(op)


@functools.lru_cache(None)
def branches(op: str) -> dict:
    """branch name -> number of cases of the op's set that take it"""
    out = {}
    for c in cases(op):
        k = classify(op, c)
        out[k] = out.get(k, 0) + 1
    return out


# ---- running an op through the library handed in (the tests' dvp fixture) and comparing ---------------------------------------------
def run_op(dvp, op, on_device, bufs=None):
    """the op over its whole case set: one packed buffer per output"""
    bufs = inputs(op) if bufs is None else bufs
    assert (len(bufs[0]) // 32) % 256 != 0
    return dvp.fr.debug_op(op, list(bufs), on_device)


def assert_same(op, got, want, what="reference"):
    for k, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        gi, wi = unpack(g), unpack(w)
        bad = [i for i in range(len(wi)) if gi[i] != wi[i]]
        i = bad[0]
        case = ", ".join(hex(x) for x in cases(op)[i])
        raise AssertionError(f"{op}: output {k} differs from the {what} at {len(bad)} of {len(wi)} elements; first at index {i}: "
                             f"inputs ({case}) gave {hex(gi[i])}, expected {hex(wi[i])}")
