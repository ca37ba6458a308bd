"""Case sets and the exact reference for the GF(2^233) arithmetic and the K-233 point formulas of dv-pari_amd/csrc/gf233.cuh and
k233.cuh (dvp_debug_gf_op, one function per element).  The reference is oracle/pyref.py alone (gf_mul, gf_sqr, gf_inv, gf_reduce,
k233_add, k233_dbl, k233_neg); the points k G come from the C oracle.  No code is shared with the library.

Why the basis: every multiplier of gf233.cuh is built from and, xor and shifts of its operands' bits, so whatever a wrong shift, mask,
fold or lane exchange turns it into is still GF(2)-bilinear, and a bilinear map is the field product iff it is on all 233 x 233 pairs
(z^i, z^j); likewise a GF(2)-linear map (squaring, x -> x^(2^k), the half-trace, a byte-table pass) is right iff it is on a basis --
for a table pass, on each of its 30 x 256 entries.  mul_basis_pairs() / tab_entries() are those sets; the edge and random operands are
for what is NOT linear in the operands: stale LDS rows, a lane reading its neighbour, exec-mask effects.

The same additivity serves the reference: frob(v, k), halftrace(v) and trace(v) combine pyref's values on the basis (233 x 232
calls of pyref.gf_sqr, once per session) instead of running k squarings per case; tests/test_gf_cases_cpu.py pins them to
pyref.gf_pow2k / gf_halftrace / gf_trace_def on samples."""
import functools
import random

import pyref as o

M = 233
MASK = (1 << M) - 1
RUN_LENGTHS = (1, 3, 63, 64, 65, 257)  # the last wave: one active lane / quad / row next to retired ones
DIGIT_WORD = 3  # the word whose comb digits are walked one by one: it holds the 117-bit split (bit 21) of gf_k_split
KS = (0, 1, 2, 7, 14, 28, 29, 30, 57, 58, 59, 115, 116, 117, 145, 174, 203, 231, 232)  # squaring counts: around every table run
TABLES = {"t29": 29, "t58": 58, "t116": 116, "th": None, "t14": 14, "t7": 7}  # None: the half-trace
TABLE_MIN_TABS = {"t14": 1, "t7": 2}  # smallest DVP_GF_INV_TABS that provides the table


def pack(vals) -> bytes:
    return b"".join([int(v).to_bytes(32, "little") for v in vals])


def unpack(buf: bytes) -> list:
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


# ---- field values ------------------------------------------------------------------------------------------------------------------
def basis() -> tuple:
    return tuple(1 << i for i in range(M))


@functools.lru_cache(None)
def equal_halves() -> tuple:
    """h | h << 117: a0 == a1 in gf_k_split, so Karatsuba's middle operand a0 + a1 is zero"""
    rnd = random.Random(23301)
    hs = [1, (1 << 116) - 1, 1 << 115, int("5" * 29, 16)] + [rnd.getrandbits(116) for _ in range(3)]
    return tuple(h | (h << 117) for h in hs)


@functools.lru_cache(None)
def digit_values() -> tuple:
    """each digit value at each comb position of word DIGIT_WORD (position 10 is the 2-bit top digit)"""
    out = []
    for pos in range(11):
        for d in range(1, 8):
            dig = (d << (3 * pos)) & 0xFFFFFFFF
            if dig:
                out.append(dig << (32 * DIGIT_WORD))
    return tuple(dict.fromkeys(out))


@functools.lru_cache(None)
def edge_values() -> tuple:
    lo = (1 << 117) - 1
    v = [0, 1, MASK, (1 << 232) | 1, lo, MASK ^ lo]
    v += list(equal_halves())
    v += [1 << 116, 1 << 117, 1 << 159]
    for k in range(1, 8):
        v += [1 << (32 * k - 1), 1 << (32 * k)]
    v.append(sum(0xC0000000 << (32 * w) for w in range(7)))  # the top comb digit of every word (word 7 ends at bit 8)
    v += [0xC0000000 << (32 * w) for w in range(7)]
    v += list(digit_values())
    assert all(0 <= x <= MASK for x in v)
    return tuple(dict.fromkeys(v))


@functools.lru_cache(None)
def random_values(n: int = 2000, seed: int = 2330) -> tuple:
    rnd = random.Random(seed)
    return tuple(rnd.getrandbits(M) for _ in range(n))


@functools.lru_cache(None)
def field_values() -> tuple:
    """what the one-operand functions see: the basis, the edges, 300 random dense values"""
    return tuple(dict.fromkeys(basis() + edge_values() + random_values()[:300]))


# ---- multiplication ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def mul_basis_pairs() -> tuple:
    """(a, b) = (z^i, z^j), all 233^2"""
    b = basis()
    return tuple((x, y) for x in b for y in b)


@functools.lru_cache(None)
def mul_other_pairs() -> tuple:
    """edges x edges, then 2 000 random pairs"""
    e, r = edge_values(), random_values()
    r2 = random_values(2000, 2331)
    return tuple((x, y) for x in e for y in e) + tuple(zip(r, r2))


def mul2_triples(pairs, rot: int) -> tuple:
    """(a1, a2, b): a1, b = the pair; a2 = the a of the pair `rot` places on with the same b where the list is a full grid (the basis
    pairs: a2 = z^(i + rot mod 233), so both first operands sweep the whole grid), of the next pair otherwise"""
    n = len(pairs)
    if n == M * M:
        return tuple((a, 1 << ((i // M + rot) % M), b) for i, (a, b) in enumerate(pairs))
    return tuple((a, pairs[(i + rot) % n][0], b) for i, (a, b) in enumerate(pairs))


@functools.lru_cache(None)
def mul_expected(which: str) -> tuple:
    return tuple(o.gf_mul(a, b) for a, b in (mul_basis_pairs() if which == "basis" else mul_other_pairs()))


# a call's first element for the products: the scanned operand's low comb digit is zero, so LDS row 0 is read before the lane has
# written any non-zero row
MUL_LEAD = (MASK ^ 7, MASK)


# ---- linear maps: the reference on the basis, combined ------------------------------------------------------------------------------
@functools.lru_cache(None)
def _frob_basis() -> tuple:
    rows = [list(basis())]
    for _ in range(M - 1):
        rows.append([o.gf_sqr(x) for x in rows[-1]])
    return tuple(tuple(r) for r in rows)


def _lin(images, v: int) -> int:
    r, i = 0, 0
    while v:
        if v & 1:
            r ^= images[i]
        v >>= 1
        i += 1
    return r


def frob(v: int, k: int) -> int:
    """v^(2^k), 0 <= k <= 232"""
    return _lin(_frob_basis()[k], v)


@functools.lru_cache(None)
def _halftrace_basis() -> tuple:
    f = _frob_basis()
    out = []
    for j in range(M):
        h = 0
        for i in range(117):
            h ^= f[2 * i][j]
        out.append(h)
    return tuple(out)


def halftrace(v: int) -> int:
    return _lin(_halftrace_basis(), v)


@functools.lru_cache(None)
def _trace_basis() -> tuple:
    f = _frob_basis()
    out = []
    for j in range(M):
        t = 0
        for k in range(M):
            t ^= f[k][j]
        assert t in (0, 1)
        out.append(t)
    return tuple(out)


def trace(v: int) -> int:
    return _lin(_trace_basis(), v)


@functools.lru_cache(None)
def inv(v: int) -> int:
    return o.gf_inv(v) if v else 0


@functools.lru_cache(None)
def inv_values() -> tuple:
    return tuple(dict.fromkeys((0, 1, MASK) + basis() + random_values()[:300]))


def table_map(name: str, v: int) -> int:
    k = TABLES[name]
    return halftrace(v) if k is None else frob(v, k)


@functools.lru_cache(None)
def tab_entries() -> tuple:
    """every (pos, byte) single-byte input of a table pass (pos 29 keeps bit 232 only), then 300 random dense values"""
    out = [((byte << (8 * pos)) & MASK) for pos in range(30) for byte in range(256)]
    return tuple(out) + random_values()[:300]


@functools.lru_cache(None)
def reduce_inputs(top: int) -> tuple:
    """512-bit polynomials as (low, high) halves: every single bit the form accepts, all ones, random ones"""
    bits = 32 * (top + 1)
    rnd = random.Random(2332 + top)
    v = [1 << i for i in range(bits)] + [(1 << bits) - 1, 0] + [rnd.getrandbits(bits) for _ in range(300)]
    v += [rnd.getrandbits(465) for _ in range(100)]  # as long as a product of two reduced elements
    return tuple(v)


def split512(vals):
    m = (1 << 256) - 1
    return [v & m for v in vals], [v >> 256 for v in vals]


# ---- points ------------------------------------------------------------------------------------------------------------------------
POINT_KS = (1, 2, 3, 0x1234567, 0x2F5D3B1C9E8A7F6055443322110FEDCBA9876543210FEDCBA98765, o.P - 5)
_ZRND = random.Random(23399)
Z_VALUES = (1, 2, MASK, _ZRND.getrandbits(M) | 1)


@functools.lru_cache(None)
def points() -> tuple:
    import c_oracle as co

    return tuple(co.k233_mulgen(k) for k in POINT_KS)


def ld_rep(pt, z):
    return (o.gf_mul(pt[0], z), o.gf_mul(pt[1], o.gf_sqr(z)), z)


def lam_of(pt):
    return pt[0] ^ o.gf_mul(pt[1], inv(pt[0]))


def lam_rep(pt, z):
    return (o.gf_mul(pt[0], z), o.gf_mul(lam_of(pt), z), z)


def ld_norm(X, Y, Z):
    """x = X / Z, y = Y / Z^2; None for Z == 0"""
    if Z == 0:
        return None
    zi = inv(Z)
    return (o.gf_mul(X, zi), o.gf_mul(Y, o.gf_sqr(zi)))


def lam_norm(X, L, Z):
    """x = X / Z, lambda = L / Z, y = x (lambda + x); None for Z == 0"""
    if Z == 0:
        return None
    zi = inv(Z)
    x, lam = o.gf_mul(X, zi), o.gf_mul(L, zi)
    return (x, o.gf_mul(x, lam ^ x))


class Case:
    """one element of a point op: ins = its input values, want = the affine result (None = infinity), flag = the flag it must return
    (None = the op has none), untouched = the op must hand p back bit for bit"""

    def __init__(self, cls, ins, want, flag=None, untouched=False):
        self.cls, self.ins, self.want, self.flag, self.untouched = cls, tuple(ins), want, flag, untouched


def _inf(rnd):
    return (rnd.getrandbits(M), rnd.getrandbits(M), 0)  # Z = 0 with garbage in the other two


# coordinates of an op's operands and of its result: "ld", "lam" or "aff"
POINT_OPS = {
    # name: (p, q, result)
    "ld_dbl": ("ld", None, "ld"), "ld_madd": ("ld", "aff", "ld"), "ld_madd_fast": ("ld", "aff", "ld"),
    "ld_add_aff_aff": ("aff", "aff", "ld"), "ld_add": ("ld", "ld", "ld"), "ld_add_nodbl": ("ld", "ld", "ld"),
    "lam_from_ld": ("ld", None, "lam"), "lam_to_ld": ("lam", None, "ld"), "lam_dbl": ("lam", None, "lam"), "lam_add": ("lam", "lam", "lam"),
    "ld_frob_n": ("ld", None, "ld"), "ld_to_aff": ("ld", None, "aff"),
}
FROB_KS = (0, 1, 2, 116, 232)


def _rep(kind, pt, z):
    return lam_rep(pt, z) if kind == "lam" else ld_rep(pt, z) if kind == "ld" else pt


@functools.lru_cache(None)
def point_cases(op: str, k: int = 0) -> tuple:
    """the cases of one point op (k: ld_frob_n's count)"""
    kp, kq, _ = POINT_OPS[op]
    rnd = random.Random(4242)
    P = points()
    cases = []
    if kq is None:  # one operand
        for pt in P:
            want = {"ld_dbl": o.k233_dbl(pt), "lam_dbl": o.k233_dbl(pt), "ld_frob_n": (frob(pt[0], k), frob(pt[1], k))}.get(op, pt)
            for z in Z_VALUES:
                cases.append(Case("generic", _rep(kp, pt, z), want, 1 if op == "ld_to_aff" else None))
        for _ in range(3):
            cases.append(Case("infinity", _inf(rnd), None, 0 if op == "ld_to_aff" else None))
        if op == "ld_dbl":  # N = (0, 1), the point of order 2: X1 == 0 -> Z3 == 0
            for z in Z_VALUES:
                cases.append(Case("order-2", ld_rep(o.N_STD, z), None))
        return tuple(cases)
    fast, nodbl = op == "ld_madd_fast", op in ("ld_add_nodbl", "lam_add")
    zq = Z_VALUES if kq != "aff" else (1,)
    zp = Z_VALUES if kp != "aff" else (1,)
    n = len(P)
    for i in range(n):
        a, b = P[i], P[(i + 1) % n]
        for za in zp:
            for zb in zq:
                cases.append(Case("generic", _rep(kp, a, za) + _rep(kq, b, zb), o.k233_add(a, b), 1 if fast or nodbl else None))
    if op == "ld_add_aff_aff":  # its contract: finite, different x
        return tuple(cases)
    for a in P[:4]:
        for za in zp:
            for zb in zq:
                if za == zb and kq != "aff":
                    continue  # two DIFFERENT representatives of one point
                cases.append(Case("P+P", _rep(kp, a, za) + _rep(kq, a, zb), o.k233_dbl(a), 0 if fast or nodbl else None, fast or nodbl))
                cases.append(Case("P-P", _rep(kp, a, za) + _rep(kq, o.k233_neg(a), zb), None, 0 if fast else 1 if nodbl else None, fast))
    if fast:  # its contract: p finite
        return tuple(cases)
    for a in P[:3]:
        for zb in zq:
            cases.append(Case("inf+Q", _inf(rnd) + _rep(kq, a, zb), a, 1 if nodbl else None))
        if kq != "aff":
            for za in zp:
                cases.append(Case("P+inf", _rep(kp, a, za) + _inf(rnd), a, 1 if nodbl else None))
    if kq != "aff":
        for _ in range(3):
            cases.append(Case("inf+inf", _inf(rnd) + _inf(rnd), None, 1 if nodbl else None))
    return tuple(cases)


def case_affine_inputs(op: str, c: Case):
    """the operands of a case as affine points (None = infinity), normalised by the reference"""
    kp, kq, _ = POINT_OPS[op]
    norm = {"ld": lambda v: ld_norm(*v), "lam": lambda v: lam_norm(*v), "aff": lambda v: v}
    np_ = 2 if kp == "aff" else 3
    out = [norm[kp](c.ins[:np_])]
    if kq is not None:
        out.append(norm[kq](c.ins[np_:]))
    return out


def chunks(n_total: int):
    """(start, length) of consecutive calls with the lengths of RUN_LENGTHS, repeated until n_total elements are covered"""
    out, at, i = [], 0, 0
    while at < n_total:
        ln = min(RUN_LENGTHS[i % len(RUN_LENGTHS)], n_total - at)
        out.append((at, ln))
        at += ln
        i += 1
    return out
