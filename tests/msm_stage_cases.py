"""The MSM bucket pipeline restated stage by stage in plain Python, from the comments of csrc/msm.hip and its stage headers msm_*.cuh (not from their code), and the parser
of the stage capture (dvp_debug_msm_capture_arm / _fetch, include/dvpari_internal.h).  Nothing here touches a device.

Every base of a test is k_i G with a known k_i, so every point the pipeline ever holds has a known discrete logarithm modulo the group
order r (pyref.P): an item of the sorted list is +- 2^(o_w) k_i (signed windows), lambda^(o_w) k_i (tau-adic rows) or k_i (a one-shot
MSM: its windows have bucket sets of their own), a pair round's slot adds two logarithms, logarithm 0 is the neutral element and is
stored as (0, 0).  check_capture walks a capture with that and compares every array bit for bit:
  (a) cnt / off / items with the bucket membership and the sort's layout (even starts, the spare word of an odd bucket);
  (b) every round's counts, offsets and descriptor words with the bookkeeping;
  (c) every output slot of every round with the group law on logarithms, through c_oracle.k233_mulgen;
  (d) bkt[k], normalised, with the sum of the bucket's round-0 inputs;
  (f) the bucket array behind every level of the merge tree: every slot the level wrote, normalised, with the logarithm the level's rule
      gives it, and the tree's invariant on the logarithms themselves;
  (g) save0 (signed digits) with bucket 0 as bkt held it, word for word;
  (h) the tails from the logarithms the last merge level left: the doubled or Frobenius-mapped points, the group sums of k_tail_groups
      one by one, the pairwise add trees;
  (i) the result -- (x, y), the infinity word and, where one was written, the 30-byte encoding -- with the oracle's.
The order inside a bucket is whatever the sort produced: membership is compared as a multiset, everything behind it is derived from the
captured order."""
import collections

import numpy as np

import pyref as o
import c_oracle as co
from util import TAU_D0, TAU_D1

R = o.P  # the group order (the scalar field)
LAMBDA = (-TAU_D0 * pow(TAU_D1, -1, R)) % R  # tau acts on E[r] as the multiplication by lambda
NONE = 0xFFFFFFFF
PAIR = 0x80000000
HDR_WORDS = 136
VERSION = 2
MAX_LEVELS = 24
TAILS = ("k_tail<true> -3", "k_tail<false> -3", "k_tail<false> frobenius", "k_tail_groups + k_tail<false> -4")
MERGE_CLASSES = ("generic", "P+P", "P-P", "O+Q", "P+O", "O+O")
MAGIC = 0x43505644
ROUTES = ("k_bucket_gather_items", "k_bucket_gather_aff", "k_bucket_pairs", "reducer_fast", "reducer_general")
CLASSES = ("generic", "P+P", "P-P", "O+Q", "P+O", "O+O", "leftover", "leftover O")
O_CLASSES = ("O+Q", "P+O", "O+O", "leftover O")


# ---- windows and recoding ------------------------------------------------------------------------------------------------------

def window_split(c):
    """234 digits in ceil(234 / c) windows whose widths differ by at most one: (windows, n_narrow), the n_narrow LOW ones c - 1 wide"""
    w = (234 + c - 1) // c
    return w, w * c - 234


def window_widths(c, W, n_narrow):
    return [c - 1 if w < n_narrow else c for w in range(W)]


def window_starts(c, W, n_narrow):
    """o_w: the first digit of window w"""
    out, at = [], 0
    for wd in window_widths(c, W, n_narrow):
        out.append(at)
        at += wd
    return out


def signed_recode(x, c):
    """the textbook signed-digit decomposition of x over the evened-out windows of window_split(c): [(o_w, d_w)] with
    sum_w d_w 2^(o_w) = x and |d_w| <= 2^(width_w - 1); window w holds its bits plus the carry from below, a digit above half its
    range becomes digit - 2^width with a carry"""
    W, n_narrow = window_split(c)
    exp, carry, off = [], 0, 0
    for wd in window_widths(c, W, n_narrow):
        d = ((x >> off) & ((1 << wd) - 1)) + carry
        carry = 0
        if d > (1 << (wd - 1)):
            d, carry = d - (1 << wd), 1
        exp.append((off, d))
        off += wd
    assert carry == 0 and sum(d << o_w for o_w, d in exp) == x
    return exp


def signed_key(d, c):
    """the bucket of a signed digit: its magnitude, 2^(c-1) sharing bucket 0"""
    return abs(d) & ((1 << (c - 1)) - 1)


def tau_windows(x, c, W, n_narrow):
    """the tau-adic {0, 1} digits of x (c_oracle.tau_digits) cut into the windows' widths: one pattern per window"""
    dg = co.tau_digits(x)
    out = []
    for o_w, wd in zip(window_starts(c, W, n_narrow), window_widths(c, W, n_narrow)):
        out.append(sum(b << t for t, b in enumerate(dg[o_w:o_w + wd])))
    assert len(dg) <= sum(window_widths(c, W, n_narrow))
    return out


def pattern_weight(d, o_w):
    """sum_t d_t lambda^(o_w + t): what a tau-adic bucket of pattern d in a window that starts at digit o_w weighs"""
    return sum(pow(LAMBDA, o_w + t, R) for t in range(d.bit_length()) if (d >> t) & 1) % R


# ---- the capture ---------------------------------------------------------------------------------------------------------------

class Capture:
    """hdr: dict of the header's fields; cnt, off, items: uint32 arrays; rounds: [dict(ocnt, ooff, desc, pts)], pts [total, 16] uint32;
    bkt [nkeys, 24] uint32; levels: [[nkeys, 24] uint32] (lambda-projective), one per merge level; save0: 24 words or None; parts:
    [nparts, 24] uint32 or None; res_xy: 16 words; res_inf: int; res_enc: 30 bytes or None"""

    def __init__(self, hdr, cnt, off, items, rounds, bkt, levels=(), save0=None, parts=None, res_xy=None, res_inf=None, res_enc=None):
        self.hdr, self.cnt, self.off, self.items, self.rounds, self.bkt = hdr, cnt, off, items, rounds, bkt
        self.levels, self.save0, self.parts, self.res_xy, self.res_inf, self.res_enc = list(levels), save0, parts, res_xy, res_inf, res_enc

    @property
    def fixed(self):
        return bool(self.hdr["flavour"] & 1)

    @property
    def signed(self):
        return bool(self.hdr["flavour"] & 2)


HDR_FIELDS = ("magic", "version", "hdr_words", "flavour", "c", "W", "n_narrow", "nkeys", "sign_mask", "n_total", "i0", "n", "ra", "ra_plan",
              "dense", "pipeline", "tpb", "aff_cap", "bmax", "bmin", "route", "K", "max_cnt", "items_len")


def parse_capture(blob):
    w = np.frombuffer(bytes(blob), dtype="<u4")
    hdr = {k: int(w[i]) for i, k in enumerate(HDR_FIELDS)}
    assert hdr["magic"] == MAGIC and hdr["version"] == VERSION and hdr["hdr_words"] == HDR_WORDS, hdr
    hdr["share"] = [int(x) for x in w[24:24 + hdr["ra"]]]
    hdr["total"] = [int(x) for x in w[64:64 + hdr["ra"]]]
    hdr.update(levels=int(w[104]), tail=int(w[105]), nparts=int(w[106]), enc=int(w[107]), rule=int(w[108]))
    assert hdr["levels"] <= MAX_LEVELS and hdr["tail"] < len(TAILS), hdr
    hdr["group"] = [int(x) for x in w[112:112 + hdr["levels"]]]
    at = [HDR_WORDS]

    def take(n):
        v = w[at[0]:at[0] + n]
        assert len(v) == n, "the blob is shorter than its header says"
        at[0] += n
        return v

    nk = hdr["nkeys"]
    cnt, off, items = take(nk), take(nk + 1), take(hdr["items_len"])
    rounds = []
    for r in range(hdr["ra"]):
        t = hdr["total"][r]
        ocnt, ooff = take(nk), take(nk + 1)
        desc = take(0 if r == 0 else (2 * t if hdr["dense"] else t))
        rounds.append(dict(ocnt=ocnt, ooff=ooff, desc=desc, pts=take(16 * t).reshape(t, 16)))
    bkt = take(24 * nk).reshape(nk, 24)
    levels = [take(24 * nk).reshape(nk, 24) for _ in range(hdr["levels"])]
    save0 = take(24) if hdr["sign_mask"] else None
    parts = take(24 * hdr["nparts"]).reshape(hdr["nparts"], 24) if hdr["tail"] == 3 else None
    res_xy, res_inf = take(16), int(take(1)[0])
    res_enc = take(8).tobytes()[:30] if hdr["enc"] else None
    assert at[0] == len(w), "the blob is longer than its header says"
    return Capture(hdr, cnt, off, items, rounds, bkt, levels, save0, parts, res_xy, res_inf, res_enc)


def words_to_int(v):
    return int.from_bytes(np.ascontiguousarray(v, dtype="<u4").tobytes(), "little")


def int_to_words(x, n=8):
    return np.frombuffer(int(x).to_bytes(4 * n, "little"), dtype="<u4")


# ---- the sort ------------------------------------------------------------------------------------------------------------------

def sort_offsets(cnt):
    """every bucket starts at an even item position: the exclusive scan of the counts rounded up to even, the total last"""
    off, at = [], 0
    for c in cnt:
        off.append(at)
        at += (int(c) + 1) & ~1
    return off + [at]


def membership(hdr, scalars, inf=None):
    """key -> multiset (Counter) of the item words the sort must put into that bucket, from the scalars of one MSM (integers, scalar j
    belongs to base i0 + j).  Fixed-base: an item names a table entry, row * n_total + i0 + j, bit 31 = it is subtracted (signed
    windows); one-shot: the item is j and the key carries the window, w 2^c + pattern."""
    c, W, nn = hdr["c"], hdr["W"], hdr["n_narrow"]
    fixed, signed = hdr["flavour"] & 1, hdr["flavour"] & 2
    out = collections.defaultdict(collections.Counter)
    for j, x in enumerate(scalars):
        if inf is not None and inf[j]:
            continue
        if signed:
            assert window_split(c) == (W, nn)
            for w, (_, d) in enumerate(signed_recode(x, c)):
                if d:
                    out[signed_key(d, c)][(w * hdr["n_total"] + hdr["i0"] + j) | (hdr["sign_mask"] if d < 0 else 0)] += 1
        else:
            for w, d in enumerate(tau_windows(x, c, W, nn)):
                if d:
                    if fixed:
                        out[d][w * hdr["n_total"] + hdr["i0"] + j] += 1
                    else:
                        out[(w << c) | d][j] += 1
    return out


def item_log(hdr, word, base_logs):
    """the discrete logarithm of the point a sorted item names: row w of a fixed-base table holds 2^(o_w) P (signed windows; the item's
    sign bit subtracts it) or tau^(o_w) P = lambda^(o_w) P; a one-shot MSM's item is the base itself"""
    idx = word & ~hdr["sign_mask"] & 0xFFFFFFFF
    if not hdr["flavour"] & 1:
        return base_logs[idx] % R
    row, i = divmod(idx, hdr["n_total"])
    o_w = window_starts(hdr["c"], hdr["W"], hdr["n_narrow"])[row]
    k = base_logs[i] * (pow(2, o_w, R) if hdr["flavour"] & 2 else pow(LAMBDA, o_w, R))
    return (-k if word & hdr["sign_mask"] else k) % R


def bucket_weight(hdr, key):
    """what bucket `key` weighs in the MSM's result"""
    c = hdr["c"]
    if hdr["flavour"] & 2:
        return key if key else 1 << (c - 1)
    if hdr["flavour"] & 1:
        return pattern_weight(key, 0)
    return pattern_weight(key & ((1 << c) - 1), window_starts(c, hdr["W"], hdr["n_narrow"])[key >> c])


# ---- round bookkeeping ---------------------------------------------------------------------------------------------------------

def halve(cnt):
    """c_r = ceil(c_(r-1) / 2) and its exclusive scan (nkeys + 1 entries, the total last)"""
    c = [(int(x) + 1) >> 1 for x in cnt]
    off, at = [], 0
    for x in c:
        off.append(at)
        at += x
    return c, off + [at]


def desc_words(c_in, o_in, o_out):
    """one word per output slot of a round after the first, in bucket order: slot o_out[k] + j adds inputs o_in[k] + 2 j and + 1 (PAIR set)
    or passes the bucket's odd leftover on"""
    d = [0] * o_out[-1]
    for k, c in enumerate(c_in):
        for j in range((c + 1) >> 1):
            d[o_out[k] + j] = (o_in[k] + 2 * j) | (PAIR if 2 * j + 1 < c else 0)
    return d


def desc_dense(c_in, o_in, o_out):
    """two words per slot {input | PAIR, output index}: a round's additions fill slots [0, A), its odd leftovers [A, total).  The pairs of
    a key start at o_r - o_(r+1), its leftover sits at A + 2 o_(r+1) - o_r, A = o_r[nkeys] - o_(r+1)[nkeys]"""
    total, A = o_out[-1], o_in[-1] - o_out[-1]
    d = [None] * total
    for k, c in enumerate(c_in):
        for j in range(c >> 1):
            d[o_in[k] - o_out[k] + j] = ((o_in[k] + 2 * j) | PAIR, o_out[k] + j)
        if c & 1:
            d[A + 2 * o_out[k] - o_in[k]] = (o_in[k] + c - 1, o_out[k] + (c >> 1))
    assert all(x is not None for x in d)
    return [w for pair in d for w in pair]


def round_slots(hdr, r, items_or_desc, total):
    """the slots of round r as the kernel sees them: [(a, b, out)] by slot number; b = None for a leftover.  Round 0 reads the sorted item
    list as (a, b) pairs (b = NONE behind an odd bucket: a leftover), later rounds their descriptors"""
    d = [int(x) for x in items_or_desc]
    if r == 0:
        return [(d[2 * s], None if d[2 * s + 1] == NONE else d[2 * s + 1], s) for s in range(total)]
    if hdr["dense"]:
        return [((d[2 * s] & ~PAIR), (d[2 * s] & ~PAIR) + 1 if d[2 * s] & PAIR else None, d[2 * s + 1]) for s in range(total)]
    return [((d[s] & ~PAIR), (d[s] & ~PAIR) + 1 if d[s] & PAIR else None, s) for s in range(total)]


# ---- slot geometry -------------------------------------------------------------------------------------------------------------

def slots_per_thread(total, cap, bmax, bmin):
    """B: a round of `total` slots is R = ceil(units / bmax) chip-fulls (units = slots per resident thread if it were one) of
    ceil(units / R) slots per thread, and never fewer than bmin"""
    units = (total + cap - 1) // cap
    rr = (units + bmax - 1) // bmax
    b = (units + rr - 1) // rr if rr else 1
    return max(b, bmin)


Position = collections.namedtuple("Position", "thread chain wg wave lane nthr B")


def slot_position(s, total, B, tpb):
    """slot s belongs to thread s mod nthr at chain position s div nthr, nthr = ceil(total / B)"""
    nthr = (total + B - 1) // B
    t = s % nthr
    return Position(t, s // nthr, t // tpb, (t % tpb) // 64, t % 64, nthr, B)


def round_positions(hdr, r):
    total = hdr["total"][r]
    B = slots_per_thread(total, hdr["aff_cap"], hdr["bmax"], hdr["bmin"])
    return [slot_position(s, total, B, hdr["tpb"]) for s in range(total)]


# ---- the group law on logarithms -----------------------------------------------------------------------------------------------

def classify(a, b):
    """the class of a slot from the logarithms of its operands (b = None: no partner)"""
    if b is None:
        return "leftover O" if a == 0 else "leftover"
    if a == 0:
        return "O+O" if b == 0 else "O+Q"
    if b == 0:
        return "P+O"
    if a == b:
        return "P+P"
    if (a + b) % R == 0:
        return "P-P"
    return "generic"


class Mulgen:
    """c_oracle.k233_mulgen with a memo: log -> the 16 words of (x, y); logarithm 0 is the marker (0, 0)"""

    def __init__(self):
        self.memo = {0: bytes(64)}
        self.calls = 0

    def words(self, k):
        k %= R
        v = self.memo.get(k)
        if v is None:
            self.calls += 1
            x, y = co.k233_mulgen(k)
            v = self.memo[k] = x.to_bytes(32, "little") + y.to_bytes(32, "little")
        return v


def ld_to_affine_bytes(w24):
    """raw Lopez-Dahab (X, Y, Z) -> the 64 bytes of (X / Z, Y / Z^2); Z = 0 is the neutral element -> (0, 0)"""
    X, Y, Z = (words_to_int(w24[8 * i:8 * i + 8]) for i in range(3))
    if Z == 0:
        return bytes(64)
    zi = co.gf_inv(Z)
    x, y = co.gf_mul(X, zi), co.gf_mul(Y, co.gf_mul(zi, zi))
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def lam_to_affine_bytes(w24):
    """lambda-projective (X, L, Z) -> the 64 bytes of (x, y) with x = X / Z, y = x (L / Z + x); Z = 0 is the neutral element -> (0, 0)"""
    X, L, Z = (words_to_int(w24[8 * i:8 * i + 8]) for i in range(3))
    if Z == 0:
        return bytes(64)
    zi = co.gf_inv(Z)
    x = co.gf_mul(X, zi)
    y = co.gf_mul(x, co.gf_mul(L, zi) ^ x)
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def batch_inverse(vals):
    """the inverses of nonzero field elements from ONE inversion: prefix products, the inverse of the last, and back"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = co.gf_mul(acc, v)
    inv, out = co.gf_inv(acc) if vals else 1, [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = co.gf_mul(inv, pre[i])
        inv = co.gf_mul(inv, vals[i])
    return out


def to_affine_many(rows, lam):
    """[lam_to_affine_bytes(r) for r in rows] (lam) or [ld_to_affine_bytes(r) for r in rows]: the same bytes, the rows sharing one
    inversion (an inversion of the oracle costs hundreds of its products)"""
    xs = [tuple(words_to_int(r[8 * i:8 * i + 8]) for i in range(3)) for r in rows]
    live = [i for i, t in enumerate(xs) if t[2]]
    out = [bytes(64)] * len(xs)
    for i, zi in zip(live, batch_inverse([xs[i][2] for i in live])):
        X, Y, _ = xs[i]
        x = co.gf_mul(X, zi)
        y = co.gf_mul(x, co.gf_mul(Y, zi) ^ x) if lam else co.gf_mul(Y, co.gf_mul(zi, zi))
        out[i] = x.to_bytes(32, "little") + y.to_bytes(32, "little")
    return out


# ---- the merge tree and the tails on logarithms -----------------------------------------------------------------------------------

def merge_level(logs, j):
    """level j of the merge tree -> (the array behind it, adds).  In every block of 2^(j+1) slots: slot s <= j becomes slot s + slot
    2^j + s, slot j + 1 becomes the old slot 2^j (T_right: the right half's total), every other slot keeps its value.  adds[blk (j + 1)
    + s] = the (left, right) operands of that addition, in the numbering the kernel gives its additions"""
    out, adds, h = list(logs), [], 1 << j
    for base in range(0, len(logs), 2 * h):
        for s in range(j + 1):
            l, r = logs[base + s], logs[base + h + s]
            adds.append((l, r))
            out[base + s] = (l + r) % R
        out[base + j + 1] = logs[base + h]
    return out, adds


def assert_merge_invariant(bucket_logs, logs, j):
    """THE invariant of the tree: after level j, slot 0 of a block of 2^(j+1) slots is the block's total and slot 1 + t (t <= j) is the
    sum of its buckets whose index has bit t set -- by the buckets the tree started from"""
    n = 2 << j
    for base in range(0, len(logs), n):
        blk = bucket_logs[base:base + n]
        assert logs[base] == sum(blk) % R, ("merge invariant", "level", j, "block", base // n, "slot", 0)
        for t in range(j + 1):
            assert logs[base + 1 + t] == sum(v for i, v in enumerate(blk) if (i >> t) & 1) % R, ("merge invariant", "level", j, "block", base // n, "slot", 1 + t)


def tail_shape(hdr):
    """(W, n_narrow) as the tail kernels take them: a fixed-base MSM has ONE bucket set and, tau-adic, rows that carry lambda^(o_w)
    already: W = 1, n_narrow = 0"""
    return (1, 0) if hdr["flavour"] & 1 else (hdr["W"], hdr["n_narrow"])


def tail_points(hdr, A, save0_log):
    """the logarithms of the points the tail adds up, from the array A the last merge level left.
    signed digits: 2^t A[1 + t], t < c - 1, then 2^(c-1) x bucket 0 as it was kept aside (save0);
    Frobenius:     lambda^k A[(w << c) + 1 + t] at position w c + t, k = w c - min(w, n_narrow) + t (the first digit of window w plus t)"""
    c = hdr["c"]
    if hdr["flavour"] & 2:
        return [(A[1 + t] << t) % R for t in range(c - 1)] + [(save0_log << (c - 1)) % R]
    W, nn = tail_shape(hdr)
    return [A[(w << c) + 1 + t] * pow(LAMBDA, w * c - min(w, nn) + t, R) % R for w in range(W) for t in range(c)]


def add_tree(logs):
    """the pairwise add tree of the tails: level after level entry i becomes entry 2 i + entry 2 i + 1, an unpaired last entry is passed
    on -> (the total, [[class of pair i] per level]); classes as `classify`, the unpaired entry a leftover"""
    levels, cur = [], [x % R for x in logs]
    while len(cur) > 1:
        pairs = [(cur[2 * i], cur[2 * i + 1] if 2 * i + 1 < len(cur) else None) for i in range((len(cur) + 1) // 2)]
        levels.append([classify(a, b) for a, b in pairs])
        cur = [a if b is None else (a + b) % R for a, b in pairs]
    return (cur[0] if cur else 0), levels


def tail_restated(hdr, A, save0_log, shape):
    """the tail of shape `shape` (TAILS) over the array A the last merge level left: dict(shape, points, groups, parts, tree, total) --
    points = tail_points; shape 3: groups[g] = add_tree's classes inside the 16 consecutive points of group g, parts[g] = its sum, tree =
    add_tree's classes over the parts; else tree = add_tree's classes over the points; total = the result's logarithm"""
    pts = tail_points(hdr, A, save0_log)
    tail = dict(shape=shape, points=pts, groups=None, parts=None)
    if shape == 3:
        sums = [add_tree(pts[g:g + 16]) for g in range(0, len(pts), 16)]
        tail["parts"], tail["groups"] = [t for t, _ in sums], [lv for _, lv in sums]
        tail["total"], tail["tree"] = add_tree(tail["parts"])
    else:
        tail["total"], tail["tree"] = add_tree(pts)
    return tail


class Checked(tuple):
    """what check_capture returns: the pair (classes, bucket_logs) it always returned, and beside it
      merge[j][a]  the class of addition a = block (j + 1) + slot of merge level j;
      tail         dict(shape, points = the logarithms the tail adds up, tree = add_tree's classes over them (shape 3: over the group
                   sums), groups = [add_tree's classes inside group g] and parts = the group sums' logarithms (shape 3, else None));
      total        the logarithm of the result"""

    def __new__(cls, classes, bucket_logs, merge, tail, total):
        self = super().__new__(cls, (classes, bucket_logs))
        self.merge, self.tail, self.total = merge, tail, total
        return self


def encode_point(log, rule, mulgen=None):
    """the oracle's 30-byte encoding of log x G under codec rule `rule`; the neutral element is 30 zero bytes"""
    if log % R == 0:
        return bytes(30)
    w = (mulgen or Mulgen()).words(log)
    pt = (int.from_bytes(w[:32], "little"), int.from_bytes(w[32:], "little"))
    return co.xsk233_encode(pt) if rule == 0 else o.xsk233_encode(pt, rule)


def check_merge_tail(cap, bucket_logs, mg):
    """checks (f) to (i) of the module's docstring; bucket_logs as check (d) found them -> (merge classes, tail dict, total)"""
    hdr = cap.hdr
    nk, c, signed = hdr["nkeys"], hdr["c"], bool(hdr["flavour"] & 2)
    assert hdr["levels"] == (c - 1 if signed else c) == len(cap.levels), ("merge", "levels", hdr["levels"])
    assert all(g in (1, 4, 16) for g in hdr["group"]), ("merge", "lanes per addition", hdr["group"])
    # (f) level by level
    logs, merge = [x % R for x in bucket_logs], []
    for j in range(hdr["levels"]):
        logs, adds = merge_level(logs, j)
        assert_merge_invariant(bucket_logs, logs, j)
        cls = [classify(l, r) for l, r in adds]
        merge.append(cls)
        n = 2 << j
        wrote = [base + s for base in range(0, nk, n) for s in range(j + 2)]  # slots 0 .. j + 1 of every block
        got = to_affine_many([cap.levels[j][i] for i in wrote], lam=True)
        for i, g in zip(wrote, got):
            blk, s = divmod(i, n)
            what = cls[blk * (j + 1) + s] if s <= j else "T_right"
            assert g == mg.words(logs[i]), ("merge", "level", j, "block", blk, "slot", s, what, "lanes", hdr["group"][j])
    # (g) bucket 0 kept aside
    if signed:
        assert cap.save0 is not None and bytes(np.ascontiguousarray(cap.save0)) == bytes(np.ascontiguousarray(cap.bkt[0])), ("save0", "is not bucket 0 as the reducer left it")
    else:
        assert cap.save0 is None, ("save0", "captured without signed digits")
    # (h) the tail, from what the last level left
    shape = hdr["tail"]
    assert (shape in (0, 1)) == signed, ("tail", "shape", TAILS[shape], "flavour", hdr["flavour"])
    tail = tail_restated(hdr, logs, bucket_logs[0], shape)
    total = tail["total"]
    if shape == 3:
        assert hdr["nparts"] == (len(tail["points"]) + 15) // 16 == len(cap.parts), ("tail groups", "nparts", hdr["nparts"])
        for g, (got, want) in enumerate(zip(to_affine_many(list(cap.parts), lam=False), tail["parts"])):
            assert got == mg.words(want), ("tail groups", "group", g, "of", hdr["nparts"], "classes", tail["groups"][g])
    else:
        assert hdr["nparts"] == 0 and cap.parts is None, ("tail groups", "captured without k_tail_groups")
    # (i) the result
    assert bytes(np.ascontiguousarray(cap.res_xy)) == mg.words(total), ("result", "xy", TAILS[shape], "tree", tail["tree"])
    assert cap.res_inf == (1 if total == 0 else 0), ("result", "inf", cap.res_inf, TAILS[shape])
    if hdr["enc"]:
        assert cap.res_enc == encode_point(total, hdr["rule"], mg), ("encoding", "rule", hdr["rule"], TAILS[shape], "neutral" if total == 0 else "finite")
    else:
        assert cap.res_enc is None, ("encoding", "captured but the header says none was written")
    return merge, tail, total


def check_capture(cap, base_logs, scalars, inf=None, mulgen=None):
    """checks (a) to (d) and (f) to (i) of the module's docstring on one capture; base_logs[i] = the logarithm of base i of the whole
    base vector, scalars = this MSM's, as integers.  Returns a Checked: the pair (classes, bucket_logs) -- classes[r][s] = the class of
    slot s of round r, bucket_logs[k] = the logarithm of bucket k's sum -- with the merge classes, the tail's and the result's logarithm
    as attributes.  An AssertionError names the stage, the round or level, and the slot, block or group."""
    hdr = cap.hdr
    nk = hdr["nkeys"]
    mg = mulgen or Mulgen()
    cnt = [int(x) for x in cap.cnt]
    off = [int(x) for x in cap.off]
    items = [int(x) for x in cap.items]
    # (a) the sort
    assert off == sort_offsets(cnt), ("sort", "off is not the scan of the counts rounded up to even")
    assert len(items) == off[-1] == hdr["items_len"]
    want = membership(hdr, scalars, inf)
    assert max(cnt, default=0) == hdr["max_cnt"], ("sort", "the largest bucket", max(cnt), hdr["max_cnt"])
    for k in range(nk):
        got = collections.Counter(items[off[k]:off[k] + cnt[k]])
        assert off[k] % 2 == 0 and got == want.get(k, collections.Counter()), ("sort", "bucket", k)
        if cnt[k] & 1:
            assert items[off[k] + cnt[k]] == NONE, ("sort", "spare word of bucket", k)
    assert sum(cnt) == sum(sum(v.values()) for v in want.values())
    # the rounds
    in_logs = None  # the logarithms of the round's input points, by input index
    c_in, o_in = cnt, off
    classes = []
    for r in range(hdr["ra"]):
        rd = cap.rounds[r]
        c_out, o_out = halve(c_in)
        # (b) bookkeeping
        assert [int(x) for x in rd["ocnt"]] == c_out, ("bookkeeping", "round", r, "counts")
        assert [int(x) for x in rd["ooff"]] == o_out, ("bookkeeping", "round", r, "offsets")
        total = o_out[-1]
        assert total == hdr["total"][r]
        if r == 0:
            slots = round_slots(hdr, 0, items, total)
        else:
            exp = desc_dense(c_in, o_in, o_out) if hdr["dense"] else desc_words(c_in, o_in, o_out)
            assert [int(x) for x in rd["desc"]] == exp, ("bookkeeping", "round", r, "descriptors")
            slots = round_slots(hdr, r, rd["desc"], total)
        # (c) every output slot
        out_logs = [None] * total
        cls = []
        raw = rd["pts"].tobytes()
        for s, (a, b, dst) in enumerate(slots):
            la = item_log(hdr, a, base_logs) if r == 0 else in_logs[a]
            lb = None if b is None else (item_log(hdr, b, base_logs) if r == 0 else in_logs[b])
            cls.append(classify(la, lb))
            lo = la if lb is None else (la + lb) % R
            assert out_logs[dst] is None, ("bookkeeping", "round", r, "two slots write output", dst)
            out_logs[dst] = lo
            assert raw[64 * dst:64 * dst + 64] == mg.words(lo), ("pair round", r, "slot", s, "output", dst, cls[-1])
        classes.append(cls)
        in_logs, c_in, o_in = out_logs, c_out, o_out
    # (d) the buckets
    bucket_logs = []
    for k in range(nk):
        lk = sum(item_log(hdr, w, base_logs) for w in items[off[k]:off[k] + cnt[k]]) % R
        bucket_logs.append(lk)
    for k, got in enumerate(to_affine_many(list(cap.bkt), lam=False)):
        assert got == mg.words(bucket_logs[k]), ("leftovers", ROUTES[hdr["route"]], "bucket", k)
    merge, tail, total = check_merge_tail(cap, bucket_logs, mg)
    assert total == weighted_sum(hdr, bucket_logs), ("tail", "the total is not the weighted sum of the buckets")
    return Checked(classes, bucket_logs, merge, tail, total)


def weighted_sum(hdr, bucket_logs):
    """the logarithm of the MSM's result from its buckets' logarithms"""
    return sum(bucket_weight(hdr, k) * lk for k, lk in enumerate(bucket_logs) if lk) % R


# ---- the placement input: crafted bucket counts for the signed fixed-base flavour at c = 8 ----------------------------------------

PLACE_C = 8  # 128 buckets; windows 0 .. 5 are seven bits wide, so a scalar below 2^8 reaches windows 0 and 1 only
PLACE_SLOTS = (8, 256, 136, 200)  # round-0 slots of the four regions below: 600 in all


def placement_input(seed=4711):
    """(base_logs, scalars, regions) for a fixed-base MSM with DVP_MSM_FIXED_C = 8: at most 1 200 bases, scalars below 2^8, largest bucket
    33 (six pair rounds).  The seven-bit window 0 reaches the keys 1 .. 64 only.  A bucket of c items takes ceil(c / 2) consecutive slots of the first pair round, bucket after bucket, so the
    counts alone decide which slot -- and with the slot geometry which lane, wave, workgroup and chain position -- a bucket's pairs get:
      region P, slots [0, 8):      buckets 1 .. 8 hold {P, -P} each: a P - P slot under ANY order inside the bucket.  Bucket 1 pairs a
                                   row-0 entry with a row-1 entry (scalar 128 on the base a / 2^7), bucket 2 holds the two row-1 entries of
                                   the scalars 256 - q, whose window-0 digits are negative (sign bit set) and land in two generic buckets;
      region A, slots [8, 264):    buckets of 32, 33, 12, 6, 4 and 2 items that are all +-P of one point per bucket: every pair is P + P or
                                   P - P whatever the order, and the rounds behind meet +-2P, +-4P and neutral operands.  Which of them
                                   depends on the order; the signs are laid out over the ranks in eight patterns so that any fixed
                                   order yields all of them;
      region G, slots [264, 400):  buckets of 9 .. 30 distinct random points: generic additions and leftovers;
      region Z, slots [400, 600):  as A; the last bucket is a {P, -P}: the last slot of the round is exceptional.
    With one slot per thread the first 264 threads meet exceptional pairs only (whole workgroups of 64, 128 and 256); with three (200
    threads) thread t owns slots t, 200 + t, 400 + t: chain positions 0 and 2 of every thread below 64 are exceptional, position 1 too.
    regions: name -> (first key, last key + 1, first slot, last slot + 1)."""
    import random

    rnd = random.Random(seed)
    inv128 = pow(128, -1, R)
    logs, scalars = [], []
    counts = {}

    def add(log, s, key_items):
        logs.append(log % R)
        scalars.append(s)
        for k in key_items:
            counts[k] = counts.get(k, 0) + 1

    def pure(key, size, pattern):
        a = rnd.randrange(1, R)
        for i in range(size):
            add(a if pattern[i % len(pattern)] == "+" else -a, key, [key])

    patterns = ["+-", "+", "++--", "+++-", "+-++", "-+++", "++-+", "+--+"]
    a1, t2 = rnd.randrange(1, R), rnd.randrange(1, R)
    g_first = None
    regions = {}
    # region P
    add(a1 * inv128, 128, [1])
    add(-a1, 1, [1])
    for k in range(3, 9):
        pure(k, 2, "+-")
    key, slot = 9, 8
    regions["P"] = (1, 9, 0, 8)

    def pure_region(name, slots, sizes, last_pair):
        nonlocal key, slot
        first_key, first_slot, left, i = key, slot, slots - (1 if last_pair else 0), 0
        while left:
            size = min(sizes[i % len(sizes)], 2 * left)
            if (size + 1) // 2 > left:
                size = 2 * left
            pat = patterns[(key + i) % len(patterns)] if size > 6 else "".join("-" if j == key % size else "+" for j in range(size))
            pure(key, size, pat)
            left -= (size + 1) // 2
            key, i = key + 1, i + 1
        if last_pair:
            pure(key, 2, "+-")
            key += 1
        slot += slots
        regions[name] = (first_key, key, first_slot, slot)

    pure_region("A", PLACE_SLOTS[1], [32, 33, 32, 12, 32, 33, 6, 32, 32, 4], False)
    # region G: distinct random points; its first two buckets also get the negative window-0 digit of a scalar 256 - q
    g_first, left, i = key, PLACE_SLOTS[2], 0
    sizes = [17, 24, 9, 20, 13, 30, 11, 16]
    while left:
        size = min(sizes[i % len(sizes)], 2 * left)
        neg = 1 if key < g_first + 2 else 0
        for _ in range(size - neg):
            add(rnd.randrange(1, R), key, [key])
        if neg:  # key `key` gets -(t2 / 128) or +(t2 / 128) with the sign bit, bucket 2 gets row 1 of it: +-t2
            add(t2 * inv128 * (1 if key == g_first else -1), 256 - key, [key, 2])
        left -= (size + 1) // 2
        key, i = key + 1, i + 1
    regions["G"] = (g_first, key, slot, slot + PLACE_SLOTS[2])
    slot += PLACE_SLOTS[2]
    pure_region("Z", PLACE_SLOTS[3], [32, 32, 33, 12, 32, 6, 32], True)
    assert key <= 65 and len(logs) <= 1200 and max(counts.values()) == 33 and counts[1] == counts[2] == 2, (key, len(logs), max(counts.values()))
    assert sum((c + 1) // 2 for c in counts.values()) == sum(PLACE_SLOTS) == slot
    return logs, scalars, regions


def named_positions(total, B, tpb):
    """the slots of a round that the placement matrix names, by name: {name: [slots]}; a position the geometry does not have (no second
    workgroup, no full one) is left out"""
    nthr = (total + B - 1) // B
    out = {"lane 0 of wave 0": [0], "lane 63 of wave 0": [63], "lane 0 of a later wave": [64]}
    if nthr >= tpb:
        out["last lane of a workgroup"] = [tpb - 1]
        out["a whole workgroup"] = [k * nthr + t for k in range(B) for t in range(tpb) if k * nthr + t < total]
    if nthr > tpb:
        out["first thread of the second workgroup"] = [tpb]
    if nthr % tpb:
        out["last live thread of the partly filled last workgroup"] = [nthr - 1]
    out["a whole wave"] = [k * nthr + t for k in range(B) for t in range(64) if k * nthr + t < total]
    if B > 1:
        out["chain position 0 of thread 0"] = [0]
        out["chain position B - 1 of thread 0"] = [(B - 1) * nthr]
    return {k: v for k, v in out.items() if all(s < total for s in v)}


def assert_placement(hdr, classes):
    """the class coverage condition of one run over placement_input(), from the classes check_capture found in its capture:
      round 0: every slot at a named position (named_positions; whole wave and whole workgroup included) is P + P or P - P -- the bucket
        counts guarantee that under any order inside the buckets -- lane 0 of wave 0 and the round's last slot are P - P, and the
        classes generic, P + P, P - P and leftover all occur.  (A neutral OPERAND cannot occur in round 0: its operands are table
        entries, and a base that is the neutral element is flagged and never sorted.)
      rounds >= 1: each of O + Q, P + O, O + O and leftover O occurs, and at least one named single-slot position holds one of them.
        Which slot gets which of the four is the order's doing (the sums of a bucket of +-P are the same multiset in any order, their
        places are not), so no more than this can be demanded of every order; the patterns of placement_input give every fixed order
        all four.
    Returns {round: {position name: classes found there}} for the record."""
    ex = ("P+P", "P-P")
    total, B = hdr["total"][0], slots_per_thread(hdr["total"][0], hdr["aff_cap"], hdr["bmax"], hdr["bmin"])
    assert total == sum(PLACE_SLOTS) and B == hdr["bmin"], (total, B)
    names = named_positions(total, B, hdr["tpb"])
    must = {"lane 0 of wave 0", "lane 63 of wave 0", "lane 0 of a later wave", "a whole wave", "last live thread of the partly filled last workgroup"}
    if B == 1:
        must |= {"last lane of a workgroup", "first thread of the second workgroup", "a whole workgroup"}
    else:
        must |= {"chain position 0 of thread 0", "chain position B - 1 of thread 0"}
    assert must <= set(names), (sorted(must - set(names)), hdr["tpb"], B)
    for name, slots in names.items():
        if B > 1 and name == "a whole workgroup" and hdr["tpb"] > 64:
            continue  # (three slots per thread: only a workgroup of one wave lies inside the exceptional regions)
        ok = ex + ("leftover",) if name.startswith("a whole") else ex  # (a bucket of 33 ends in a leftover: no addition either)
        bad = [(s, classes[0][s]) for s in slots if classes[0][s] not in ok]
        assert not bad, ("placement", "round 0", name, bad[:4])
    assert classes[0][0] == "P-P" and classes[0][total - 1] == "P-P"
    assert {"generic", "P+P", "P-P", "leftover"} <= set(classes[0]), ("placement", "round 0 lacks", {"generic", "P+P", "P-P", "leftover"} - set(classes[0]))
    later = set().union(*[set(c) for c in classes[1:]])
    assert set(O_CLASSES) <= later, ("placement", "rounds >= 1 lack", sorted(set(O_CLASSES) - later))
    found = {}
    for r in range(1, len(classes)):
        t = hdr["total"][r]
        pos = named_positions(t, slots_per_thread(t, hdr["aff_cap"], hdr["bmax"], hdr["bmin"]), hdr["tpb"])
        found[r] = {name: sorted({classes[r][s] for s in slots}) for name, slots in pos.items()}
    assert any(len(v) == 1 and v[0] in O_CLASSES for f in found.values() for name, v in f.items() if not name.startswith("a whole")), ("placement", found)
    return found


# ---- a synthetic capture: the pipeline run by the restatements themselves, the points from the oracle ---------------------------

def synthetic_capture(hdr, base_logs, scalars, rng, ra, mulgen=None):
    """the blob-shaped arrays a correct pipeline would leave for (hdr, scalars), with the items of every bucket in an order drawn from
    rng: what check_capture must accept"""
    mg = mulgen or Mulgen()
    nk = hdr["nkeys"]
    mem = membership(hdr, scalars)
    cnt = [sum(mem[k].values()) if k in mem else 0 for k in range(nk)]
    off = sort_offsets(cnt)
    items = [0xDEADBEEF] * off[-1]
    for k in range(nk):
        lst = sorted(mem[k].elements()) if k in mem else []
        rng.shuffle(lst)
        items[off[k]:off[k] + len(lst)] = lst
        if len(lst) & 1:
            items[off[k] + len(lst)] = NONE
    hdr = dict(hdr, ra=ra, items_len=off[-1], max_cnt=max(cnt), total=[], share=[0] * ra)
    rounds, c_in, o_in, in_logs = [], cnt, off, None
    for r in range(ra):
        c_out, o_out = halve(c_in)
        total = o_out[-1]
        desc = [] if r == 0 else (desc_dense(c_in, o_in, o_out) if hdr["dense"] else desc_words(c_in, o_in, o_out))
        out_logs = [0] * total
        for a, b, dst in round_slots(hdr, r, items if r == 0 else desc, total):
            la = item_log(hdr, a, base_logs) if r == 0 else in_logs[a]
            lb = 0 if b is None else (item_log(hdr, b, base_logs) if r == 0 else in_logs[b])
            out_logs[dst] = (la + lb) % R
        pts = np.frombuffer(b"".join(mg.words(x) for x in out_logs), dtype="<u4").reshape(total, 16)
        rounds.append(dict(ocnt=np.array(c_out, dtype=np.uint32), ooff=np.array(o_out, dtype=np.uint32), desc=np.array(desc, dtype=np.uint32), pts=pts))
        hdr["total"].append(total)
        c_in, o_in, in_logs = c_out, o_out, out_logs
    bkt = np.zeros((nk, 24), dtype=np.uint32)
    for k in range(nk):
        lk = sum(item_log(hdr, w, base_logs) for w in items[off[k]:off[k] + cnt[k]]) % R
        if lk == 0:
            bkt[k, 0] = 1  # (1, 0, 0)
        else:
            bkt[k, :16] = np.frombuffer(mg.words(lk), dtype="<u4")
            bkt[k, 16] = 1
    cap = Capture(hdr, np.array(cnt, dtype=np.uint32), np.array(off, dtype=np.uint32), np.array(items, dtype=np.uint32), rounds, bkt)
    bucket_logs = [sum(item_log(hdr, w, base_logs) for w in items[off[k]:off[k] + cnt[k]]) % R for k in range(nk)]
    synthetic_merge_tail(cap, bucket_logs, mg)
    return cap


def synthetic_merge_tail(cap, bucket_logs, mg):
    """the sections behind bkt as a correct merge tree and tail would leave them, into cap: the levels in lambda-projective coordinates
    with Z != 1 for most points (x Z, (x + y / x) Z, Z), the neutral element as (1, 1, 0).  hdr["tail"], ["enc"], ["rule"] are the
    caller's; ["group"] too if given (else 1 lane per addition)"""
    hdr = cap.hdr
    signed, c = bool(hdr["flavour"] & 2), hdr["c"]
    hdr["levels"] = c - 1 if signed else c
    hdr.setdefault("group", [1] * hdr["levels"])
    hdr.setdefault("tail", 0 if signed else (3 if tail_shape(hdr)[0] * c > 32 else 2))
    hdr.setdefault("enc", 0)
    hdr.setdefault("rule", 0)
    per_level, logs = [], [x % R for x in bucket_logs]
    for j in range(hdr["levels"]):
        logs, _ = merge_level(logs, j)
        per_level.append(logs)
    distinct = sorted({x for lv in per_level for x in lv if x})
    xy = {k: (int.from_bytes(mg.words(k)[:32], "little"), int.from_bytes(mg.words(k)[32:], "little")) for k in distinct}
    lam = {0: np.array(list(int_to_words(1)) * 2 + [0] * 8, dtype=np.uint32)}
    for k, xi in zip(distinct, batch_inverse([xy[k][0] for k in distinct])):
        x, y = xy[k]
        z = 1 if k % 5 == 0 else ((k >> 7) & ((1 << 233) - 1)) | 1
        lam[k] = np.concatenate([int_to_words(co.gf_mul(x, z)), int_to_words(co.gf_mul(x ^ co.gf_mul(y, xi), z)), int_to_words(z)])
    cap.levels = [np.array([lam[x] for x in lv], dtype=np.uint32) for lv in per_level]
    cap.save0 = cap.bkt[0].copy() if signed else None

    def ld(k):
        if k == 0:
            return np.array(list(int_to_words(1)) + [0] * 16, dtype=np.uint32)
        return np.concatenate([np.frombuffer(mg.words(k), dtype="<u4"), int_to_words(1)])

    pts = tail_points(hdr, logs, bucket_logs[0])
    if hdr["tail"] == 3:
        parts = [add_tree(pts[g:g + 16])[0] for g in range(0, len(pts), 16)]
        hdr["nparts"] = len(parts)
        cap.parts = np.array([ld(k) for k in parts], dtype=np.uint32)
        total = add_tree(parts)[0]
    else:
        hdr["nparts"], cap.parts = 0, None
        total = add_tree(pts)[0]
    cap.res_xy = np.frombuffer(mg.words(total), dtype="<u4").copy()
    cap.res_inf = 1 if total == 0 else 0
    cap.res_enc = encode_point(total, hdr["rule"], mg) if hdr["enc"] else None


# ---- placed inputs for the merge tree and the tails: one base per bucket, the bucket's logarithm chosen ----------------------------
# With one item per bucket no pair round runs and the leftover route is a gather (k_bucket_gather_items): bucket k of the array the merge
# tree starts from IS the chosen point.  What the tree and the tails then meet -- P + P, P - P, neutral operands, and in which lane
# group -- is decided by sums over sub-blocks of the chosen logarithms, so it is laid out here and proven on the logarithms alone
# (assert_merge_placement, assert_tail_placement) before a device sees it.

def plan_windows(flavour, c):
    """(W, n_narrow, nkeys) as the library plans them: flavour 3 fixed-base signed digits, 1 fixed-base tau-adic (one overflow window),
    0 one-shot (overflow windows up to 240 digits, a bucket set per window)"""
    W, nn = window_split(c)
    if flavour == 1:
        W += 1
    elif flavour == 0:
        W += (240 - 234 + c - 1) // c
    return W, nn, (1 << (c - 1) if flavour == 3 else (1 << c if flavour == 1 else W << c))


def placeable_windows(flavour, c):
    """the windows a placed scalar may target: signed digits -- the first full-width one (a key shifted there is that window's digit and
    nothing else), fixed-base tau-adic too (one bucket set; the key is the pattern); one-shot -- every window but the top two real ones
    and the overflow windows (sum_t d_t lambda^(o_w + t) mod r re-expands to other digits up there)"""
    W, nn = window_split(c)
    return [nn] if flavour & 1 else list(range(W - 2))


def placed_scalars(flavour, c, bucket_logs):
    """(base_logs, scalars, keys) that put exactly the point bucket_logs[key] x G into bucket `key` (0 = the bucket stays empty): one base
    and one scalar per populated bucket.
      signed digits: scalar key << o_w (key 0: 2^(c-1) << o_w, the magnitude that shares bucket 0) for the full-width window w, base
        logarithm v 2^(-o_w): the table row w holds 2^(o_w) P;
      tau-adic:      scalar sum_t d_t lambda^(o_w + t) mod r; one-shot: key = (w << c) | d, base logarithm v (the item is the base
        itself); fixed-base: key = d through the full-width window w, base logarithm v lambda^(-o_w): row w holds lambda^(o_w) P.
    Every scalar's window property is asserted with the recoding restated above / the oracle's tau-adic digits."""
    W, nn, nk = plan_windows(flavour, c)
    assert len(bucket_logs) == nk
    starts, ok_w = window_starts(c, W, nn), set(placeable_windows(flavour, c))
    logs, scalars, keys = [], [], []
    for key, v in enumerate(bucket_logs):
        v %= R
        if v == 0:
            continue
        if flavour == 3:
            w = nn
            assert window_widths(c, W, nn)[w] == c
            x = (key if key else 1 << (c - 1)) << starts[w]
            digits = [d for _, d in signed_recode(x, c)]
            assert x < R and digits[w] > 0 and signed_key(digits[w], c) == key and not any(d for i, d in enumerate(digits) if i != w), (key, digits)
            logs.append(v * pow(2, -starts[w], R) % R)
        else:
            w, d = key >> c, key & ((1 << c) - 1)
            if flavour == 1:  # one bucket set for all windows: the key is the pattern, placed through the full-width window nn
                w, d = nn, key
            assert d and w in ok_w, ("no scalar reaches bucket", key)
            x = pattern_weight(d, starts[w])
            assert tau_windows(x, c, W, nn) == [d if i == w else 0 for i in range(W)], ("the tau-adic digits of the placed scalar", key)
            logs.append(v * pow(LAMBDA, -starts[w], R) % R if flavour == 1 else v)
        scalars.append(x)
        keys.append(key)
    return logs, scalars, keys


def node_comp(logs, base, size, s):
    """component s of the node (sub-block) logs[base : base + size]: s = 0 its total, s = 1 + t the sum of its entries whose index inside
    the node has bit t set -- what slot s of the node holds once the tree has merged it"""
    return sum(v for i, v in enumerate(logs[base:base + size]) if s == 0 or (i >> (s - 1)) & 1) % R


def set_node_comp(logs, base, size, s, value):
    """makes component s of the node `value` and leaves its other components alone: entry 0 alone moves the total; entry 2^t moves
    component 1 + t and the total, entry 0 takes the total back"""
    d = (value - node_comp(logs, base, size, s)) % R
    if s == 0:
        logs[base] = (logs[base] + d) % R
    else:
        logs[base + (1 << (s - 1))] = (logs[base + (1 << (s - 1))] + d) % R
        logs[base] = (logs[base] - d) % R


def apply_merge_wish(logs, j, blk, s, cls, side="R"):
    """makes addition (blk, s) of merge level j the class `cls` by moving one component of its right operand's node (side 'L': of the
    left one's): the operands are component s of the two halves of block blk"""
    h = 1 << j
    L, Rb = blk * 2 * h, blk * 2 * h + h
    if cls in ("O+Q", "O+O"):
        set_node_comp(logs, L, h, s, 0)
    if cls in ("P+O", "O+O"):
        set_node_comp(logs, Rb, h, s, 0)
    if cls in ("P+P", "P-P"):
        sign = 1 if cls == "P+P" else -1
        if side == "R":
            set_node_comp(logs, Rb, h, s, sign * node_comp(logs, L, h, s))
        else:
            set_node_comp(logs, L, h, s, sign * node_comp(logs, Rb, h, s))


def merge_placed_logs(flavour, c, variant, seed=77):
    """bucket logarithms for the merge tree: random (every addition generic) except where this schedule asks otherwise.  X = P + P
    (variants "pp", "o0") or P - P (variant "mm").  Additions are numbered a = block (j + 1) + slot as the kernel numbers them.
      level 0 (bucket pairs):  a = 0 and the last addition X; a = 4 .. 7 P + P, P - P, P + O, generic (one wave of rows of 16 lanes,
                               neighbouring groups of a wave of quads); a = 12 O + Q, a = 13 O + O, a = 15 P + P (the last row of a
                               workgroup of rows), a = 16 O + O with buckets 36 .. 39 empty too; a = 255, 256 X where the level has them
                               (the last lane of one workgroup and the first of the next, one lane per addition);
      level 1:                 a = 0 X ("pp": the level's block 0 has an exceptional slot 0; "mm": its left operand vanished at level 0, so
                               the P - P at addition 0 is level 2's), the last addition X, a = 8 .. 11 P + P, P - P, P + O, generic,
                               a = 15 and a = 31 P + P (slot j; the last row of a workgroup of rows, the last quad of one of quads), a = 32
                               P + P (slot 0, the first group of a wave); blocks 6, 8, 9 meet the empty buckets: P + O, O + Q, O + O;
      level 2:                 a = 0 X in "mm";
      levels >= 1 with four blocks or more (signed digits): the last addition P + P ("pp") or P - P ("o0"; "mm" too, but for level 2) --
                               at 1 024 buckets level 2's is the last live lane of a half-filled workgroup of single lanes.
    "o0" is "pp" with bucket 0 empty: addition 0 of level 0 -- the lane that keeps bucket 0 aside -- is O + Q.  The tau-adic flavours keep
    pattern 0 of every window empty, and nothing is placed where placeable_windows() says no scalar reaches."""
    import random

    rnd = random.Random(seed + 1000 * c + flavour)
    W, nn, nk = plan_windows(flavour, c)
    logs = [rnd.randrange(1, R) for _ in range(nk)]
    X = "P-P" if variant == "mm" else "P+P"
    # one-shot: the schedule starts at bucket `at` = 64, behind the narrow low windows (their upper patterns are no buckets), and `live`
    # ends where placeable_windows() does; 64 buckets are whole workgroups of rows at levels 0 and 1, so the lane groups stay as described
    at = 0 if flavour else 64
    live = nk if flavour else len(placeable_windows(0, c)) << c
    for i in (24, 27, 32, 33, 36, 37, 38, 39):
        logs[at + i] = 0
    forced = set()
    if flavour != 3:  # pattern 0 of a window and the top bit of a narrow window are no buckets of the tau-adic flavours; the unplaceable windows stay empty
        widths = window_widths(c, W, nn)
        forced = {i for i in range(nk) if i >= live or not i & ((1 << c) - 1) or (i & ((1 << c) - 1)) >> widths[i >> c]}
    for i in forced:
        logs[i] = 0
    a0, a1, a2 = at >> 1, at >> 1, (at >> 3) * 3  # the additions of levels 0, 1, 2 in front of bucket `at`
    wishes = [(0, a0, 0, X), (0, live // 2 - 1, 0, X if flavour == 3 else "generic"), (0, a0 + 4, 0, "P+P"), (0, a0 + 5, 0, "P-P"), (0, a0 + 6, 0, "P+O"), (0, a0 + 15, 0, "P+P")]
    if live // 2 > 256:
        wishes += [(0, 255, 0, X), (0, 256, 0, X)]
    b1 = a1 // 2
    wishes += [(1, b1 + 4, 0, "P+P"), (1, b1 + 4, 1, "P-P"), (1, b1 + 5, 0, "P+O"), (1, b1 + 7, 1, "P+P", "L"), (1, b1 + 15, 1, "P+P", "L"), (1, b1 + 16, 0, "P+P")]
    wishes.append((2, a2 // 3, 0, X) if variant == "mm" else (1, b1, 0, X))
    # the last addition of the levels behind level 0, by its left operand (the right one holds the lower levels' last additions): "mm"
    # leaves level 2 alone, where the P - P of level 0 has emptied the right operand; "o0" takes P - P from level 1 on
    for j in range(1, (c - 1 if flavour == 3 else c)):
        if flavour == 3 and not (variant == "mm" and j == 2) and (live >> (j + 1)) >= 4:  # (the left operand of a level of two blocks starts in the middle: additions 255, 256)
            wishes.append((j, (live >> (j + 1)) - 1, j, "P+P" if variant == "pp" else "P-P", "L"))
    for w in sorted(wishes, key=lambda t: (t[0], t[1], t[2])):
        apply_merge_wish(logs, *w)
    if variant == "o0":
        logs[0] = 0
    assert not any(logs[i] for i in forced if not (at <= i < at + 2)), "a wish moved a bucket no scalar reaches"
    for i in forced:  # (the one-shot flavour has no addition 0 to place: bucket `at` is a pattern 0)
        logs[i] = 0
    return logs


def merge_classes(flavour, c, bucket_logs):
    """the classes of every addition of every merge level, by the restatement alone: merge[j][a]"""
    logs, out = [x % R for x in bucket_logs], []
    for j in range(c - 1 if flavour == 3 else c):
        logs, adds = merge_level(logs, j)
        out.append([classify(l, r) for l, r in adds])
    return out


MERGE_CONDITIONS = ("classes", "addition 0", "save0", "last addition", "groups", "neighbours", "slots")


def assert_merge_placement(runs, require=MERGE_CONDITIONS, require_first=None):
    """the class coverage of the merge tree over `runs` = [(group, merge)], group[j] = lanes per addition of level j (the capture
    header's), merge[j][a] = the class of addition a (check_capture's).  For every instantiation k_merge<GROUP, FIRST> that occurs
    (FIRST = level 0), over all its levels of all runs -- a condition not in `require` is not demanded (a shape that cannot reach it):
      classes        all six classes occur;
      addition 0     P + P and P - P occur at addition 0 of a level;
      save0          FIRST only: addition 0 -- the lane that keeps bucket 0 aside -- once with bucket 0 populated, once with it neutral;
      last addition  P + P and P - P occur at the last addition of a level whose last workgroup is partly filled;
      groups         GROUP > 1: P + P in the first group of a wave and in the last group of a workgroup;
      neighbours     GROUP > 1: four neighbouring groups of one wave hold P + P, P - P, an addition with a neutral operand and a generic one;
      slots          not FIRST: P + P at slot 0 (the lane that also stores T_right) and at slot j; a level-1 block with an exceptional slot 0.
    Returns {(GROUP, FIRST): {condition: where it was met}}; a missing class fails."""
    inst = {}
    for group, merge in runs:
        for j, cls in enumerate(merge):
            inst.setdefault((group[j], j == 0), []).append((j, cls))
    found = {}
    require_all, require_1st = require, require if require_first is None else require_first
    for (G, first), lst in sorted(inst.items()):
        f = found[(G, first)] = {}
        require = require_1st if first else require_all
        if first and G > 1:
            # level 0 of 2^(c-1) >= 128 buckets fills whole workgroups of quads and of rows, and the one-shot flavour's last live addition
            # lies in the overflow windows, which no scalar reaches: no shape has a placeable last addition in a partly filled workgroup here
            require = tuple(x for x in require if x != "last addition")
        per_wg, per_wave = 256 // G, 64 // G
        where = lambda want, pick: [(j, a) for j, cls in lst for a in pick(j, cls) if cls[a] in want]  # noqa: E731
        seen = {x for _, cls in lst for x in cls}
        f["classes"] = sorted(seen)
        if "classes" in require:
            assert set(MERGE_CLASSES) <= seen, ("merge placement", G, first, "classes missing", sorted(set(MERGE_CLASSES) - seen))
        for name, pick in (("addition 0", lambda j, cls: [0]), ("last addition", lambda j, cls: [len(cls) - 1] if len(cls) % per_wg else [])):
            f[name] = {x: where((x,), pick)[:2] for x in ("P+P", "P-P")}
            if name in require:
                assert all(f[name].values()), ("merge placement", G, first, name, f[name])
        if first:
            f["save0"] = {"populated": where(("P+P", "P-P", "P+O", "generic"), lambda j, cls: [0])[:1], "neutral": where(("O+Q", "O+O"), lambda j, cls: [0])[:1]}
            if "save0" in require:
                assert all(f["save0"].values()), ("merge placement", G, first, "save0", f["save0"])
        if G > 1:
            f["groups"] = {"first of a wave": where(("P+P",), lambda j, cls: range(0, len(cls), per_wave))[:2],
                           "last of a workgroup": where(("P+P",), lambda j, cls: range(per_wg - 1, len(cls), per_wg))[:2]}
            if "groups" in require:
                assert all(f["groups"].values()), ("merge placement", G, first, "groups", f["groups"])
            f["neighbours"] = [(j, a) for j, cls in lst for a in range(len(cls) - 3) if a // per_wave == (a + 3) // per_wave
                               and {"P+P", "P-P", "generic"} < set(cls[a:a + 4]) and set(cls[a:a + 4]) & {"O+Q", "P+O", "O+O"}][:2]
            if "neighbours" in require:
                assert f["neighbours"], ("merge placement", G, first, "no wave holds the four kinds side by side")
        if not first:
            f["slots"] = {"slot 0": where(("P+P",), lambda j, cls: range(0, len(cls), j + 1))[:2], "slot j": where(("P+P",), lambda j, cls: range(j, len(cls), j + 1))[:2],
                          "level 1 slot 0": [(j, a) for j, a in where(("P+P", "P-P"), lambda j, cls: range(0, len(cls), j + 1)) if j == 1][:2]}
            if "slots" in require:
                assert all(f["slots"].values()), ("merge placement", G, first, "slots", f["slots"])
    return found


# ---- placed inputs for the tails -------------------------------------------------------------------------------------------------

TAIL_VARIANTS = ("a", "b", "c", "z")


def tail_targets(flavour, c, variant, seed=91):
    """the logarithms E[i] the tail is to add up (tail_points' order), random except:
      "a"  first pair P + P, the next two pairs O + Q and P + O, the last pair of the first level P - P;
      "b"  first pair P - P, the next pair O + O, the last pair P + P;
      "c"  as "a" with the last point neutral (signed digits: bucket 0 empty);
      "z"  a neutral result: one point is minus the sum of the others.
    The one-shot flavour (W c points in groups of 16) starts this at point 16, behind the narrow windows, and gives the pair (0, 1) and
    the last pair of group 1 the same two classes; its last placeable pair ends where placeable_windows() does -- the last pair of the
    single-workgroup tail's first level lies in the overflow windows and stays neutral.  In every variant: group 5 is sixteen neutral points; group 6 is {x, -x, neutral ..}: a neutral sum
    through P - P; groups 8 and 9 hold one point each with EQUAL images and groups 10 and 11 one each with OPPOSITE images (lambda^k of
    different k applied to different points): k_tail(-4) meets P + P and P - P between group sums."""
    import random

    rnd = random.Random(seed + 100 * c + flavour)
    W, nn, _ = plan_windows(flavour, c)
    n = c if flavour & 1 else W * c
    live = n if flavour & 1 else len(placeable_windows(0, c)) * c
    at = 0 if flavour & 1 else 16
    E = [rnd.randrange(1, R) if i < live else 0 for i in range(n)]
    if not flavour & 1:  # a narrow window has no top digit
        for w in range(nn):
            E[w * c + c - 1] = 0
        for i in range(80, 96):
            E[i] = 0
        for g, i, v in ((6, 0, 5), (6, 1, -5), (8, 3, 7), (9, 7, 7), (10, 1, 9), (11, 12, -9)):
            for k in range(16 * g, 16 * g + 16):
                E[k] = 0 if k != 16 * g + i and (g != 6 or k > 16 * g + 1) else E[k]
            E[16 * g + i] = v * E[0] % R
    last = live // 2 - 1  # the last pair of the first level that is a pair of placeable points
    if variant in ("a", "c"):
        E[at + 1], E[at + 2], E[at + 5], E[2 * last + 1] = E[at], 0, 0, R - E[2 * last]
        if variant == "c":
            E[live - 1] = 0
        if at:  # the very first pair, and the last pair of the group the schedule starts in
            E[1], E[at + 15] = E[0], R - E[at + 14]
    elif variant == "b":
        E[at + 1], E[at + 2], E[at + 3], E[2 * last + 1] = R - E[at], 0, 0, E[2 * last]
        if at:
            E[1], E[at + 15] = R - E[0], E[at + 14]
    elif variant == "z":
        E[at + 4] = 0
        E[at + 4] = -sum(E) % R
    return E


def tail_placed_logs(flavour, c, E, seed=92):
    """bucket logarithms, random where a scalar reaches, whose merged array A makes the tail's points the E of tail_targets: bit sum t of
    window w is moved to E[w c + t] / 2^t (signed; bucket 0 is E[c - 1] / 2^(c-1)) or E[w c + t] / lambda^k by the one bucket 2^t"""
    import random

    rnd = random.Random(seed + 100 * c + flavour)
    W, nn, nk = plan_windows(flavour, c)
    Wt, nnt = (1, 0) if flavour & 1 else (W, nn)
    widths = [c - 1] if flavour == 3 else ([c] if flavour == 1 else window_widths(c, W, nn))
    size = 1 << (c - 1 if flavour == 3 else c)
    logs = [0] * nk
    for w in (range(Wt) if flavour & 1 else placeable_windows(0, c)):
        for d in range(1, 1 << widths[w]):
            logs[w * size + d] = rnd.randrange(1, R)
        for t in range(widths[w]):
            k = t if flavour == 3 else w * c - min(w, nnt) + t
            want = E[w * c + t] * pow(2 if flavour == 3 else LAMBDA, -k, R)
            i = w * size + (1 << t)
            logs[i] = (logs[i] + want - node_comp(logs, w * size, size, 1 + t)) % R
    if flavour == 3:
        logs[0] = E[c - 1] * pow(2, -(c - 1), R) % R
    return logs


def merged_array(flavour, c, bucket_logs):
    """the array the last merge level leaves, on logarithms"""
    logs = [x % R for x in bucket_logs]
    for j in range(c - 1 if flavour == 3 else c):
        logs, _ = merge_level(logs, j)
    return logs


TAIL_CONDITIONS = ("empty slot", "first pair", "last pair", "neutral operands", "parity", "bucket 0", "result", "groups")


def assert_tail_placement(runs, require=TAIL_CONDITIONS):
    """the class coverage of ONE tail shape over `runs` = [check_capture's tail dict] (or tail_restated's); a condition not in `require`
    is not demanded:
      empty slot        a point that is neutral before it is doubled or mapped (signed digits: a bit slot, not bucket 0);
      first pair        P + P and P - P at the first pair of the first level of an add tree (shape 3: of a group's);
      last pair         P + P and P - P at the last PAIR of that level (an odd count's leftover is no pair; shape 3: pair 7 of a full group);
      neutral operands  O + Q, P + O and O + O occur in a tree;
      parity            an odd and an even point count (signed digits);
      bucket 0          signed digits: bucket 0 populated and bucket 0 empty;
      result            a finite result and a neutral one;
      groups            shape 3: a partly filled last group, a group of 16 neutral points, a group with live points whose sum is neutral
                        through P - P, two neighbouring group sums that are equal and two that are opposite (P + P / P - P in the
                        first level of k_tail(-4)'s tree).
    Returns {condition: what met it}."""
    shape = runs[0]["shape"]
    assert all(t["shape"] == shape for t in runs)
    signed = shape in (0, 1)
    f = {}
    firsts, lasts, every = [], [], []
    for t in runs:
        trees = t["groups"] if shape == 3 else [t["tree"]]
        counts = [min(16, len(t["points"]) - 16 * g) for g in range(len(trees))] if shape == 3 else [len(t["points"])]
        for lv, n in zip(trees, counts):
            if lv:
                firsts.append(lv[0][0])
                if shape != 3 or n == 16:
                    lasts.append(lv[0][n // 2 - 1])
            every += [x for level in lv for x in level]
        if shape == 3:
            every += [x for level in t["tree"] for x in level]
    f["empty slot"] = [i for t in runs for i, v in enumerate(t["points"][:-1] if signed else t["points"]) if v == 0][:3]
    f["first pair"], f["last pair"] = sorted(set(firsts) & {"P+P", "P-P"}), sorted(set(lasts) & {"P+P", "P-P"})
    f["neutral operands"] = sorted(set(every) & {"O+Q", "P+O", "O+O"})
    f["parity"] = sorted({len(t["points"]) & 1 for t in runs})
    f["bucket 0"] = sorted({t["points"][-1] != 0 for t in runs}) if signed else None
    f["result"] = sorted({t["total"] != 0 for t in runs})
    want = {"empty slot": bool(f["empty slot"]), "first pair": len(f["first pair"]) == 2, "last pair": len(f["last pair"]) == 2,
            "neutral operands": len(f["neutral operands"]) == 3, "parity": len(f["parity"]) == 2 or not signed,
            "bucket 0": not signed or len(f["bucket 0"]) == 2, "result": len(f["result"]) == 2}
    if shape == 3:
        g = f["groups"] = {"partly filled": [], "neutral": [], "P-P": [], "equal": [], "opposite": []}
        for t in runs:
            pts = t["points"]
            if len(pts) % 16:
                g["partly filled"].append(len(pts) % 16)
            for k, lv in enumerate(t["groups"]):
                grp = pts[16 * k:16 * k + 16]
                if len(grp) == 16 and not any(grp):
                    g["neutral"].append(k)
                if any(grp) and t["parts"][k] == 0 and any("P-P" in level for level in lv):
                    g["P-P"].append(k)
            g["equal"] += [i for i, x in enumerate(t["tree"][0]) if x == "P+P"]
            g["opposite"] += [i for i, x in enumerate(t["tree"][0]) if x == "P-P"]
        want["groups"] = all(g.values())
    for name in require:
        if name in want:
            assert want[name], ("tail placement", TAILS[shape], name, f.get(name))
    return f
