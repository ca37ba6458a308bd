"""The MSM bucket pipeline restated stage by stage in plain Python, from the comments of csrc/msm.hip and its stage headers msm_*.cuh (not from their code), and the parser
of the stage capture (dvp_debug_msm_capture_arm / _fetch, include/dvpari_internal.h).  Nothing here touches a device.

Every base of a test is k_i G with a known k_i, so every point the pipeline ever holds has a known discrete logarithm modulo the group
order r (pyref.P): an item of the sorted list is +- 2^(o_w) k_i (signed windows), lambda^(o_w) k_i (tau-adic rows) or k_i (a one-shot
MSM: its windows have bucket sets of their own), a pair round's slot adds two logarithms, logarithm 0 is the neutral element and is
stored as (0, 0).  check_capture walks a capture with that and compares every array bit for bit:
  (a) cnt / off / items with the bucket membership and the sort's layout (even starts, the spare word of an odd bucket);
  (b) every round's counts, offsets and descriptor words with the bookkeeping;
  (c) every output slot of every round with the group law on logarithms, through c_oracle.k233_mulgen;
  (d) bkt[k], normalised, with the sum of the bucket's round-0 inputs.
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
HDR_WORDS = 104
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
    bkt [nkeys, 24] uint32"""

    def __init__(self, hdr, cnt, off, items, rounds, bkt):
        self.hdr, self.cnt, self.off, self.items, self.rounds, self.bkt = hdr, cnt, off, items, rounds, bkt

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
    assert hdr["magic"] == MAGIC and hdr["version"] == 1 and hdr["hdr_words"] == HDR_WORDS, hdr
    hdr["share"] = [int(x) for x in w[24:24 + hdr["ra"]]]
    hdr["total"] = [int(x) for x in w[64:64 + hdr["ra"]]]
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
    assert at[0] == len(w), "the blob is longer than its header says"
    return Capture(hdr, cnt, off, items, rounds, bkt)


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


def check_capture(cap, base_logs, scalars, inf=None, mulgen=None):
    """checks (a) to (d) of the module's docstring on one capture; base_logs[i] = the logarithm of base i of the whole base vector,
    scalars = this MSM's, as integers.  Returns (classes, bucket_logs): classes[r][s] = the class of slot s of round r, bucket_logs[k] =
    the logarithm of bucket k's sum.  An AssertionError names the stage, the round and the slot."""
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
        assert ld_to_affine_bytes(cap.bkt[k]) == mg.words(lk), ("leftovers", ROUTES[hdr["route"]], "bucket", k)
    return classes, bucket_logs


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
    return Capture(hdr, np.array(cnt, dtype=np.uint32), np.array(off, dtype=np.uint32), np.array(items, dtype=np.uint32), rounds, bkt)
