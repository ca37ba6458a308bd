"""Cases and the oracle stream of the circuit hash (dvp_prover_circuit_hash): what the commented-out body of
Transcript::circuit_info_hash would hash (src/proving.rs:111-134) on the instance update_to_include_vandermode_matrix_d leaves
(src/gnark_r1cs.rs:333-386).  The stream is built here from pyref.r1cs_with_vandermonde alone, by the two serialisation rules:

  row part          for every row, the coeff_id of every term of its A, B and C side, a u32 little-endian each (no wire ids);
  coefficient part  Vec<Fr>::serialize_uncompressed: the count as u64 little-endian, then 29 bytes little-endian per entry.

A case keeps its three matrices apart (each with its own n_rows <= m), as the prover holds them; the oracle sees the m rows they
make together, rows a matrix does not have being empty."""
import functools
import random
import struct

import pyref as o

P = o.P
CHUNK = 1024
WINDOWS = (None, 1, 2, 3)  # DVP_CIRCUIT_HASH_WINDOW in chunks; None = the default


class Case:
    def __init__(self, name, log_m, k, coeffs, mats, n_wires=None):
        self.name, self.log_m, self.m, self.k, self.coeffs = name, log_m, 1 << log_m, k, [int(c) % P for c in coeffs]
        self.mats = [[list(r) for r in mt] for mt in mats]  # three lists of rows of (wire, coeff_id)
        assert all(len(mt) <= self.m for mt in self.mats)
        used = [w for mt in self.mats for r in mt for w, _ in r]
        self.n_wires = n_wires or max([1 + k] + [w + 1 for w in used])
        assert all(c < len(self.coeffs) for mt in self.mats for r in mt for _, c in r)

    def rows(self):
        """the m rows the oracle sees: (A_i, B_i, C_i), empty where a matrix has no row i"""
        return [tuple(mt[i] if i < len(mt) else [] for mt in self.mats) for i in range(self.m)]

    def row_ptrs(self):
        out = []
        for mt in self.mats:
            rp = [0]
            for r in mt:
                rp.append(rp[-1] + len(r))
            out.append(rp)
        return out

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def domain(log_m):
    """D of a prover with 2^log_m constraints: the even leaves of the oracle's tree with 2^(log_m + 1) leaves"""
    return tuple(o.FFTree(log_m + 1).both_domains()[0])


def oracle_instance(case):
    rows2, coeffs2, m = o.r1cs_with_vandermonde(case.rows(), case.coeffs, list(domain(case.log_m)), case.k)
    assert m == case.m
    return rows2, coeffs2


def stream_of(rows2, coeffs2):
    """(stream, length of the row part)"""
    row_part = b"".join(struct.pack("<I", cid) for row in rows2 for side in row for _, cid in side)
    coeff_part = struct.pack("<Q", len(coeffs2)) + b"".join(int(c).to_bytes(29, "little") for c in coeffs2)
    return row_part + coeff_part, len(row_part)


@functools.lru_cache(maxsize=None)
def _stream_cached(name):
    return stream_of(*oracle_instance(BY_NAME[name]))


def stream(case):
    return _stream_cached(case.name)


@functools.lru_cache(maxsize=None)
def digest_by_name(name):
    return o.blake3(_stream_cached(name)[0])


def digest(case):
    return digest_by_name(case.name)


def closed_form(case):
    """i1, n1, N and the dword offset of every row (and of the end) by the issue's formulas"""
    n0 = len(case.coeffs)
    i1 = case.coeffs.index(P - 1) if P - 1 in case.coeffs else n0
    n1 = n0 if i1 < n0 else n0 + 1
    N = n1 + case.m * max(case.k - 1, 0)
    rps = case.row_ptrs()
    off = [sum(rp[min(i, len(rp) - 1)] for rp in rps) + case.k * i for i in range(case.m + 1)]
    return i1, n1, N, off


def straddled_edges(case, window):
    """(edges of `window`-chunk windows inside the stream that cut a row, edges that cut a 29-byte record), from byte counts"""
    s, row_bytes = stream(case)
    _, _, _, off = closed_form(case)
    starts = {4 * x for x in off}
    edges = range(window * CHUNK, len(s), window * CHUNK)
    in_row = [e for e in edges if e < row_bytes and e not in starts]
    in_rec = [e for e in edges if e > row_bytes + 8 and (e - row_bytes - 8) % 29 != 0]
    return in_row, in_rec


def random_rows(rng, n_rows, n_wires, n_coeffs, lo, hi):
    return [[(rng.randrange(n_wires), rng.randrange(n_coeffs)) for _ in range(rng.randint(lo, hi))] for _ in range(n_rows)]


def _toy(k):
    return Case(f"toy-k{k}", 3, k, o.TOY_COEFFS, [[list(r[q]) for r in o.TOY_ROWS] for q in range(3)], n_wires=8)


def _sized(target):
    """a stream of exactly `target` bytes: log_m 2, one public input, p - 1 not in the table (so it is appended), padded with terms"""
    log_m, k = 2, 1
    for n1 in range(3, 7):
        rest = target - 8 - 29 * n1
        if rest % 4 == 0:
            break
    nnz = rest // 4 - k * (1 << log_m)
    rng = random.Random(target)
    coeffs = [rng.randrange(1, P - 1) for _ in range(n1 - 1)]
    mats = [[[] for _ in range(3)] for _ in range(3)]
    for _ in range(nnz):
        mats[rng.randrange(3)][rng.randrange(3)].append((rng.randrange(6), rng.randrange(n1 - 1)))
    return Case(f"bytes-{target}", log_m, k, coeffs, mats, n_wires=6)


def _minus_one(name, coeffs):
    rng = random.Random(name)
    return Case(name, 3, 2, coeffs, [random_rows(rng, 6, 8, len(coeffs), 0, 3) for _ in range(3)], n_wires=8)


def _build():
    rng = random.Random(0xC1C)
    cases = [_toy(0), _toy(1), _toy(2), _toy(5)]
    cases += [_sized(1024), _sized(1025), _sized(2048)]
    cases += [_minus_one("m1-absent", [5, 7, 11]), _minus_one("m1-first", [P - 1, 5, 7]), _minus_one("m1-middle", [5, 7, P - 1, 11, 13]),
              _minus_one("m1-twice", [3, P - 1, 4, P - 1, 9])]
    # 0, 1, p - 1, p - 2 and 2^224 + .. have every kind of 29th byte; every entry is used by some term
    edge = [0, 1, P - 1, P - 2, (1 << 224) + 0x1234567, 0x7F << 224]
    cases.append(Case("coeff-values", 3, 2, edge, [[[(w % 8, (i + w) % len(edge)) for w in range(i % 3 + 1)] for i in range(7)] for _ in range(3)], n_wires=8))
    # three matrices of 9, 13 and 11 rows under m = 16: rows 13 .. 15 carry Vandermonde ids only; empty rows inside each matrix
    cases.append(Case("ragged-rows", 4, 3, [2, 3, 5, 7], [random_rows(rng, n, 10, 4, 0, 4) for n in (9, 13, 11)], n_wires=10))
    # B has no row at all, C has six rows and no term
    cases.append(Case("empty-matrices", 3, 2, [2, 3, 5], [random_rows(rng, 8, 8, 3, 0, 3), [], [[] for _ in range(6)]], n_wires=8))
    # one row of 300 terms: longer than a chunk, so it crosses a window edge at window = 1
    long_rows = random_rows(rng, 5, 8, 4, 0, 2)
    long_rows[2] = [(t % 8, t % 4) for t in range(300)]
    cases.append(Case("long-row", 3, 2, [9, 8, 7, 6], [random_rows(rng, 5, 8, 4, 1, 2), long_rows, random_rows(rng, 5, 8, 4, 0, 2)], n_wires=8))
    # 2^8 rows, 1 - 6 terms per row and matrix, three public inputs: tens of KB
    cases.append(Case("sparse-8", 8, 3, [rng.randrange(P) for _ in range(64)], [random_rows(rng, 256, 300, 64, 1, 6) for _ in range(3)], n_wires=300))
    # rows of one dword: 2^8 rows, one public input, no term at all, and the same with a term in every 50th row of A -- 256 dwords of
    # the row part then span more rows than a workgroup of the generator keeps offsets for (rows_spanned_by_256_dwords)
    cases.append(Case("ids-only", 8, 1, [4, 5], [[], [], []], n_wires=2))
    cases.append(Case("mostly-empty", 8, 1, [4, 5, 6], [[[(1, i % 3)] * (3 if i % 50 == 0 else 0) for i in range(256)], [[] for _ in range(40)], []], n_wires=2))
    return cases


def rows_spanned_by_256_dwords(case):
    """the most rows any aligned run of 256 dwords of the row part touches"""
    off = closed_form(case)[3]
    row_of = [i for i in range(case.m) for _ in range(off[i + 1] - off[i])]
    return max(row_of[min(g + 255, len(row_of) - 1)] - row_of[g] + 1 for g in range(0, len(row_of), 256))


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def toy_with_changed_coeff_id(k):
    """the toy circuit with ONE coeff_id changed (row 2 of A reads coefficient 0 instead of 1): another circuit, another hash"""
    c = _toy(k)
    assert c.mats[0][2] == [(4, 1)]
    c.mats[0][2] = [(4, 0)]
    c.name = f"toy-k{k}-changed"
    return c


def py_dump(rows, coeffs):
    """the R1CS dump of src/gnark_r1cs.rs:84-91 for rows of (l, r, o) term lists"""
    out = [struct.pack("<I", len(coeffs))] + [int(c).to_bytes(32, "big") for c in coeffs] + [struct.pack("<I", len(rows))]
    for l, r, oo in rows:
        out.append(struct.pack("<III", len(l), len(r), len(oo)))
        for part in (l, r, oo):
            for w, c in part:
                out.append(struct.pack("<II", w, c))
    return b"".join(out)
