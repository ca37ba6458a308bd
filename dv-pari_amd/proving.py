"""Host mirror of src/proving.rs: Proof (to_bits/from_bits), Transcript challenge, and Proof::prove
driven through the GPU prover context (dvp_prover_* / dvp_prove in include/dvpari.h)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import fr
from ._native import lib, check, ptr
from .gnark_r1cs import R1CSInstance

P = fr.P


@dataclass
class Proof:
    """src/proving.rs:40-50"""
    commit_p: bytes  # 30
    kzg_k: bytes     # 30
    a0: bytes        # 29 = 232 LE bits (FrBits)
    b0: bytes

    def to_bytes(self) -> bytes:
        return self.commit_p + self.kzg_k + self.a0 + self.b0

    @staticmethod
    def from_bytes(b: bytes):
        assert len(b) == 118
        return Proof(b[:30], b[30:60], b[60:89], b[89:118])

    def to_bits(self):
        """Proof::to_bits, src/proving.rs:691-718 (LE bit order inside each byte)."""
        return [(byte >> i) & 1 for byte in self.to_bytes() for i in range(8)]

    @staticmethod
    def from_bits(bits):
        """Proof::from_bits, src/proving.rs:721-770."""
        assert len(bits) == 944
        by = bytes(sum(bits[8 * i + j] << j for j in range(8)) for i in range(118))
        return Proof.from_bytes(by)

    @staticmethod
    def prove(cache_dir, public_inputs, private_inputs) -> "Proof":
        """Proof::prove(cache_dir, public_inputs, private_inputs), src/proving.rs:426-688, with the reference's own
        signature: the R1CS dump and the SRS point files are read from cache_dir on the first call and stay in HBM
        (dvp_prove_cache_dir); release_cache_dir() frees them."""
        import os

        pub = _fr_arg(public_inputs)
        prv = _fr_arg(private_inputs)
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove_cache_dir(os.fspath(cache_dir).encode(), ptr(pub), pub.shape[0], ptr(prv), prv.shape[0], ptr(out)),
              "dvp_prove_cache_dir")
        return Proof.from_bytes(out.tobytes())

    @staticmethod
    def prove_ark(cache_dir, public_ark, private_ark) -> "Proof":
        """Proof.prove with both vectors as arkworks holds them in memory (uint64 [n, 4] of a * 2^256 mod p, fr.to_ark): they are
        converted on the GPU, in the prover's witness buffer (dvp_prove_cache_dir_ark)"""
        import os

        pub, prv = fr._ark_arg(public_ark, "prove_ark"), fr._ark_arg(private_ark, "prove_ark")
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove_cache_dir_ark(os.fspath(cache_dir).encode(), ptr(pub) if pub.shape[0] else None, pub.shape[0],
                                          ptr(prv) if prv.shape[0] else None, prv.shape[0], ptr(out)), "dvp_prove_cache_dir_ark")
        return Proof.from_bytes(out.tobytes())

    @staticmethod
    def prove_witness_file(cache_dir, num_public_inputs: int, witness_path=None):
        """load_witness_from_file + Proof::prove in one call (dvp_prove_cache_dir_witness_file): the witness file (None =
        cache_dir/witness_to_dvsnark) is mapped and its elements are reduced mod p on the GPU.  Returns (Proof, public_inputs as
        uint64 [num_public_inputs, 4])."""
        import os

        out = np.zeros(118, dtype=np.uint8)
        pub = np.zeros((max(num_public_inputs, 1), 4), dtype=np.uint64)
        wp = None if witness_path is None else os.fspath(witness_path).encode()
        check(lib.dvp_prove_cache_dir_witness_file(os.fspath(cache_dir).encode(), num_public_inputs, wp, ptr(out), ptr(pub)),
              "dvp_prove_cache_dir_witness_file")
        return Proof.from_bytes(out.tobytes()), pub[:num_public_inputs]

    @staticmethod
    def prove_multi(cache_dirs, public_inputs, private_inputs) -> list:
        """one witness, one proof per verifier: cache_dirs[0] is the primary directory (circuit and its own SRS), every further
        directory the SRS of another verifier, loaded into a slot of the primary's prover (add_srs_dir).  Phase 1 runs once
        (dvp_prove_cache_dir_multi).  Returns a list in the order of cache_dirs: a Proof, or the DvpError of that verifier's slot."""
        primary, slots = _multi_dirs(cache_dirs, len(_fr_arg(public_inputs)))
        pub, prv = _fr_arg(public_inputs), _fr_arg(private_inputs)
        out, st = np.zeros((len(slots), 118), dtype=np.uint8), np.zeros(len(slots), dtype=np.int32)
        check(lib.dvp_prove_cache_dir_multi(primary, pub.shape[0], ptr(slots), len(slots), ptr(pub) if pub.shape[0] else None,
                                            ptr(prv) if prv.shape[0] else None, prv.shape[0], ptr(out), ptr(st)), "dvp_prove_cache_dir_multi")
        return _multi_results(out, st, "dvp_prove_cache_dir_multi")

    @staticmethod
    def prove_multi_witness_file(cache_dirs, num_public_inputs: int, witness_path=None):
        """prove_multi from a witness file (None = cache_dirs[0]/witness_to_dvsnark; dvp_prove_cache_dir_multi_witness_file): returns
        (list of Proof or DvpError, public_inputs as uint64 [num_public_inputs, 4])"""
        import os

        primary, slots = _multi_dirs(cache_dirs, num_public_inputs)
        out, st = np.zeros((len(slots), 118), dtype=np.uint8), np.zeros(len(slots), dtype=np.int32)
        pub = np.zeros((max(num_public_inputs, 1), 4), dtype=np.uint64)
        wp = None if witness_path is None else os.fspath(witness_path).encode()
        check(lib.dvp_prove_cache_dir_multi_witness_file(primary, num_public_inputs, ptr(slots), len(slots), wp, ptr(out), ptr(st), ptr(pub)),
              "dvp_prove_cache_dir_multi_witness_file")
        return _multi_results(out, st, "dvp_prove_cache_dir_multi_witness_file"), pub[:num_public_inputs]

    def a0_fr(self):
        v = int.from_bytes(self.a0, "little")
        return (v, True) if v < P else (0, False)  # FrBits::to_fr, src/curve.rs:43-59

    def b0_fr(self):
        v = int.from_bytes(self.b0, "little")
        return (v, True) if v < P else (0, False)


def _fr_arg(v) -> np.ndarray:
    a = v if isinstance(v, np.ndarray) else (fr.vec(v) if len(v) else np.zeros((0, 4), dtype=np.uint64))
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def _raw_arg(v) -> np.ndarray:
    """_fr_arg for the witness check: python ints below 2^256 become limbs as they are, NOT reduced mod p"""
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
    from ._native import ints_to_limbs

    return ints_to_limbs([int(x) for x in v]) if len(v) else np.zeros((0, 4), dtype=np.uint64)


def _expand_slots(slots, live) -> np.ndarray:
    """the `slots` argument of the prove_multi forms as uint32: None = every slot of `live` (the non-empty slots, in index order)"""
    if slots is None:
        slots = list(live)
    elif isinstance(slots, (str, bytes)) or not hasattr(slots, "__iter__"):
        raise TypeError("slots must be a sequence of slot indices or None")
    vals = [int(k) for k in slots]
    if any(k < 0 or k >= 1 << 32 for k in vals):
        raise ValueError("a slot index is a uint32")
    return np.array(vals, dtype=np.uint32)


def _multi_results(proofs, status, where) -> list:
    """per slot: the Proof, or the DvpError of its status (returned, not raised: the other slots' proofs stand)"""
    from ._native import DvpError

    proofs = np.asarray(proofs, dtype=np.uint8).reshape(-1, 118)
    return [Proof.from_bytes(proofs[j].tobytes()) if int(s) == 0 else DvpError(int(s), f"{where}[{j}]") for j, s in enumerate(status)]


def _dirs_arg(cache_dirs) -> list:
    """a non-empty list / tuple of directories as bytes; a single path is refused (it would be read as its characters)"""
    import os

    if isinstance(cache_dirs, (str, bytes, os.PathLike)) or not isinstance(cache_dirs, (list, tuple)):
        raise TypeError("cache_dirs must be a list of directories, the primary first")
    if not cache_dirs:
        raise ValueError("cache_dirs is empty")
    return [os.fspath(d).encode() if not isinstance(d, bytes) else d for d in cache_dirs]


def _multi_dirs(cache_dirs, num_public_inputs: int):
    """(primary directory, slots as uint32): slot 0 for the primary, add_srs_dir's slot for every further directory"""
    dirs = _dirs_arg(cache_dirs)
    slots = [0] + [add_srs_dir(dirs[0], num_public_inputs, d) if d != dirs[0] else 0 for d in dirs[1:]]
    return dirs[0], np.array(slots, dtype=np.uint32)


def add_srs_dir(cache_dir, num_public_inputs: int, srs_dir) -> int:
    """dvp_cache_dir_add_srs_dir: the five SRS point files of srs_dir (another verifier's SRS for the same circuit) into a new slot of the
    prover Proof.prove(cache_dir, ..) keeps; returns the slot (the one it already has when srs_dir was added before)"""
    import os

    k = C.c_uint32(0)
    cd = cache_dir if isinstance(cache_dir, bytes) else os.fspath(cache_dir).encode()
    sd = srs_dir if isinstance(srs_dir, bytes) else os.fspath(srs_dir).encode()
    check(lib.dvp_cache_dir_add_srs_dir(cd, num_public_inputs, sd, C.byref(k)), "dvp_cache_dir_add_srs_dir")
    return int(k.value)


def set_cache_dir_slot_binding(cache_dir, num_public_inputs: int, slot: int, srs_hash=None, circuit_hash=None, bind_srs: bool = False):
    """dvp_cache_dir_slot_set_binding: set_cache_dir_binding for one SRS slot of cache_dir's prover"""
    import os

    ks, s = _hash_arg(srs_hash, "srs_hash")
    kc, c = _hash_arg(circuit_hash, "circuit_hash")
    check(lib.dvp_cache_dir_slot_set_binding(os.fspath(cache_dir).encode(), num_public_inputs, slot, s, c, int(bool(bind_srs))),
          "dvp_cache_dir_slot_set_binding")


def release_cache_dir(cache_dir=None):
    """drop the prover(s) dvp_prove_cache_dir keeps for cache_dir (None: all)"""
    import os

    lib.dvp_cache_dir_release(None if cache_dir is None else os.fspath(cache_dir).encode())


PREP_WROTE_TREE2N, PREP_WROTE_BAR_WTS, PREP_WROTE_Z_VALS2INV, PREP_Z_POLY_NOT_MONIC = 0x1, 0x2, 0x4, 0x8
PREP_BAD_Z_POLY, PREP_BAD_BAR_WTS, PREP_BAD_Z_VALS2INV, PREP_BAD_TREE2N = 0x100, 0x200, 0x400, 0x800


def prover_prepares_precomputes(cache_dir, validate_precompute: bool = False) -> int:
    """prover_prepares_precomputes, src/proving.rs:225-325, through the C entry of the same name: needs z_poly in
    cache_dir (its length fixes m), reads tree2n or writes a minimal one, produces bar_wts and z_vals2inv when they are
    missing -- from the isogeny chain in milliseconds.  The GPU prover itself regenerates all of these on the device and
    reads none of the files; this exists so that a cache_dir prepared here is complete for a reference prover as well.
    validate_precompute: z_poly must vanish on D (the reference's asserts, :281-296) and every file found is compared
    with the regenerated values.  Returns the PREP_* report bits; a failed validation raises ValueError naming the file."""
    import os

    rep = C.c_uint32(0)
    rc = lib.dvp_prover_prepares_precomputes(os.fspath(cache_dir).encode(), int(bool(validate_precompute)), C.byref(rep))
    bad = [n for n, b in (("z_poly", PREP_BAD_Z_POLY), ("bar_wts", PREP_BAD_BAR_WTS), ("z_vals2inv", PREP_BAD_Z_VALS2INV),
                          ("tree2n", PREP_BAD_TREE2N)) if rep.value & b]
    if bad:
        msg = "vanishing poly does not evaluate to zero at all points in domain" if bad == ["z_poly"] else "differs from the regenerated values"
        raise ValueError(f"{cache_dir}: {', '.join(bad)}: {msg} (first bad index {lib.dvp_last_error_index()})")
    check(rc, "dvp_prover_prepares_precomputes")
    return rep.value


def _hash_arg(h, name):
    """a 32-byte hash (or None) as an array that outlives the call, and the pointer to pass"""
    if h is None:
        return None, None
    b = bytes(h)
    if len(b) != 32:
        raise ValueError(f"{name} must be 32 bytes")
    a = np.frombuffer(b, dtype=np.uint8).copy()
    return a, ptr(a)


def transcript_challenge(commit_p: bytes, public_inputs, srs_hash=None, circuit_hash=None) -> int:
    """Transcript::output, src/proving.rs:164-197.  srs_hash / circuit_hash: the binding (dvp_transcript_challenge_bound); None is
    BLAKE3(""), what the reference hashes."""
    cp = np.frombuffer(commit_p, dtype=np.uint8).copy()
    pub = fr.vec(public_inputs) if len(public_inputs) else np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    ks, s = _hash_arg(srs_hash, "srs_hash")
    kc, c = _hash_arg(circuit_hash, "circuit_hash")
    check(lib.dvp_transcript_challenge_bound(ptr(cp), ptr(pub), len(public_inputs), s, c, ptr(out)), "dvp_transcript_challenge_bound")
    return fr.to_int(out)


def blake3(data: bytes) -> bytes:
    d = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    check(lib.dvp_blake3(ptr(d), len(data), ptr(out)), "dvp_blake3")
    return out.tobytes()


def blake3_dev(d_ptr: int, nbytes: int, stream: int = 0) -> bytes:
    """BLAKE3 of nbytes at the device address d_ptr (any byte alignment; 0 is allowed for nbytes = 0), chunk-parallel on the GPU
    (dvp_blake3_dev).  The call itself only enqueues on `stream`; this wrapper then waits for the 32 bytes."""
    import torch

    out = torch.empty(32, dtype=torch.uint8, device="cuda")
    check(lib.dvp_blake3_dev(d_ptr or None, nbytes, out.data_ptr(), stream or None), "dvp_blake3_dev")
    if stream:
        torch.cuda.ExternalStream(stream).synchronize()
    else:
        torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


def set_cache_dir_binding(cache_dir, num_public_inputs: int, srs_hash=None, circuit_hash=None, bind_srs: bool = False):
    """dvp_cache_dir_set_binding: Prover.set_transcript_binding for the prover(s) Proof.prove(cache_dir, ..) keeps; bind_srs with
    srs_hash None binds the opened prover's own Prover.srs_hash()"""
    import os

    ks, s = _hash_arg(srs_hash, "srs_hash")
    kc, c = _hash_arg(circuit_hash, "circuit_hash")
    check(lib.dvp_cache_dir_set_binding(os.fspath(cache_dir).encode(), num_public_inputs, s, c, int(bool(bind_srs))), "dvp_cache_dir_set_binding")


def circuit_hash_cache_dir(cache_dir, num_public_inputs: int) -> bytes:
    """dvp_circuit_hash_cache_dir: Prover.circuit_hash() from <cache_dir>/r1cs_to_dvsnark alone -- the verifier's way to the value.
    The prover Proof.prove(cache_dir, ..) keeps for the directory is used when it is open; otherwise one without SRS is built from
    the dump and destroyed"""
    import os

    out = np.zeros(32, dtype=np.uint8)
    check(lib.dvp_circuit_hash_cache_dir(os.fspath(cache_dir).encode(), num_public_inputs, ptr(out)), "dvp_circuit_hash_cache_dir")
    return out.tobytes()


@dataclass
class WitnessReport:
    """dvp_witness_report with its two lists: rows = [{"row", "a", "b", "c", "i"}] (ints; a*b != c + i mod p for each), the first
    failing rows in row order; wires = [(wire, n_terms)], the first suspect wires in wire order (at least one term in a failing row,
    none in a satisfied one).  first_* are -1 when there is none."""
    n_unsat: int
    first_unsat: int
    n_noncanonical: int
    first_noncanonical: int
    n_suspect_wires: int
    constant_wire_is_one: bool
    rows: list
    wires: list

    @property
    def ok(self) -> bool:
        """satisfied, canonical, and the constant wire is 1"""
        return self.n_unsat == 0 and self.n_noncanonical == 0 and self.constant_wire_is_one


def _check_witness(call, max_rows: int, max_wires: int, where: str) -> WitnessReport:
    """call(rows, rows_cap, wires, wires_cap, report) -> status: one of the dvp_*check_witness* entries behind its own leading arguments"""
    from ._native import UnsatRow, SuspectWire, WitnessReport as Rep

    rows = (UnsatRow * max_rows)() if max_rows else None
    wires = (SuspectWire * max_wires)() if max_wires else None
    rep = Rep()
    check(call(rows, max_rows, wires, max_wires, C.byref(rep)), where)
    val = lambda limbs: sum(int(x) << (64 * k) for k, x in enumerate(limbs))
    return WitnessReport(int(rep.n_unsat), int(rep.first_unsat), int(rep.n_noncanonical), int(rep.first_noncanonical),
                         int(rep.n_suspect_wires), bool(rep.constant_wire_is_one),
                         [{"row": int(r.row), "a": val(r.a), "b": val(r.b), "c": val(r.c), "i": val(r.i)} for r in rows[:rep.n_rows_listed]] if rows else [],
                         [(int(w.wire), int(w.n_terms)) for w in wires[:rep.n_wires_listed]] if wires else [])


def check_witness_file(cache_dir, num_public_inputs: int, witness_path=None, max_rows: int = 16, max_wires: int = 16) -> WitnessReport:
    """dvp_check_witness_cache_dir_witness_file: Prover.check_witness_be32 on a witness file (None = cache_dir/witness_to_dvsnark), on the
    prover Proof.prove(cache_dir, ..) keeps when it is open, else on one built from the dump without SRS and destroyed"""
    import os

    wp = None if witness_path is None else os.fspath(witness_path).encode()
    return _check_witness(lambda *tail: lib.dvp_check_witness_cache_dir_witness_file(os.fspath(cache_dir).encode(), num_public_inputs, wp, *tail),
                          max_rows, max_wires, "dvp_check_witness_cache_dir_witness_file")


TRACE_SCALARS, TRACE_DIGESTS, TRACE_POINTS, TRACE_ALL = 0x1, 0x2, 0x4, 0x7  # DVP_TRACE_*
TRACE_MISMATCH_COMMIT, TRACE_MISMATCH_KZG = 0x1, 0x2


def _trace_record(t) -> dict:
    """a dvp_prove_trace as a plain dict: header fields and scalars as ints, a point as {"x", "y", "inf", "enc"}, a digest as 32 bytes
    under the name src/proving.rs gives its vector ("evals2.i", "k_scalar_r", ..)"""
    from . import _native as nat

    rec = {f: int(getattr(t, f)) for f in nat.TRACE_HEADER}
    for f in nat.TRACE_SCALARS:
        rec[f] = sum(int(x) << (64 * k) for k, x in enumerate(getattr(t, f)))
    for f in nat.TRACE_POINTS:
        pt = getattr(t, f)
        rec[f] = {"x": sum(int(x) << (64 * k) for k, x in enumerate(pt.xy[:4])), "y": sum(int(x) << (64 * k) for k, x in enumerate(pt.xy[4:])),
                  "inf": int(pt.inf), "enc": bytes(pt.enc)}
    for f, name in nat.TRACE_DIGESTS:
        rec[name] = bytes(getattr(t, f))
    return rec


def format_prove_trace(rec) -> str:
    """one prove-trace record as text, one `name = hex` line per field (what examples/dvp_prove_cli --trace prints): header words as
    eight hex digits, scalars and coordinates as big-endian hex numbers, flags as two hex digits, encodings and digests byte by byte"""
    from . import _native as nat

    lines = [f"{f} = {rec[f]:08x}" for f in nat.TRACE_HEADER]
    lines += [f"{f} = {rec[f]:064x}" for f in nat.TRACE_SCALARS]
    for f in nat.TRACE_POINTS:
        pt = rec[f]
        lines += [f"{f}_x = {pt['x']:064x}", f"{f}_y = {pt['y']:064x}", f"{f}_inf = {pt['inf']:02x}", f"{f}_enc = {pt['enc'].hex()}"]
    lines += [f"{name} = {rec[name].hex()}" for _, name in nat.TRACE_DIGESTS]
    return "\n".join(lines)


def parse_prove_trace(text: str) -> dict:
    """format_prove_trace's (and the CLI's) lines back into a record; lines without ` = ` are skipped"""
    from . import _native as nat

    vals = dict(ln.split(" = ") for ln in text.splitlines() if " = " in ln)
    rec = {f: int(vals[f], 16) for f in nat.TRACE_HEADER + nat.TRACE_SCALARS}
    for f in nat.TRACE_POINTS:
        rec[f] = {"x": int(vals[f + "_x"], 16), "y": int(vals[f + "_y"], 16), "inf": int(vals[f + "_inf"], 16),
                  "enc": bytes.fromhex(vals[f + "_enc"].strip())}
    for _, name in nat.TRACE_DIGESTS:
        rec[name] = bytes.fromhex(vals[name].strip())
    return rec


def _trace_last(handle, parts: int, stream: int = 0) -> dict:
    from ._native import ProveTrace

    t = ProveTrace()
    check(lib.dvp_prover_trace_last(handle, parts, C.byref(t), stream or None), "dvp_prover_trace_last")
    return _trace_record(t)


def trace_cache_dir(cache_dir, num_public_inputs: int, parts: int = TRACE_ALL) -> dict:
    """Prover.trace_last on the prover Proof.prove(cache_dir, ..) keeps for the directory (dvp_cache_dir_prover): the stages of the last
    proof made from cache_dir.  The handle is borrowed and the call does not take a turn: do not prove from cache_dir on another thread
    meanwhile."""
    import os

    h = C.c_void_p()
    check(lib.dvp_cache_dir_prover(os.fspath(cache_dir).encode(), num_public_inputs, C.byref(h)), "dvp_cache_dir_prover")
    return _trace_last(h, parts)


class Prover:
    """The artefacts Proof::prove reads from cache_dir (R1CS dump, SRS point vectors, TREE_2N and the
    prover precomputes, src/proving.rs:435-511,562-565,666-672), loaded once and kept in HBM."""

    def __init__(self, inst: R1CSInstance):
        self.inst = inst
        self.m = inst.num_constraints
        self.log_m = self.m.bit_length() - 1
        h = C.c_void_p()
        check(lib.dvp_prover_create(self.log_m, inst.num_public_inputs, inst.n_wires, C.byref(h)), "dvp_prover_create")
        self._h = h
        check(lib.dvp_prover_set_coeffs(h, ptr(inst.coeffs), inst.coeffs.shape[0]), "dvp_prover_set_coeffs")
        for which, mat in enumerate((inst.l, inst.r, inst.o)):
            check(lib.dvp_prover_set_matrix(h, which, inst.n_rows, ptr(mat.row_ptr), ptr(mat.wire), ptr(mat.coeff)),
                  "dvp_prover_set_matrix")

    @staticmethod
    def of_cache_dir(cache_dir, num_public_inputs: int, m: int) -> "Prover":
        """the prover Proof.prove(cache_dir, ..) keeps for cache_dir (opened if need be): a borrowed handle for
        inspection (debug reads, MSM plans), released by release_cache_dir, never closed from here"""
        import os

        self = Prover.__new__(Prover)
        self.inst, self.m, self.log_m, self._borrowed = None, m, m.bit_length() - 1, True
        h = C.c_void_p()
        check(lib.dvp_cache_dir_prover(os.fspath(cache_dir).encode(), num_public_inputs, C.byref(h)), "dvp_cache_dir_prover")
        self._h = h
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                lib.dvp_prover_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- SRS -------------------------------------------------------------------------------------
    def set_srs(self, srs):
        for which, (xy, inf) in enumerate(srs.as_list()):
            xy = np.ascontiguousarray(xy, dtype=np.uint64)
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            check(lib.dvp_prover_set_srs_affine(self._h, which, ptr(xy), ptr(inf), xy.shape[0]), "dvp_prover_set_srs_affine")

    def set_srs_encoded(self, which: int, enc: np.ndarray):
        """payload of a reference point-vector file (n x 30 bytes, src/io_utils.rs:83-111)"""
        e = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 30)
        check(lib.dvp_prover_set_srs_encoded(self._h, which, ptr(e), e.shape[0]), "dvp_prover_set_srs_encoded")

    # ---- SRS slots: one SRS per verifier on one prover (include/dvpari.h, dvp_prover_srs_slot_*) ------------
    def add_srs(self, srs_or_encoded=None) -> int:
        """a new SRS slot (or a dropped index reused); not selected.  srs_or_encoded: an SRS (set_srs) or the five encoded payloads
        [g_m, g_q, g_k_0, g_k_1, g_k_2] (set_srs_encoded), loaded into the slot; None leaves it empty"""
        k = C.c_uint32(0)
        check(lib.dvp_prover_srs_slot_add(self._h, C.byref(k)), "dvp_prover_srs_slot_add")
        slot = int(k.value)
        self._dropped_slots().discard(slot)
        if srs_or_encoded is not None:
            back = self.active_srs()
            self.select_srs(slot)
            try:
                if hasattr(srs_or_encoded, "as_list"):
                    self.set_srs(srs_or_encoded)
                else:
                    for which, enc in enumerate(srs_or_encoded):
                        self.set_srs_encoded(which, enc)
            finally:
                self.select_srs(back)
        return slot

    def _dropped_slots(self) -> set:
        if not hasattr(self, "_dropped"):
            self._dropped = set()
        return self._dropped

    def select_srs(self, slot: int):
        """make `slot` the active one: every other method (set_srs, prove, srs_hash, msm_plan, set_table_budget, ..) acts on it"""
        check(lib.dvp_prover_srs_slot_select(self._h, slot), "dvp_prover_srs_slot_select")

    def active_srs(self) -> int:
        return int(lib.dvp_prover_srs_slot_active(self._h))

    def srs_slots(self) -> list:
        """the slot indices in use (handed out and not dropped through this object), in index order"""
        return [k for k in range(int(lib.dvp_prover_srs_slot_count(self._h))) if k not in self._dropped_slots()]

    def drop_srs(self, slot: int):
        """free the slot's bases and tables; the index is reused by a later add_srs.  The active slot cannot be dropped"""
        check(lib.dvp_prover_srs_slot_drop(self._h, slot), "dvp_prover_srs_slot_drop")
        self._dropped_slots().add(int(slot))

    def srs_slot_bytes(self, slot: int):
        """(bases, tables): bytes of HBM the slot holds now (tables are built by its first proof)"""
        b, t = C.c_uint64(0), C.c_uint64(0)
        check(lib.dvp_prover_srs_slot_bytes(self._h, slot, C.byref(b), C.byref(t)), "dvp_prover_srs_slot_bytes")
        return int(b.value), int(t.value)

    def _multi(self, slots, call, where) -> list:
        sl = _expand_slots(slots, self.srs_slots())
        n = len(sl)
        out, st = np.zeros((max(n, 1), 118), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
        check(call(ptr(sl) if n else None, n, ptr(out), ptr(st)), where)
        return _multi_results(out[:n], st[:n], where)

    def prove_multi(self, public_inputs, private_inputs, slots=None) -> list:
        """one witness, one proof per SRS slot: phase 1 once, the MSMs and the challenge phase per slot (dvp_prove_multi).  slots:
        the slot indices in the order wanted (None = every slot in use).  Returns a list: a Proof, or the DvpError of a slot that
        could not be proven (the others stand); a failure of the witness itself (DVP_EUNSAT, ..) raises"""
        pub, prv = _fr_arg(public_inputs), _fr_arg(private_inputs)
        return self._multi(slots, lambda s, n, out, st: lib.dvp_prove_multi(self._h, s, n, ptr(pub) if pub.shape[0] else None, pub.shape[0],
                                                                           ptr(prv) if prv.shape[0] else None, prv.shape[0], out, st),
                           "dvp_prove_multi")

    def prove_multi_be32(self, raw, slots=None) -> list:
        """prove_multi from the witness as its file holds it (prove_be32's argument; dvp_prove_multi_be32)"""
        a = fr._be32_arg(raw)
        return self._multi(slots, lambda s, n, out, st: lib.dvp_prove_multi_be32(self._h, s, n, ptr(a) if a.shape[0] else None, a.shape[0], out, st),
                           "dvp_prove_multi_be32")

    def prove_multi_dev(self, d_assignment: int, slots=None, stream: int = 0) -> list:
        """prove_multi with the assignment already in HBM (prove_dev's argument; dvp_prove_multi_dev)"""
        return self._multi(slots, lambda s, n, out, st: lib.dvp_prove_multi_dev(self._h, s, n, d_assignment, out, st, stream),
                           "dvp_prove_multi_dev")

    def srs_hash(self) -> bytes:
        """BLAKE3 of to_bytes() of g_k[0], g_k[1], g_k[2], g_q, g_m in that order (the stream Transcript::srs_hash would hash,
        src/proving.rs:91-101), encoded and hashed on the device; depends on the codec rule in force (dvp_prover_srs_hash)"""
        out = np.zeros(32, dtype=np.uint8)
        check(lib.dvp_prover_srs_hash(self._h, ptr(out)), "dvp_prover_srs_hash")
        return out.tobytes()

    def circuit_hash(self) -> bytes:
        """BLAKE3 of the stream Transcript::circuit_info_hash would hash (src/proving.rs:111-134) on the instance with the Vandermonde
        terms (src/gnark_r1cs.rs:333-386): per row the coeff_ids of A, B, C and the Vandermonde ids as u32 LE (no wire ids), then
        the updated coefficient table as a count and 29-byte entries; generated and hashed on the device (dvp_prover_circuit_hash).
        Needs the coefficients and the matrices, no SRS"""
        out = np.zeros(32, dtype=np.uint8)
        check(lib.dvp_prover_circuit_hash(self._h, ptr(out)), "dvp_prover_circuit_hash")
        return out.tobytes()

    def set_transcript_binding(self, srs_hash=None, circuit_hash=None):
        """bind this prover's challenges to (srs_hash, circuit_hash): the transcript's compile-time half becomes
        H(srs_hash || circuit_hash), None = BLAKE3(""); (None, None) restores the reference's constant"""
        ks, s = _hash_arg(srs_hash, "srs_hash")
        kc, c = _hash_arg(circuit_hash, "circuit_hash")
        check(lib.dvp_prover_set_transcript_binding(self._h, s, c), "dvp_prover_set_transcript_binding")

    # ---- domain data -------------------------------------------------------------------------------
    def domains(self):
        d = np.zeros((self.m, 4), dtype=np.uint64)
        d2 = np.zeros((self.m, 4), dtype=np.uint64)
        check(lib.dvp_prover_domains(self._h, ptr(d), ptr(d2)), "dvp_prover_domains")
        return d, d2

    def domain_tables(self, which: int):
        a = np.zeros((self.m, 4), dtype=np.uint64)
        b = np.zeros((self.m, 4), dtype=np.uint64)
        check(lib.dvp_prover_domain_tables(self._h, which, ptr(a), ptr(b)), "dvp_prover_domain_tables")
        return a, b

    def vanish_at(self, which: int, x: int) -> int:
        """Z_D(x) / Z_D'(x) through the isogeny chain"""
        from .ec_fft import FFTree  # noqa: F401  (same chain as dvp_ecfft_vanish_at, on the prover's own tree)
        if not hasattr(self, "_tree"):
            self._tree = FFTree(2 * self.m)
        out = np.zeros(4, dtype=np.uint64)
        check(lib.dvp_ecfft_vanish_at(self._tree._h, which, ptr(fr.limbs(x)), ptr(out)), "dvp_ecfft_vanish_at")
        return fr.to_int(out)

    # ---- prove -------------------------------------------------------------------------------------
    def prove(self, public_inputs, private_inputs) -> Proof:
        """Proof::prove(cache_dir, public_inputs, private_inputs), src/proving.rs:426-688."""
        pub, prv = _fr_arg(public_inputs), _fr_arg(private_inputs)
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove(self._h, ptr(pub), pub.shape[0], ptr(prv), prv.shape[0], ptr(out)), "dvp_prove")
        return Proof.from_bytes(out.tobytes())

    def prove_be32(self, raw) -> Proof:
        """the same from the witness as its file holds it (gnark_r1cs.read_witness_raw): at least n_wires elements of
        [1, public.., private..], 32 big-endian bytes each, reduced mod p on the GPU (dvp_prove_be32)"""
        a = fr._be32_arg(raw)
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove_be32(self._h, ptr(a) if a.shape[0] else None, a.shape[0], ptr(out)), "dvp_prove_be32")
        return Proof.from_bytes(out.tobytes())

    def prove_ark(self, public_ark, private_ark) -> Proof:
        """prove with both vectors as arkworks holds them in memory (uint64 [n, 4] of a * 2^256 mod p, fr.to_ark): converted on the
        GPU, in place in the witness buffer (dvp_prove_ark)"""
        pub, prv = fr._ark_arg(public_ark, "prove_ark"), fr._ark_arg(private_ark, "prove_ark")
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove_ark(self._h, ptr(pub) if pub.shape[0] else None, pub.shape[0], ptr(prv) if prv.shape[0] else None,
                                prv.shape[0], ptr(out)), "dvp_prove_ark")
        return Proof.from_bytes(out.tobytes())

    # ---- the stages of the last proof -----------------------------------------------------------------------
    def trace_last(self, parts: int = TRACE_ALL, stream: int = 0) -> dict:
        """dvp_prover_trace_last: scalars, partial commitments and vector digests of this prover's last complete proof (the record of
        format_prove_trace); DvpError (DVP_EINVAL) when there is none.  Costs more than the proof; changes nothing a later proof reads."""
        return _trace_last(self._h, parts, stream)

    def prove_trace(self, public_inputs, private_inputs, parts: int = TRACE_ALL):
        """prove, then trace_last: (Proof, record)"""
        proof = self.prove(public_inputs, private_inputs)
        return proof, self.trace_last(parts)

    # ---- explain an unsatisfied witness (needs coefficients and matrices, no SRS) -------------------
    def check_witness(self, public_inputs, private_inputs, max_rows: int = 16, max_wires: int = 16) -> WitnessReport:
        """why prove(public_inputs, private_inputs) would answer DVP_EUNSAT: every failing row counted and the first max_rows listed
        with a, b, c, i; entries >= p counted; the first max_wires suspect wires (dvp_prover_check_witness).  Values may be any
        integers below 2^256; rows are evaluated on them reduced mod p."""
        pub, prv = _raw_arg(public_inputs), _raw_arg(private_inputs)
        return _check_witness(lambda *tail: lib.dvp_prover_check_witness(self._h, ptr(pub) if pub.shape[0] else None, pub.shape[0],
                                                                         ptr(prv) if prv.shape[0] else None, prv.shape[0], *tail),
                              max_rows, max_wires, "dvp_prover_check_witness")

    def check_witness_be32(self, raw, max_rows: int = 16, max_wires: int = 16) -> WitnessReport:
        """the same from the witness as its file holds it (at least n_wires elements of 32 big-endian bytes); element 0 is reported,
        not refused (dvp_prover_check_witness_be32)"""
        a = fr._be32_arg(raw)
        return _check_witness(lambda *tail: lib.dvp_prover_check_witness_be32(self._h, ptr(a) if a.shape[0] else None, a.shape[0], *tail),
                              max_rows, max_wires, "dvp_prover_check_witness_be32")

    def check_witness_dev(self, d_assignment: int, max_rows: int = 16, max_wires: int = 16, stream: int = 0) -> WitnessReport:
        """the same with the assignment [1, public.., private..] (n_wires x 4 uint64, any values) already in HBM"""
        return _check_witness(lambda *tail: lib.dvp_prover_check_witness_dev(self._h, d_assignment, *tail, stream),
                              max_rows, max_wires, "dvp_prover_check_witness_dev")

    def row_terms(self, which: int, row: int):
        """[(wire_id, coeff_id)] of row `row` of A / B / C (which = 0 / 1 / 2) from the resident matrices; [] for a padding row"""
        n = C.c_size_t(0)
        check(lib.dvp_prover_row_terms(self._h, which, row, None, None, 0, C.byref(n)), "dvp_prover_row_terms")
        if not n.value:
            return []
        w, c = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        check(lib.dvp_prover_row_terms(self._h, which, row, ptr(w), ptr(c), n.value, C.byref(n)), "dvp_prover_row_terms")
        return list(zip(w.tolist(), c.tolist()))

    def debug(self, name: str, n: int = None):
        if n is None:
            n = 1 if name in ("alpha", "a0", "b0", "i0", "r0") else (2 * self.m if name == "kr" else self.m)
        out = np.zeros((n, 4), dtype=np.uint64)
        check(lib.dvp_prover_debug_read(self._h, name.encode(), ptr(out), n), "dvp_prover_debug_read")
        return out

    def transcript_dev(self, commit_p: bytes, public_inputs):
        """(alpha, -Z_D(alpha)) from the DEVICE flavour of the transcript (k_transcript / k_zalpha): parity-test access"""
        pub = _fr_arg(public_inputs)
        cp = np.frombuffer(bytes(commit_p), dtype=np.uint8).copy()
        a, z = np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
        check(lib.dvp_prover_debug_transcript_dev(self._h, ptr(cp), ptr(pub) if pub.shape[0] else None, pub.shape[0], ptr(a), ptr(z)),
              "dvp_prover_debug_transcript_dev")
        return fr.to_int(a), fr.to_int(z)

    def force_alpha(self, alpha):
        """TEST ONLY (dvp_prover_debug_force_alpha): every later proof on this prover takes this alpha (an int below p) instead of
        the transcript's output -- the way to a challenge inside D u D', which the library refuses with DVP_ECHALLENGE; None clears it"""
        a = None if alpha is None else _raw_arg([alpha])
        check(lib.dvp_prover_debug_force_alpha(self._h, None if a is None else ptr(a)), "dvp_prover_debug_force_alpha")

    # ---- device-resident / phased flavours --------------------------------------------------------------
    def prove_dev(self, d_assignment: int, stream: int = 0) -> Proof:
        """assignment = [1, public.., private..] as n_wires x 4 uint64 already in HBM (device pointer)."""
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove_dev(self._h, d_assignment, ptr(out), stream), "dvp_prove_dev")
        return Proof.from_bytes(out.tobytes())

    def begin(self, d_assignment: int, stream: int = 0, need_extend: bool = True):
        check(lib.dvp_prove_begin_partial(self._h, d_assignment, int(need_extend), stream), "dvp_prove_begin")

    def extend_count(self) -> int:
        """3 (a, b, c'; i by Horner) or 4: the vectors Proof::extend_evals extends (src/proving.rs:410-422)"""
        return int(lib.dvp_prover_extend_count(self._h))

    def extend_vectors(self, mask: int, stream: int = 0):
        check(lib.dvp_prove_extend_vectors(self._h, mask, stream), "dvp_prove_extend_vectors")

    def extended_ptr(self, v: int) -> int:
        out = C.c_void_p()
        check(lib.dvp_prover_extended_ptr(self._h, v, C.byref(out)), "dvp_prover_extended_ptr")
        return out.value

    def mark_extended(self, v: int):
        check(lib.dvp_prove_mark_extended(self._h, v), "dvp_prove_mark_extended")

    def quotient(self, stream: int = 0):
        check(lib.dvp_prove_quotient(self._h, stream), "dvp_prove_quotient")

    def msm_size(self, which: int) -> int:
        return int(lib.dvp_prover_msm_size(self._h, which))

    def msm_plan(self, which: int):
        """(window bits, windows) of the fixed-base MSM `which`, (0, 0) before its first use"""
        c, w = C.c_int(0), C.c_int(0)
        check(lib.dvp_prover_msm_plan(self._h, which, C.byref(c), C.byref(w)), "dvp_prover_msm_plan")
        return c.value, w.value

    def msm_table(self, which: int):
        """(bytes of HBM, signed binary windows -- the default flavour -- ?) of the fixed-base tables of MSM `which`"""
        s = C.c_int(0)
        b = int(lib.dvp_prover_msm_table_bytes(self._h, which, C.byref(s)))
        return b, bool(s.value)

    def set_table_budget(self, nbytes):
        """the most HBM per device the fixed-base tables of this prover may hold (None = no limit, 0 = no tables); tables that no
        longer fit are released at once, the next proof follows the new plan (dvp_prover_set_table_budget)"""
        b = (1 << 64) - 1 if nbytes is None else min(int(nbytes), (1 << 64) - 1)
        check(lib.dvp_prover_set_table_budget(self._h, b), "dvp_prover_set_table_budget")

    def msm_coverage(self, which: int):
        """(covered, total, reason): leading bases of MSM `which` served from tables, its size, and why not all of it --
        0 not limited, 1 the budget, 2 an allocation the runtime refused (dvp_prover_msm_coverage)"""
        cov, tot, why = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        check(lib.dvp_prover_msm_coverage(self._h, which, C.byref(cov), C.byref(tot), C.byref(why)), "dvp_prover_msm_coverage")
        return int(cov.value), int(tot.value), int(why.value)

    def msm_partial(self, which: int, lo: int, hi: int, d_out_xy: int, d_out_inf: int, stream: int = 0):
        check(lib.dvp_prover_msm_partial(self._h, which, lo, hi, d_out_xy, d_out_inf, stream), "dvp_prover_msm_partial")

    def challenge(self, d_commit_xy: int, d_commit_inf: int, stream: int = 0):
        check(lib.dvp_prove_challenge(self._h, d_commit_xy, d_commit_inf, stream), "dvp_prove_challenge")

    def challenge_partial(self, d_commit_xy: int, d_commit_inf: int, d_range, k_range, d_record: int, stream: int = 0):
        """phase 2, part 1 of an index-sharded prove: this rank's slice of the barycentric sums (d_range of D) and the inverse
        denominators its K-scalar range needs -> a 128-byte record at d_record (dvp_prove_challenge_partial)"""
        check(lib.dvp_prove_challenge_partial(self._h, d_commit_xy, d_commit_inf, d_range[0], d_range[1], k_range[0], k_range[1], d_record, stream),
              "dvp_prove_challenge_partial")

    def challenge_finish(self, d_records: int, n_records: int, k_range, stream: int = 0):
        """part 2: a0 b0 i0 r0 from the records of all ranks, then the K scalars of k_range only"""
        check(lib.dvp_prove_challenge_finish(self._h, d_records, n_records, k_range[0], k_range[1], stream), "dvp_prove_challenge_finish")

    def finish(self, d_kzg_xy: int, d_kzg_inf: int, stream: int = 0) -> Proof:
        out = np.zeros(118, dtype=np.uint8)
        check(lib.dvp_prove_finish(self._h, d_kzg_xy, d_kzg_inf, ptr(out), stream), "dvp_prove_finish")
        return Proof.from_bytes(out.tobytes())
