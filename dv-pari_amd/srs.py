"""Host mirror of src/srs.rs: Trapdoor, SRS, verifier_runs_setup (in memory, and the cache_dir flavour that
reads the R1CS dump and writes the reference's SRS / precompute files) and verify.  Every vector stage runs
on the GPU through the C ABI; python ints only appear for the handful of trapdoor scalars."""
import os

from dataclasses import dataclass

import numpy as np

from . import curve, fr
from .gnark_r1cs import R1CSInstance, evaluate_monomial_basis_poly

P = fr.P


@dataclass
class Trapdoor:
    """src/srs.rs:41-50"""
    tau: int
    delta: int
    epsilon: int


@dataclass
class SRS:
    """src/srs.rs:30-39; bases as affine [n,8] uint64 + infinity masks."""
    g_m: tuple
    g_q: tuple
    g_k: tuple  # three (xy, inf) pairs

    def as_list(self):
        return [self.g_m, self.g_q, self.g_k[0], self.g_k[1], self.g_k[2]]


def srs_scalars(prover, inst: R1CSInstance, td: Trapdoor):
    """The scalars k with base = k*G for every SRS vector of an instance that exists only in python (bench.py's synthetic
    circuits, the tests): verifier_runs_setup + compute_srs_matrices, src/srs.rs:112-167,177-361 (Lagrange bases at tau through
    the barycentric formula, src/ec_fft.rs:340-390,424-450; accumulate_m_values, src/srs.rs:53-84).  ONE implementation since
    round 5: the device pipeline of dvp_setup_cache_dir (csrc/setup.hip: setup_scalars_core), fed this instance's CSR matrices
    through dvp_setup_scalars; rounds 1-4 orchestrated the same stages from here, vector by vector over the host-pointer seams
    (srs_scalars_hostside below keeps that route as the cross-check the tests compare against)."""
    import ctypes as C

    from ._native import lib, check, ptr

    assert td.tau % P and td.delta % P and td.epsilon % P  # src/srs.rs:199-201
    m = inst.num_constraints
    log_m = m.bit_length() - 1
    t, d, e = (fr.limbs(x) for x in (td.tau, td.delta, td.epsilon))
    mats = (inst.l, inst.r, inst.o)
    keep = [[np.ascontiguousarray(getattr(mt, f), dtype=np.uint32) for mt in mats] for f in ("row_ptr", "wire", "coeff")]
    arr = [(C.c_void_p * 3)(*[a.ctypes.data for a in col]) for col in keep]
    coeffs = np.ascontiguousarray(inst.coeffs, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros((inst.n_wires + 5 * m, 4), dtype=np.uint64)
    check(lib.dvp_setup_scalars(ptr(t), ptr(d), ptr(e), log_m, inst.num_public_inputs, inst.n_rows, inst.n_wires, ptr(coeffs), coeffs.shape[0],
                                arr[0], arr[1], arr[2], ptr(out), out.shape[0]), "dvp_setup_scalars")
    o = inst.n_wires
    return out[:o], out[o:o + m], [out[o + m:o + 2 * m], out[o + 2 * m:o + 3 * m], out[o + 3 * m:]]


def srs_scalars_hostside(prover, inst: R1CSInstance, td: Trapdoor):
    """rounds 1-4's orchestration of the same stages from python (every vector through the host-pointer seams): kept as the
    independent cross-check of srs_scalars / dvp_setup_cache_dir in the tests"""
    assert td.tau % P and td.delta % P and td.epsilon % P  # src/srs.rs:199-201
    m = inst.num_constraints
    d, d2 = prover.domains()
    bar, z2inv = prover.domain_tables(0)      # 1/Z_D'(D_i), 1/Z_D(D'_i)
    bard, z2dinv = prover.domain_tables(1)    # 1/Z_D''(D'_i), 1/Z_D'(D_i)
    z_tau = prover.vanish_at(0, td.tau)
    zd_tau = prover.vanish_at(1, td.tau)
    assert z_tau and zd_tau
    delta2 = td.delta * td.delta % P
    # L_i(tau) = Z(tau) / ((tau - s_i) Z'(s_i))
    l_tau = fr.scale(fr.mul(fr.batch_inverse(fr.scalar_sub(td.tau, d)), bar), z_tau)
    l_taud = fr.scale(fr.mul(fr.batch_inverse(fr.scalar_sub(td.tau, d2)), bard), zd_tau)
    l_taul = np.empty((2 * m, 4), dtype=np.uint64)  # unified domain, interleaved (src/ec_fft.rs:445-448)
    l_taul[0::2] = fr.scale(fr.mul(l_tau, z2dinv), zd_tau)
    l_taul[1::2] = fr.scale(fr.mul(l_taud, z2inv), z_tau)
    # m_j(tau, delta) = sum_i (A_ij + delta B_ij + delta^2 C'_ij) L_i(tau), C' = C - D (Vandermonde on the public wires)
    lt_rows = l_tau[: inst.n_rows]
    mv = fr.spmv(*_t(inst.l, inst.n_wires), inst.coeffs, lt_rows)
    mb = fr.spmv(*_t(inst.r, inst.n_wires), inst.coeffs, lt_rows)
    mc = fr.spmv(*_t(inst.o, inst.n_wires), inst.coeffs, lt_rows)
    m_vals = fr.axpy(fr.axpy(mv, td.delta, mb), delta2, mc)  # whole vectors on the GPU: n_wires is 2^23 for the SP1 circuit
    pw = np.zeros((m, 4), dtype=np.uint64)  # d_i^0
    pw[:, 0] = 1
    for j in range(inst.num_public_inputs):  # -d_i^j on wire 1+j of every row (src/gnark_r1cs.rs:333-386)
        m_vals[1 + j] = fr.limbs((fr.to_int(m_vals[1 + j]) - delta2 * fr.dot(pw, l_tau)) % P)
        pw = fr.mul(pw, d)
    g_m = fr.scale(m_vals, td.epsilon)
    g_q = fr.scale(l_taud, z_tau * delta2 % P * td.epsilon % P)
    g_k = [l_tau, fr.scale(l_tau, td.delta), fr.scale(l_taul, delta2)]
    return g_m, g_q, g_k


def verifier_runs_setup_cache_dir(td: Trapdoor, cache_dir, num_public_inputs: int, write_precomputes: bool = True,
                                  return_scalars: bool = False):
    """SRS::verifier_runs_setup(trapdoor, cache_dir, num_public_inputs, ..), src/srs.rs:177-361, as the reference
    runs it: ONE library call (dvp_setup_cache_dir, csrc/setup.hip) reads cache_dir/r1cs_to_dvsnark, computes the SRS
    scalars on the device, writes g_m, g_q, g_k_0..2 as point-vector files (compute_srs_matrices ->
    write_point_vec_to_file) and, with write_precomputes, the domain files a reference prover/verifier would otherwise
    spend hours on (z_poly, z_polyd, bar_wts, bar_wtsd, z_vals2inv, z_vals2dinv).
    Returns (instance, prover context with the SRS loaded from the files just written)."""
    import ctypes as C

    from . import artifacts as A, io_utils
    from ._native import lib, check, ptr
    from .proving import Prover

    os.makedirs(cache_dir, exist_ok=True)
    t, d, e = (fr.limbs(x) for x in (td.tau, td.delta, td.epsilon))
    scalars = None
    if return_scalars:  # the discrete logs of the bases just written (tests pin the proof's commitments with them)
        nw, lg = C.c_uint32(0), C.c_uint32(0)
        inst = R1CSInstance.from_dump_file(os.path.join(cache_dir, A.R1CS_CONSTRAINTS_FILE), num_public_inputs)
        m = inst.num_constraints
        buf = np.zeros((inst.n_wires + 5 * m, 4), dtype=np.uint64)
        check(lib.dvp_setup_cache_dir_ex(ptr(t), ptr(d), ptr(e), os.fsencode(cache_dir), num_public_inputs, int(write_precomputes),
                                         ptr(buf), buf.shape[0], C.byref(nw), C.byref(lg)), "dvp_setup_cache_dir")
        assert nw.value == inst.n_wires and (1 << lg.value) == m
        o = inst.n_wires
        scalars = (buf[:o], buf[o:o + m], [buf[o + m:o + 2 * m], buf[o + 2 * m:o + 3 * m], buf[o + 3 * m:]])
    else:
        check(lib.dvp_setup_cache_dir(ptr(t), ptr(d), ptr(e), os.fsencode(cache_dir), num_public_inputs, int(write_precomputes)),
              "dvp_setup_cache_dir")
        inst = R1CSInstance.from_dump_file(os.path.join(cache_dir, A.R1CS_CONSTRAINTS_FILE), num_public_inputs)
    pv = Prover(inst)
    for which, name in enumerate(A.SRS_FILES):
        pv.set_srs_encoded(which, io_utils.read_point_vec_payload(os.path.join(cache_dir, name)))
    if return_scalars:
        return inst, pv, scalars
    return inst, pv


# dvp_srs_check_cache_dir (include/dvpari.h: DVP_SRS_VEC_*)
SRS_VEC_MISSING, SRS_VEC_LENGTH, SRS_VEC_DECODE, SRS_VEC_BAD_POINT, SRS_VEC_WRONG = 1, 2, 3, 4, 5
SRS_VECTORS = ("g_m", "g_q", "g_k_0", "g_k_1", "g_k_2")


@dataclass
class SrsVectorCheck:
    """one vector of an SrsCheckReport: status 0 or SRS_VEC_*, path curve.DLOG_PATH_* (0: never reached the check), first_bad the index
    of its first offending entry or None, count the entries expected"""
    name: str
    status: int
    path: int
    first_bad: int
    count: int

    @property
    def ok(self) -> bool:
        return self.status == 0


@dataclass
class SrsCheckReport:
    """verdict 0 = the directory holds the SRS of the trapdoor; bad_vectors: bit v = vector v failed; vectors: the five
    SrsVectorCheck in file order, also reachable by name (report["g_k_2"])"""
    verdict: int
    bad_vectors: int
    vectors: tuple

    @property
    def ok(self) -> bool:
        return self.verdict == 0

    def __getitem__(self, name):
        return self.vectors[SRS_VECTORS.index(name)]


def check_cache_dir(td: Trapdoor, cache_dir, num_public_inputs: int, seed=None, exact: bool = False) -> SrsCheckReport:
    """dvp_srs_check_cache_dir: are g_m, g_q, g_k_0..2 in cache_dir the SRS of `td` for cache_dir's R1CS dump and num_public_inputs?
    One combined MSM per vector (curve.check_dlogs on the scalars the setup would compute); every vector is checked and a wrong entry
    is named.  A missing, short or undecodable file is that vector's status; a zero trapdoor element raises DvpError(DVP_EINVAL)."""
    import ctypes as C

    from ._native import lib, check, ptr, SrsCheckReport as _Rep

    keep, (t, d, e) = _trapdoor_args(td)
    sd = curve._seed_arg(seed)
    rep = _Rep()
    check(lib.dvp_srs_check_cache_dir(t, d, e, os.fsencode(cache_dir), num_public_inputs, None if sd is None else ptr(sd),
                                      1 if exact else 0, C.byref(rep)), "dvp_srs_check_cache_dir")
    vecs = tuple(SrsVectorCheck(SRS_VECTORS[v], int(rep.status[v]), int(rep.path[v]), None if rep.first_bad[v] < 0 else int(rep.first_bad[v]),
                                int(rep.count[v])) for v in range(5))
    return SrsCheckReport(int(rep.verdict), int(rep.bad_vectors), vecs)


def _t(csr, n_wires):
    t = csr.transpose(n_wires)
    return t.row_ptr, t.wire, t.coeff


def verifier_runs_setup(prover, inst: R1CSInstance, td: Trapdoor) -> SRS:
    """SRS::verifier_runs_setup, src/srs.rs:177-361: the 6m fixed-base multiplications of
    compute_srs_matrices (:126-160) run as one batched GPU kernel per vector."""
    g_m, g_q, g_k = srs_scalars(prover, inst, td)
    mg = curve.point_scalar_mul_gen_batch
    return SRS(mg(g_m), mg(g_q), tuple(mg(v) for v in g_k))


def verify(td: Trapdoor, public_inputs, proof) -> bool:
    """SRS::verify, src/srs.rs:374-428."""
    from .proving import Proof, transcript_challenge

    pr = proof if isinstance(proof, Proof) else Proof.from_bytes(proof)
    try:
        pts, inf = curve.from_bytes(np.frombuffer(pr.commit_p + pr.kzg_k, dtype=np.uint8).reshape(2, 30))
    except Exception:
        return False
    a0, ok_a = pr.a0_fr()
    b0, ok_b = pr.b0_fr()
    if not (ok_a and ok_b):
        return False
    alpha = transcript_challenge(pr.commit_p, public_inputs, *get_verify_binding())  # the binding the GPU verifier follows too
    i0 = evaluate_monomial_basis_poly(public_inputs, alpha)
    r0 = (a0 * b0 - i0) % P
    delta2 = td.delta * td.delta % P
    u0 = (a0 + td.delta * b0 + delta2 * r0) % P * td.epsilon % P
    v0 = (td.tau - alpha) * td.epsilon % P
    gxy, ginf = curve.point_scalar_mul_gen_batch(fr.vec([1]))
    bases = np.stack([pts[1], gxy[0]])
    binf = np.array([inf[1], 0], dtype=np.uint8)
    lhs, lhs_inf = curve.multi_scalar_mul(fr.vec([v0, u0]), bases, binf)
    if lhs_inf or inf[0]:
        return bool(lhs_inf) and bool(inf[0])
    return bool((lhs == pts[0]).all())


# ---- the verifier on the GPU (csrc/verify.hip): SRS::verify for many proofs at once, one verdict per proof ------------------
VERIFY_BAD_COMMIT_P, VERIFY_BAD_KZG_K, VERIFY_BAD_A0, VERIFY_BAD_B0, VERIFY_BAD_PUBLIC, VERIFY_EQUATION = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
VERIFY_RLC_COMBINED, VERIFY_RLC_FALLBACK = 0x1, 0x2


def _raw_limbs(v) -> np.ndarray:
    """an int as 4 x u64 LE WITHOUT reduction (the C entries reject values >= p themselves)"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8").copy()


def _trapdoor_args(td: Trapdoor):
    from ._native import ptr

    arrs = [_raw_limbs(x) for x in (td.tau, td.delta, td.epsilon)]
    return arrs, [ptr(a) for a in arrs]


def _proofs_array(proofs) -> np.ndarray:
    from .proving import Proof

    if isinstance(proofs, np.ndarray):
        return np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 118)
    raw = b"".join(p.to_bytes() if isinstance(p, Proof) else bytes(p) for p in proofs)
    return np.frombuffer(raw, dtype=np.uint8).reshape(-1, 118).copy()


def _public_array(public_inputs, n: int) -> np.ndarray:
    """n rows of public inputs -> n x n_public x 4 u64 (values taken as given: the C entry checks them)"""
    if isinstance(public_inputs, np.ndarray) and public_inputs.dtype == np.uint64 and public_inputs.ndim == 3:
        return np.ascontiguousarray(public_inputs)
    rows = [list(r) for r in public_inputs]
    assert len(rows) == n, (len(rows), n)
    k = len(rows[0]) if rows else 0
    assert all(len(r) == k for r in rows), "every proof needs the same number of public inputs"
    out = np.zeros((n, k, 4), dtype=np.uint64)
    if n and k:
        buf = b"".join(int(v).to_bytes(32, "little") for r in rows for v in r)
        out[:] = np.frombuffer(buf, dtype="<u8").reshape(n, k, 4)
    return out


def set_verify_binding(srs_hash=None, circuit_hash=None):
    """dvp_verify_set_binding: the (srs_hash, circuit_hash) pair every verify entry of this process checks proofs against from now on;
    None = BLAKE3(""), (None, None) = the reference's unbound transcript.  A verifier that ran the setup from cache_dir gets the
    circuit half with proving.circuit_hash_cache_dir(cache_dir, num_public_inputs), which reads the R1CS dump alone"""
    from ._native import lib, check
    from .proving import _hash_arg

    ks, s = _hash_arg(srs_hash, "srs_hash")
    kc, c = _hash_arg(circuit_hash, "circuit_hash")
    check(lib.dvp_verify_set_binding(s, c), "dvp_verify_set_binding")


def get_verify_binding():
    """(srs_hash, circuit_hash) in force for the verify entries (BLAKE3("") where none is set)"""
    from ._native import lib, check, ptr

    s, c = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    check(lib.dvp_verify_get_binding(ptr(s), ptr(c)), "dvp_verify_get_binding")
    return s.tobytes(), c.tobytes()


def verify_batch(td: Trapdoor, public_inputs, proofs) -> np.ndarray:
    """SRS::verify (src/srs.rs:374-428) for n proofs against one trapdoor on the GPU (dvp_verify_batch): proofs = a list of
    Proof (or 118-byte strings) or an n x 118 uint8 array; public_inputs = one row per proof (list of lists, n x n_public ints
    or n x n_public x 4 uint64 limbs).  Returns n uint8 verdicts: 0 = accepted, else VERIFY_* bits."""
    from ._native import lib, check, ptr

    pa = _proofs_array(proofs)
    n = pa.shape[0]
    pub = _public_array(public_inputs, n)
    keep, (t, d, e) = _trapdoor_args(td)
    out = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return out
    pub_buf = pub if pub.size else np.zeros(4, dtype=np.uint64)
    check(lib.dvp_verify_batch(t, d, e, ptr(pub_buf), pub.shape[1], ptr(pa), n, ptr(out)), "dvp_verify_batch")
    return out


def verify_batch_rlc(td: Trapdoor, public_inputs, proofs, seed=None):
    """verify_batch by one random linear combination (dvp_verify_batch_rlc): the well-formed proofs are checked together by one
    MSM, and only when that check fails does the per-lane check run over the batch.  seed: 32 bytes, or None for the key derived
    from the trapdoor.  Returns (verdicts, report): verdicts as verify_batch's (equal to them except with probability <= 2^-127),
    report = VERIFY_RLC_COMBINED, VERIFY_RLC_FALLBACK, or 0 when no proof was well formed."""
    import ctypes as C

    from ._native import lib, check, ptr

    pa = _proofs_array(proofs)
    n = pa.shape[0]
    pub = _public_array(public_inputs, n)
    keep, (t, d, e) = _trapdoor_args(td)
    out = np.zeros(n, dtype=np.uint8)
    rep = C.c_uint32(0)
    if seed is not None:
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
    sd = None if seed is None else np.frombuffer(seed, dtype=np.uint8).copy()
    pub_buf = pub if pub.size else np.zeros(4, dtype=np.uint64)
    pa_buf = pa if n else np.zeros((1, 118), dtype=np.uint8)
    out_buf = out if n else np.zeros(1, dtype=np.uint8)
    check(lib.dvp_verify_batch_rlc(t, d, e, ptr(pub_buf), pub.shape[1], ptr(pa_buf), n, None if sd is None else ptr(sd), ptr(out_buf),
                                   C.byref(rep)), "dvp_verify_batch_rlc")
    return out, int(rep.value)


def verify_device(td: Trapdoor, public_inputs, proof) -> bool:
    """SRS::verify for one proof through dvp_verify (the same kernel as verify_batch)"""
    import ctypes as C

    from ._native import lib, check, ptr

    pa = _proofs_array([proof])
    pub = _public_array([list(public_inputs)], 1)
    pub_buf = pub if pub.size else np.zeros(4, dtype=np.uint64)
    keep, (t, d, e) = _trapdoor_args(td)
    acc, why = C.c_int(0), C.c_uint32(0)
    check(lib.dvp_verify(t, d, e, ptr(pub_buf), pub.shape[1], ptr(pa), C.byref(acc), C.byref(why)), "dvp_verify")
    return bool(acc.value)


# ---- verifier-side vectors (csrc/simulate.hip): accepted proofs from the trapdoor, and the verifier's stage values per proof ---------
SIM_GENERIC, SIM_T_HALF, SIM_P_ZERO, SIM_U0_ZERO, SIM_K_PLUS_G, SIM_K_MINUS_G, SIM_K_ZERO = range(7)
SIM_CASES = ("generic", "t_half", "p_zero", "u0_zero", "k_plus_g", "k_minus_g", "k_zero")  # SIM_CASES[SIM_T_HALF] == "t_half"
SIM_OK, SIM_V0_ZERO, SIM_BAD_PUBLIC, SIM_BAD_CASE, SIM_BAD_B0 = 0x00, 0x01, 0x02, 0x04, 0x08

_FR_FIELDS = ("alpha", "i0", "r0", "u0", "v0")
_POINT_FIELDS = ("p", "k", "vk", "ug", "sum")
VERIFY_TRACE_DTYPE = np.dtype([(f, "<u8", (4,)) for f in _FR_FIELDS] + [(f + "_xy", "<u8", (8,)) for f in _POINT_FIELDS]
                              + [(f + "_inf", "u1") for f in _POINT_FIELDS] + [("verdict", "u1"), ("pad", "u1", (2,))])
assert VERIFY_TRACE_DTYPE.itemsize == 488  # dvp_verify_trace, include/dvpari.h


def simulate_batch(td: Trapdoor, public_inputs, seed=None, index_base: int = 0, cases=None, b0=None, return_dlogs: bool = False):
    """dvp_simulate_batch: one accepted proof per row of public_inputs, made from the trapdoor alone (include/dvpari.h states the
    construction).  seed: 32 bytes, or None for the key derived from the trapdoor; cases: SIM_* per proof (None = all generic);
    b0: ints or n x 4 uint64 limbs (None = drawn).  Returns (proofs n x 118 uint8, status n uint8[, dlogs n x 2 x 4 uint64: p then k]);
    a proof with a nonzero status (SIM_V0_ZERO) is zero bytes."""
    from ._native import lib, check, ptr

    rows = public_inputs if isinstance(public_inputs, np.ndarray) else [list(r) for r in public_inputs]
    n = len(rows)
    pub = _public_array(rows, n)
    keep, (t, d, e) = _trapdoor_args(td)
    sd = curve._seed_arg(seed)
    cs = None if cases is None else np.ascontiguousarray(cases, dtype=np.uint8).reshape(n)
    if b0 is not None and not (isinstance(b0, np.ndarray) and b0.dtype == np.uint64):
        b0 = np.stack([_raw_limbs(v) for v in b0]) if n else np.zeros((0, 4), dtype=np.uint64)
    bb = None if b0 is None else np.ascontiguousarray(b0).reshape(n, 4)
    proofs = np.zeros((n, 118), dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    dlogs = np.zeros((n, 2, 4), dtype=np.uint64)
    pub_buf = pub if pub.size else np.zeros(4, dtype=np.uint64)
    opt = lambda a: None if a is None else ptr(a)  # noqa: E731
    check(lib.dvp_simulate_batch(t, d, e, ptr(pub_buf), pub.shape[1] if n else 0, n, opt(sd), index_base, opt(cs), opt(bb),
                                 ptr(proofs) if n else None, ptr(status) if n else None, ptr(dlogs) if (n and return_dlogs) else None),
          "dvp_simulate_batch")
    return (proofs, status, dlogs) if return_dlogs else (proofs, status)


def verify_trace(td: Trapdoor, public_inputs, proofs) -> np.ndarray:
    """dvp_verify_trace_batch: the arguments of verify_batch; one VERIFY_TRACE_DTYPE record per proof -- alpha, i0, r0, u0, v0 as limbs,
    the decoded points p (commit_p) and k (kzg_k), vk = v0 K, ug = u0 G and sum = vk + ug as *_xy / *_inf, and verdict, verify_batch's
    byte.  A record with a validity bit in its verdict is zero elsewhere."""
    from ._native import lib, check, ptr

    pa = _proofs_array(proofs)
    n = pa.shape[0]
    pub = _public_array(public_inputs, n)
    keep, (t, d, e) = _trapdoor_args(td)
    out = np.zeros(n, dtype=VERIFY_TRACE_DTYPE)
    if n == 0:
        return out
    pub_buf = pub if pub.size else np.zeros(4, dtype=np.uint64)
    check(lib.dvp_verify_trace_batch(t, d, e, ptr(pub_buf), pub.shape[1], ptr(pa), n, ptr(out)), "dvp_verify_trace_batch")
    return out


def format_verify_trace(rec) -> str:
    """one verify_trace record as text, one `name = hex` line per field (what examples/dvp_verify_cli --trace prints): scalars and
    coordinates as big-endian hex numbers, flags and the verdict as two hex digits"""
    lines = [f"{f} = {fr.to_int(rec[f]):064x}" for f in _FR_FIELDS]
    for f in _POINT_FIELDS:
        xy = np.asarray(rec[f + "_xy"])
        lines += [f"{f}_x = {fr.to_int(xy[:4]):064x}", f"{f}_y = {fr.to_int(xy[4:]):064x}"]
    lines += [f"{f}_inf = {int(rec[f + '_inf']):02x}" for f in _POINT_FIELDS]
    lines.append(f"verdict = {int(rec['verdict']):02x}")
    return "\n".join(lines)


def parse_verify_trace(text: str) -> np.ndarray:
    """format_verify_trace's (and the CLI's) lines back into one record; lines without ` = ` are skipped"""
    vals = dict(ln.split(" = ") for ln in text.splitlines() if " = " in ln)
    rec = np.zeros((), dtype=VERIFY_TRACE_DTYPE)
    for f in _FR_FIELDS:
        rec[f] = _raw_limbs(int(vals[f], 16))
    for f in _POINT_FIELDS:
        rec[f + "_xy"] = np.concatenate([_raw_limbs(int(vals[f + "_x"], 16)), _raw_limbs(int(vals[f + "_y"], 16))])
        rec[f + "_inf"] = int(vals[f + "_inf"], 16)
    rec["verdict"] = int(vals["verdict"], 16)
    return rec


def sp1_public_input(raw: int) -> int:
    """sp1_generate_scalar_from_raw_public_input, src/gnark_r1cs.rs:214-229 (dvp_sp1_public_input)"""
    from ._native import lib, check, ptr

    out = np.zeros(4, dtype=np.uint64)
    check(lib.dvp_sp1_public_input(int(raw), ptr(out)), "dvp_sp1_public_input")
    return fr.to_int(out)
