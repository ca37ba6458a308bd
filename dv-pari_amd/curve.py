"""Host mirror of src/curve.rs (multi_scalar_mul, point_scalar_mul_gen, to_bytes/from_bytes).

Points are numpy uint64 [n, 8] = x||y (4 limbs each) of the prime-order representative on
y^2+xy=x^3+1, plus an optional uint8 [n] infinity mask; scalars are uint64 [n, 4] canonical."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._native import lib, check, ptr, EPOINT, DlogReport as _DlogReport

FR_MODULUS = 3450873173395281893717377931138512760570940988862252126328087024741343


def multi_scalar_mul(scalars: np.ndarray, points_xy: np.ndarray, points_inf: np.ndarray = None):
    """multi_scalar_mul(&[Fr], &[CurvePoint]) -> CurvePoint, src/curve.rs:141-158.
    Returns (xy[8] uint64, is_infinity)."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    b = np.ascontiguousarray(points_xy, dtype=np.uint64)
    n = s.shape[0]
    assert s.shape == (n, 4) and b.shape == (n, 8), (s.shape, b.shape)
    inf_p = None
    if points_inf is not None:
        pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
        assert pi.shape == (n,)
        inf_p = ptr(pi)
    out = np.zeros(8, dtype=np.uint64)
    is_inf = C.c_int(0)
    check(lib.dvp_msm_affine(ptr(s), ptr(b), inf_p, n, ptr(out), C.byref(is_inf)), "dvp_msm_affine")
    return out, bool(is_inf.value)


def multi_scalar_mul_dev(d_scalars: int, d_bases: int, d_inf: int, n: int, d_out_xy: int, d_out_inf: int, stream: int = 0):
    check(lib.dvp_msm_affine_dev(d_scalars, d_bases, d_inf, n, d_out_xy, d_out_inf, stream), "dvp_msm_affine_dev")


def point_scalar_mul(scalars: np.ndarray, points_xy: np.ndarray, points_inf: np.ndarray = None):
    """point_scalar_mul over a vector, src/curve.rs:113-126: k_i P_i for n independent pairs in one launch.  scalars [n, 4], or
    [1, 4] / [4] = one scalar for every point.  Returns (xy [n,8], inf [n]); raises DvpError(DVP_EINVAL) with .index = the first
    non-canonical scalar, and in strict mode DvpError(DVP_EPOINT) for a bad point (points are checked before scalars)."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(points_xy, dtype=np.uint64).reshape(-1, 8)
    n = b.shape[0]
    inf_p = None
    if points_inf is not None:
        pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
        assert pi.shape == (n,)
        inf_p = ptr(pi)
    xy = np.zeros((n, 8), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    check(lib.dvp_points_mul(ptr(s), s.shape[0], ptr(b), inf_p, n, ptr(xy), ptr(inf)), "dvp_points_mul")
    return xy, inf


def point_scalar_mul_dev(d_scalars: int, n_scalars: int, d_xy: int, d_inf: int, n: int, d_out_xy: int, d_out_inf: int, d_summary: int,
                         stream: int = 0):
    """dvp_points_mul_dev: enqueue only; d_out_xy may be d_xy, d_inf may be 0; d_summary (16 bytes) = {u64 first non-canonical scalar
    or ~0, u64 how many}, reset by the call.  Such a lane gives O."""
    check(lib.dvp_points_mul_dev(d_scalars, n_scalars, d_xy, d_inf or None, n, d_out_xy, d_out_inf, d_summary, stream), "dvp_points_mul_dev")


def point_scalar_mul_bytes(scalars32: np.ndarray, enc30: np.ndarray) -> np.ndarray:
    """the same on the reference's wire formats: scalars [n, 32] (or one) little-endian bytes, points [n, 30] -> [n, 30]"""
    s = np.ascontiguousarray(scalars32, dtype=np.uint8).reshape(-1, 32)
    e = np.ascontiguousarray(enc30, dtype=np.uint8).reshape(-1, 30)
    out = np.zeros((e.shape[0], 30), dtype=np.uint8)
    check(lib.dvp_points_mul_xsk233(ptr(s), s.shape[0], ptr(e), e.shape[0], ptr(out)), "dvp_points_mul_xsk233")
    return out


def _seg_ptr(seg_ptr) -> np.ndarray:
    sp = np.ascontiguousarray(seg_ptr, dtype=np.uint64).reshape(-1)
    assert sp.shape[0] >= 1, "seg_ptr holds n_seg + 1 offsets"
    return sp


def multi_scalar_mul_segments(scalars: np.ndarray, points_xy: np.ndarray, seg_ptr, points_inf: np.ndarray = None):
    """n_seg independent multi_scalar_mul (src/curve.rs:141-158) over consecutive slices in one call: out[j] = sum of k_i P_i for
    seg_ptr[j] <= i < seg_ptr[j+1].  seg_ptr is CSR-style (n_seg + 1 offsets, 0 first, n last, non-decreasing); empty segments give
    O.  Returns (xy [n_seg, 8], inf [n_seg]); errors as point_scalar_mul, plus DvpError(DVP_EINVAL) with .index = the first offending
    segment for a bad seg_ptr."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(points_xy, dtype=np.uint64).reshape(-1, 8)
    sp = _seg_ptr(seg_ptr)
    n, n_seg = b.shape[0], sp.shape[0] - 1
    assert s.shape[0] == n, (s.shape, b.shape)
    inf_p = None
    if points_inf is not None:
        pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
        assert pi.shape == (n,)
        inf_p = ptr(pi)
    xy = np.zeros((n_seg, 8), dtype=np.uint64)
    inf = np.zeros(n_seg, dtype=np.uint8)
    check(lib.dvp_msm_segments(ptr(s), ptr(b), inf_p, n, ptr(sp), n_seg, ptr(xy), ptr(inf)), "dvp_msm_segments")
    return xy, inf


def segments_work_bytes(n: int, n_seg: int) -> int:
    """dvp_msm_segments_work_bytes: the d_work a multi_scalar_mul_segments_dev call of this shape needs (host arithmetic)"""
    return int(lib.dvp_msm_segments_work_bytes(n, n_seg))


def multi_scalar_mul_segments_dev(d_scalars: int, d_xy: int, d_inf: int, n: int, seg_ptr, d_out_xy: int, d_out_inf: int, d_work: int,
                                  work_bytes: int, d_summary: int, stream: int = 0):
    """dvp_msm_segments_dev: enqueue only.  seg_ptr is a HOST array, read during the call; d_inf may be 0; d_out_inf is n_seg bytes;
    d_work holds segments_work_bytes(n, n_seg) bytes; d_summary (16 bytes) as point_scalar_mul_dev.  Outputs must not overlap the
    inputs or d_work."""
    sp = _seg_ptr(seg_ptr)
    check(lib.dvp_msm_segments_dev(d_scalars or None, d_xy or None, d_inf or None, n, ptr(sp), sp.shape[0] - 1, d_out_xy, d_out_inf,
                                   d_work or None, work_bytes, d_summary, stream), "dvp_msm_segments_dev")


def multi_scalar_mul_segments_bytes(scalars32: np.ndarray, enc30: np.ndarray, seg_ptr) -> np.ndarray:
    """the same on the reference's wire formats: scalars [n, 32] little-endian bytes, points [n, 30] -> [n_seg, 30]"""
    s = np.ascontiguousarray(scalars32, dtype=np.uint8).reshape(-1, 32)
    e = np.ascontiguousarray(enc30, dtype=np.uint8).reshape(-1, 30)
    sp = _seg_ptr(seg_ptr)
    assert s.shape[0] == e.shape[0]
    out = np.zeros((sp.shape[0] - 1, 30), dtype=np.uint8)
    check(lib.dvp_msm_segments_xsk233(ptr(s), ptr(e), e.shape[0], ptr(sp), sp.shape[0] - 1, ptr(out)), "dvp_msm_segments_xsk233")
    return out


def point_scalar_mul_gen_batch(scalars: np.ndarray):
    """point_scalar_mul_gen over a vector (src/curve.rs:129-137, loops at src/srs.rs:130-160).
    Returns (xy [n,8], inf [n])."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = s.shape[0]
    xy = np.zeros((n, 8), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    check(lib.dvp_mulgen_batch_affine(ptr(s), n, ptr(xy), ptr(inf)), "dvp_mulgen_batch_affine")
    return xy, inf


def point_scalar_mul_gen_batch_bytes(scalars: np.ndarray) -> np.ndarray:
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = s.shape[0]
    out = np.zeros((n, 30), dtype=np.uint8)
    check(lib.dvp_mulgen_batch(ptr(s), n, ptr(out)), "dvp_mulgen_batch")
    return out


def to_bytes(points_xy: np.ndarray, points_inf: np.ndarray = None) -> np.ndarray:
    """CurvePoint::to_bytes over a vector, src/curve.rs:93-100."""
    b = np.ascontiguousarray(points_xy, dtype=np.uint64).reshape(-1, 8)
    n = b.shape[0]
    inf_p = None
    if points_inf is not None:
        pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
        inf_p = ptr(pi)
    out = np.zeros((n, 30), dtype=np.uint8)
    check(lib.dvp_points_encode(ptr(b), inf_p, n, ptr(out)), "dvp_points_encode")
    return out


def from_bytes(enc: np.ndarray):
    """CurvePoint::from_bytes over a vector, src/curve.rs:103-109; raises DvpError(DVP_EDECODE)
    on an invalid encoding (the reference asserts, src/io_utils.rs:223)."""
    e = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 30)
    n = e.shape[0]
    xy = np.zeros((n, 8), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    check(lib.dvp_points_decode(ptr(e), n, ptr(xy), ptr(inf)), "dvp_points_decode")
    return xy, inf


# classes of dvp_points_check (include/dvpari.h: DVP_POINT_*); 0 = a reduced point of E[r]
POINT_UNREDUCED, POINT_OFF_CURVE, POINT_ORDER4, POINT_COSET_N = 0x01, 0x02, 0x04, 0x08


def check_points(points_xy: np.ndarray, points_inf: np.ndarray = None):
    """dvp_points_check: (classes uint8 [n], index of the first bad point or None).  Does not raise for bad points: a point whose
    infinity flag is set is class 0 whatever its coordinates hold.  COSET_N is P + N with P in E[r], N = (0,1): the affine view
    xs233 itself holds of a group element; this library takes the E[r] representative P (or the 30-byte encoding)."""
    b = np.ascontiguousarray(points_xy, dtype=np.uint64).reshape(-1, 8)
    n = b.shape[0]
    inf_p = None
    if points_inf is not None:
        pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
        assert pi.shape == (n,)
        inf_p = ptr(pi)
    classes = np.zeros(n, dtype=np.uint8)
    n_bad = C.c_size_t(0)
    rc = lib.dvp_points_check(ptr(b), inf_p, n, ptr(classes), C.byref(n_bad))
    if rc == EPOINT:
        return classes, int(lib.dvp_last_error_index())
    check(rc, "dvp_points_check")
    return classes, None


def check_points_dev(d_xy: int, d_inf: int, n: int, d_classes: int, d_summary: int, stream: int = 0):
    """dvp_points_check_dev: enqueue only; d_summary (16 bytes) = {u64 first bad index or ~0, u64 bad points}, reset by the call"""
    check(lib.dvp_points_check_dev(d_xy, d_inf, n, d_classes, d_summary, stream), "dvp_points_check_dev")


# dvp_points_check_dlog (include/dvpari.h: DVP_DLOG_*)
DLOG_CHECK_EXACT = 0x1
DLOG_BAD_POINT, DLOG_WRONG = 0x1, 0x2
DLOG_PATH_COMBINED, DLOG_PATH_LOCATED, DLOG_PATH_EXACT = 1, 2, 3


@dataclass
class DlogReport:
    """verdict: 0 = every point is its scalar's multiple of G, else DLOG_BAD_POINT / DLOG_WRONG; path: DLOG_PATH_*; first_bad: index of
    the first wrong or ill-formed point, or None; point_class: its POINT_* class (0 for a well-formed wrong point)"""
    verdict: int
    path: int
    first_bad: int
    point_class: int

    @property
    def ok(self) -> bool:
        return self.verdict == 0


def _seed_arg(seed):
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    return np.frombuffer(seed, dtype=np.uint8).copy()


def _dlog_report(rep) -> DlogReport:
    return DlogReport(int(rep.verdict), int(rep.path), None if rep.first_bad < 0 else int(rep.first_bad), int(rep.point_class))


def check_dlogs(scalars: np.ndarray, points_xy: np.ndarray, points_inf: np.ndarray = None, seed=None, exact: bool = False) -> DlogReport:
    """dvp_points_check_dlog: is points[i] == scalars[i] * G for every i?  One combined MSM of n + 1 points under coefficients hashed
    from the points themselves (wrong vectors pass with probability <= 2^-127), then -- only when that fails, or alone with exact --
    the entry-for-entry comparison that names the first wrong index.  seed: 32 bytes or None.  A bad point (outside E[r], unreduced,
    off the curve) is the report's verdict; a non-canonical scalar raises DvpError(DVP_EINVAL) with .index."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(points_xy, dtype=np.uint64).reshape(-1, 8)
    n = b.shape[0]
    assert s.shape[0] == n, (s.shape, b.shape)
    pi = None
    if points_inf is not None:
        pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
        assert pi.shape == (n,)
    sd = _seed_arg(seed)
    rep = _DlogReport()
    check(lib.dvp_points_check_dlog(ptr(s) if n else None, ptr(b) if n else None, None if pi is None or not n else ptr(pi), n,
                                    None if sd is None else ptr(sd), DLOG_CHECK_EXACT if exact else 0, C.byref(rep)), "dvp_points_check_dlog")
    return _dlog_report(rep)


def check_dlogs_work_bytes(n: int) -> int:
    """dvp_points_check_dlog_work_bytes: the d_work a check_dlogs_dev call over n points needs (host arithmetic)"""
    return int(lib.dvp_points_check_dlog_work_bytes(n))


def check_dlogs_dev(d_scalars: int, d_xy: int, d_inf: int, n: int, d_work: int, work_bytes: int, seed=None, exact: bool = False,
                    stream: int = 0) -> DlogReport:
    """dvp_points_check_dlog_dev: the same on device buffers; d_inf may be 0; d_work: check_dlogs_work_bytes(n) bytes, 256-byte aligned.
    Waits for its verdict."""
    sd = _seed_arg(seed)
    rep = _DlogReport()
    check(lib.dvp_points_check_dlog_dev(d_scalars or None, d_xy or None, d_inf or None, n, None if sd is None else ptr(sd),
                                        DLOG_CHECK_EXACT if exact else 0, d_work or None, work_bytes, C.byref(rep), stream),
          "dvp_points_check_dlog_dev")
    return _dlog_report(rep)


def set_strict_points(on: bool):
    """dvp_points_set_strict: process-wide; when on, the entries that take affine points from the host (multi_scalar_mul,
    FixedBaseMsm, Prover.set_srs, add, to_bytes) check them first and raise DvpError(DVP_EPOINT) with .index = the first bad point"""
    check(lib.dvp_points_set_strict(int(bool(on))), "dvp_points_set_strict")


def strict_points() -> bool:
    return bool(lib.dvp_points_get_strict())


def add(a_xy, b_xy, a_inf=None, b_inf=None):
    """CurvePoint::add over two vectors, src/curve.rs:84-90.  Returns (xy [n,8], inf [n]).  In strict mode operand a is checked
    first, then b: DvpError.index is the first bad point of a, and of b only when a is clean."""
    a = np.ascontiguousarray(a_xy, dtype=np.uint64).reshape(-1, 8)
    b = np.ascontiguousarray(b_xy, dtype=np.uint64).reshape(-1, 8)
    n = a.shape[0]
    assert b.shape[0] == n
    ai = None if a_inf is None else np.ascontiguousarray(a_inf, dtype=np.uint8)
    bi = None if b_inf is None else np.ascontiguousarray(b_inf, dtype=np.uint8)
    xy = np.zeros((n, 8), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    check(lib.dvp_points_add(ptr(a), None if ai is None else ptr(ai), ptr(b), None if bi is None else ptr(bi), n, ptr(xy), ptr(inf)),
          "dvp_points_add")
    return xy, inf


def multi_scalar_mul_bytes(scalars32: np.ndarray, bases30: np.ndarray) -> bytes:
    s = np.ascontiguousarray(scalars32, dtype=np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(bases30, dtype=np.uint8).reshape(-1, 30)
    assert s.shape[0] == b.shape[0]
    out = np.zeros(30, dtype=np.uint8)
    check(lib.dvp_msm_xsk233(ptr(s), ptr(b), s.shape[0], ptr(out)), "dvp_msm_xsk233")
    return out.tobytes()


def multi_scalar_mul_bytes_ark(scalars_ark: np.ndarray, bases30: np.ndarray) -> bytes:
    """multi_scalar_mul_bytes with the scalars as arkworks holds them in memory (uint64 [n, 4] of a * 2^256 mod p, fr.to_ark),
    converted on the GPU (dvp_msm_xsk233_ark)"""
    from . import fr

    s = fr._ark_arg(scalars_ark, "multi_scalar_mul_bytes_ark")
    b = np.ascontiguousarray(bases30, dtype=np.uint8).reshape(-1, 30)
    if s.shape[0] != b.shape[0]:
        raise ValueError(f"multi_scalar_mul_bytes_ark: {s.shape[0]} scalars for {b.shape[0]} bases")
    out = np.zeros(30, dtype=np.uint8)
    check(lib.dvp_msm_xsk233_ark(ptr(s), ptr(b), s.shape[0], ptr(out)), "dvp_msm_xsk233_ark")
    return out.tobytes()


class FixedBaseMsm:
    """multi_scalar_mul against a fixed base vector (an SRS vector): dvp_msm_ctx_* in include/dvpari.h."""

    def __init__(self, points_xy: np.ndarray, points_inf: np.ndarray = None, range_hint: int = 0):
        b = np.ascontiguousarray(points_xy, dtype=np.uint64).reshape(-1, 8)
        self.n = b.shape[0]
        inf_p = None
        if points_inf is not None:
            pi = np.ascontiguousarray(points_inf, dtype=np.uint8)
            inf_p = ptr(pi)
        h = C.c_void_p()
        check(lib.dvp_msm_ctx_create(ptr(b), inf_p, self.n, range_hint, C.byref(h)), "dvp_msm_ctx_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and lib is not None:  # lib is None while the interpreter shuts down
            lib.dvp_msm_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def plan(self):
        """(window bits, windows) the context settled on"""
        c, w = C.c_int(0), C.c_int(0)
        check(lib.dvp_msm_ctx_plan(self._h, C.byref(c), C.byref(w)), "dvp_msm_ctx_plan")
        return c.value, w.value

    def table(self):
        """(bytes of HBM, signed binary windows -- the default flavour -- ?) of the pre-rotated table"""
        s = C.c_int(0)
        b = int(lib.dvp_msm_ctx_table_bytes(self._h, C.byref(s)))
        return b, bool(s.value)

    def run(self, scalars: np.ndarray, lo: int = 0, hi: int = None):
        hi = self.n if hi is None else hi
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        assert s.shape[0] == hi - lo
        out = np.zeros(8, dtype=np.uint64)
        is_inf = C.c_int(0)
        check(lib.dvp_msm_ctx_run(self._h, ptr(s), lo, hi, ptr(out), C.byref(is_inf)), "dvp_msm_ctx_run")
        return out, bool(is_inf.value)

    def run_ark(self, scalars_ark: np.ndarray, lo: int = 0, hi: int = None):
        """run with the scalars as arkworks holds them in memory (fr.to_ark), converted on the GPU (dvp_msm_ctx_run_ark)"""
        from . import fr

        hi = self.n if hi is None else hi
        s = fr._ark_arg(scalars_ark, "run_ark")
        if s.shape[0] != hi - lo:
            raise ValueError(f"run_ark: {s.shape[0]} scalars for bases [{lo}, {hi})")
        out = np.zeros(8, dtype=np.uint64)
        is_inf = C.c_int(0)
        check(lib.dvp_msm_ctx_run_ark(self._h, ptr(s), lo, hi, ptr(out), C.byref(is_inf)), "dvp_msm_ctx_run_ark")
        return out, bool(is_inf.value)
