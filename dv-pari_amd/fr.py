"""Fr vectors as numpy uint64 [n,4] canonical limbs, with the GPU vector ops of the C ABI.
(src/curve.rs:16-22; the rayon pointwise maps of src/proving.rs:492-654.)"""
import numpy as np

from ._native import lib, check, ptr

P = 3450873173395281893717377931138512760570940988862252126328087024741343
MASK64 = (1 << 64) - 1


def limbs(v) -> np.ndarray:
    """python int -> [4] uint64"""
    v = int(v) % P
    return np.array([(v >> (64 * i)) & MASK64 for i in range(4)], dtype=np.uint64)


def vec(vals) -> np.ndarray:
    vals = [int(v) % P for v in vals]
    buf = b"".join(v.to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), 4).copy()


def to_int(a) -> int:
    return int.from_bytes(np.ascontiguousarray(a, dtype="<u8").tobytes(), "little")


def to_ints(arr) -> list:
    raw = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _c(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def mul(a, b):
    a, b = _c(a), _c(b)
    out = np.empty_like(a)
    check(lib.dvp_fr_vec_mul(ptr(a), ptr(b), a.shape[0], ptr(out)), "dvp_fr_vec_mul")
    return out


def scale(a, s: int):
    a = _c(a)
    out = np.empty_like(a)
    check(lib.dvp_fr_vec_scale(ptr(a), ptr(limbs(s)), a.shape[0], ptr(out)), "dvp_fr_vec_scale")
    return out


def axpy(a, s: int, b):
    """a + s * b"""
    a, b = _c(a), _c(b)
    out = np.empty_like(a)
    check(lib.dvp_fr_vec_axpy(ptr(a), ptr(limbs(s)), ptr(b), a.shape[0], ptr(out)), "dvp_fr_vec_axpy")
    return out


def scalar_sub(s: int, a):
    a = _c(a)
    out = np.empty_like(a)
    check(lib.dvp_fr_vec_scalar_sub(ptr(limbs(s)), ptr(a), a.shape[0], ptr(out)), "dvp_fr_vec_scalar_sub")
    return out


def dot(a, b) -> int:
    a, b = _c(a), _c(b)
    out = np.zeros(4, dtype=np.uint64)
    check(lib.dvp_fr_vec_dot(ptr(a), ptr(b), a.shape[0], ptr(out)), "dvp_fr_vec_dot")
    return to_int(out)


def batch_inverse(a):
    """ark_ff::batch_inversion (zeros stay zero)."""
    a = _c(a).copy()
    check(lib.dvp_fr_batch_inverse(ptr(a), a.shape[0]), "dvp_fr_batch_inverse")
    return a


def vec_digest(v) -> bytes:
    """BLAKE3 of Vec<Fr>::serialize_uncompressed of v (uint64 [n, 4] canonical, or ints): the u64 count, then 29 bytes little-endian
    per entry -- the bytes io_utils.write_fr_vec_to_file writes; packed and hashed on the GPU (dvp_fr_vec_digest).  An entry >= p
    raises DvpError (DVP_EINVAL) with its index."""
    a = _c(v) if isinstance(v, np.ndarray) else (vec(v) if len(v) else np.zeros((0, 4), dtype=np.uint64))
    out = np.zeros(32, dtype=np.uint8)
    check(lib.dvp_fr_vec_digest(ptr(a) if a.shape[0] else None, a.shape[0], ptr(out)), "dvp_fr_vec_digest")
    return out.tobytes()


def vec_digest_dev(d_fr: int, n: int, montgomery: bool = False, stream: int = 0) -> bytes:
    """the same over n x 32 bytes at the device address d_fr (dvp_fr_vec_digest_dev; montgomery: the entries are a R mod p and are
    converted first).  The low 29 bytes of every entry are hashed unchecked.  The call only enqueues on `stream`; this wrapper then
    waits for the 32 bytes."""
    import torch

    out = torch.empty(32, dtype=torch.uint8, device="cuda")
    check(lib.dvp_fr_vec_digest_dev(d_fr or None, n, int(bool(montgomery)), out.data_ptr(), stream or None), "dvp_fr_vec_digest_dev")
    if stream:
        torch.cuda.ExternalStream(stream).synchronize()
    else:
        torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


def _be32_arg(raw) -> np.ndarray:
    """n x 32 big-endian bytes (bytes-like, or a uint8 array of shape [n, 32] / [32 n]) as a contiguous uint8 [n, 32]"""
    a = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.asarray(raw)
    if a.dtype != np.uint8:
        raise ValueError(f"from_be32: expected bytes or a uint8 array, got {a.dtype}")
    if a.ndim == 2 and a.shape[1] != 32 or a.ndim > 2 or a.size % 32:
        raise ValueError(f"from_be32: expected n x 32 bytes, got shape {a.shape}")
    return np.ascontiguousarray(a).reshape(-1, 32)


def from_be32(raw) -> np.ndarray:
    """gnark_element_to_fr over a vector (src/gnark_r1cs.rs:58-77): n x 32 big-endian bytes, any value below 2^256, -> uint64 [n, 4]
    canonical, reduced mod p on the GPU (dvp_fr_from_be32)"""
    a = _be32_arg(raw)
    out = np.zeros((a.shape[0], 4), dtype=np.uint64)
    if a.shape[0]:
        check(lib.dvp_fr_from_be32(ptr(a), a.shape[0], ptr(out)), "dvp_fr_from_be32")
    return out


def from_be32_host(raw) -> np.ndarray:
    """the host build of the same function (dvp_debug_fr_from_be32_host): no GPU needed; for tests"""
    a = _be32_arg(raw)
    out = np.zeros((a.shape[0], 4), dtype=np.uint64)
    if a.shape[0]:
        check(lib.dvp_debug_fr_from_be32_host(ptr(a), a.shape[0], ptr(out)), "dvp_debug_fr_from_be32_host")
    return out


def from_be32_dev(d_be32: int, n: int, d_out: int = None, stream: int = 0):
    """dvp_fr_from_be32_dev: n elements at the device address d_be32 -> d_out (None = in place), both 16-byte aligned; only enqueues
    on `stream`"""
    check(lib.dvp_fr_from_be32_dev(d_be32 or None, n, (d_be32 if d_out is None else d_out) or None, stream or None), "dvp_fr_from_be32_dev")


def _ark_arg(v, who: str) -> np.ndarray:
    """n elements of four u64 each (a uint64 array of shape [n, 4] / [4 n], or bytes of 32 n) as a uint64 [n, 4] view; the memory may
    start at any address (a byte-offset view is passed on as it is)"""
    if isinstance(v, (bytes, bytearray, memoryview)):
        if len(v) % 32:
            raise ValueError(f"{who}: expected n x 32 bytes, got {len(v)}")
        return np.frombuffer(v, dtype=np.uint64).reshape(-1, 4)
    a = np.asarray(v)
    if a.dtype != np.uint64:
        raise ValueError(f"{who}: expected a uint64 array, got {a.dtype}")
    if a.ndim == 2 and a.shape[1] != 4 or a.ndim > 2 or a.size % 4:
        raise ValueError(f"{who}: expected n x 4 limbs, got shape {a.shape}")
    return np.ascontiguousarray(a).reshape(-1, 4)


def _ark_call(fn, name, v, *lead):
    a = _ark_arg(v, name)
    out = np.zeros((a.shape[0], 4), dtype=np.uint64)
    if a.shape[0]:
        check(fn(*lead, ptr(a), a.shape[0], ptr(out)), name)
    return out


def from_ark(ark) -> np.ndarray:
    """Fr as arkworks holds it in memory (four LE u64 of a * 2^256 mod p, src/curve.rs:16-22) -> uint64 [n, 4] canonical, on the GPU
    (dvp_fr_from_ark): into_bigint() over a vector.  Total: any value below 2^256 is reduced first."""
    return _ark_call(lib.dvp_fr_from_ark, "dvp_fr_from_ark", ark)


def to_ark(limbs_) -> np.ndarray:
    """canonical limbs (any value below 2^256, reduced first) -> the arkworks in-memory form, on the GPU (dvp_fr_to_ark)"""
    return _ark_call(lib.dvp_fr_to_ark, "dvp_fr_to_ark", limbs_)


def from_ark_host(ark) -> np.ndarray:
    """the host build of from_ark's per-element function (dvp_debug_fr_ark_host): no GPU needed; for tests and baselines"""
    return _ark_call(lib.dvp_debug_fr_ark_host, "dvp_debug_fr_ark_host", ark, 0)


def to_ark_host(limbs_) -> np.ndarray:
    """the host build of to_ark's per-element function (dvp_debug_fr_ark_host): no GPU needed"""
    return _ark_call(lib.dvp_debug_fr_ark_host, "dvp_debug_fr_ark_host", limbs_, 1)


def from_ark_dev(d_in: int, n: int, d_out: int = None, stream: int = 0):
    """dvp_fr_from_ark_dev: n elements at the device address d_in -> d_out (None = in place), both 16-byte aligned; only enqueues on
    `stream`"""
    check(lib.dvp_fr_from_ark_dev(d_in or None, n, d_out or None, stream or None), "dvp_fr_from_ark_dev")


def to_ark_dev(d_in: int, n: int, d_out: int = None, stream: int = 0):
    """dvp_fr_to_ark_dev: the other direction, same rules"""
    check(lib.dvp_fr_to_ark_dev(d_in or None, n, d_out or None, stream or None), "dvp_fr_to_ark_dev")


def ark_is_one(ark32) -> bool:
    """fr_ark_is_one on 32 bytes: is this arkworks-form element the field's one (2^256 mod p, any representative below 2^256)?"""
    a = np.frombuffer(bytes(ark32), dtype=np.uint8)
    if a.size != 32:
        raise ValueError(f"ark_is_one: expected 32 bytes, got {a.size}")
    return bool(lib.dvp_debug_fr_ark_is_one(ptr(a)))


# enum dvp_fr_op (include/dvpari_internal.h): name -> (number, inputs, outputs)
DEBUG_OPS = {name: (k, n_in, n_out) for k, (name, n_in, n_out) in enumerate([
    ("add", 2, 1), ("sub", 2, 1), ("neg", 1, 1), ("dbl", 1, 1), ("cond_sub_p", 1, 1), ("is_canonical", 1, 1), ("mul", 2, 1),
    ("sqr", 1, 1), ("to_mont", 1, 1), ("from_mont", 1, 1), ("dot2", 4, 1), ("muladd29", 3, 1), ("mul29", 2, 1), ("roundtrip29", 1, 1),
    ("roundtrip30", 1, 1), ("const30", 1, 1), ("canon30", 1, 1), ("sub_lazy30", 2, 1), ("muladd30", 3, 1), ("muladd30_x2", 6, 2),
    ("inv", 1, 1), ("inv_gcd_raw", 1, 1), ("inv_fermat", 1, 1), ("pow_u64", 2, 1), ("limbs29", 1, 1), ("limbs30", 1, 1)])}


def debug_op(name: str, inputs, on_device: bool):
    """dvp_debug_fr_op: one function of csrc/fr.cuh per element.  inputs: one bytes object of n x 32 bytes (raw little-endian 256-bit
    values) per operand; returns the outputs the same way.  on_device=False runs the host build of the function, without a GPU."""
    import ctypes as C

    op, n_in, n_out = DEBUG_OPS[name]
    assert len(inputs) == n_in and len({len(b) for b in inputs}) == 1 and len(inputs[0]) % 32 == 0
    n = len(inputs[0]) // 32
    ins = [np.frombuffer(bytes(b), dtype="<u8") for b in inputs]
    outs = [np.zeros(4 * n, dtype=np.uint64) for _ in range(n_out)]
    pin = (C.c_void_p * 6)(*[a.ctypes.data for a in ins])
    pout = (C.c_void_p * 2)(*[a.ctypes.data for a in outs])
    check(lib.dvp_debug_fr_op(op, pin, n, 1 if on_device else 0, pout), f"dvp_debug_fr_op({name})")
    return [a.tobytes() for a in outs]


def spmv(row_ptr, col, coeff_ids, coeffs, x):
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    coeff_ids = np.ascontiguousarray(coeff_ids, dtype=np.uint32)
    coeffs, x = _c(coeffs), _c(x)
    n_rows = row_ptr.shape[0] - 1
    out = np.zeros((n_rows, 4), dtype=np.uint64)
    check(lib.dvp_fr_spmv(ptr(row_ptr), ptr(col), ptr(coeff_ids), n_rows, ptr(coeffs), coeffs.shape[0], ptr(x), x.shape[0], ptr(out)),
          "dvp_fr_spmv")
    return out
