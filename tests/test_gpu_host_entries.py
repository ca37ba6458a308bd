"""GPU tests (-m gpu) of the host-pointer flavours of the C ABI as a family: what each of them stages around its _dev flavour.

Table-driven: every row is one entry at n in {0, 1, 65, 257} (one lane, across a 64-lane wave, across a 256-thread block), with the
infinity mask null and given (one flagged point), and its result must equal the _dev flavour of the same entry on the same data -- or
python integers, where the entry is field arithmetic.  The scalar rows hold the range check at p's limb boundaries: 0, 1, p - 1 and p
with limb k lowered (the limbs below all ones) pass; p, p + 1, 2^256 - 1 and p with limb k raised (the limbs below zero) are
DVP_EINVAL with dvp_last_error_index = their position, first and last.  The scalars of the _xsk233 entries sit at an odd address.

Asserted elsewhere and not repeated here: dvp_verify_batch_rlc against its _dev flavour, its argument order and *report = 0 for
n = 0 (test_gpu_verify_rlc: test_dev_flavour_on_a_stream_matches_host, test_argument_errors), dvp_verify_batch likewise
(test_gpu_verify), the fr vector entries on random data (test_gpu_fr_vec), dvp_points_check's classes against the case file
(test_gpu_points_check), dvp_ecfft_extend / enter / exit against the oracle (test_gpu_ecfft), the ark flavours (test_gpu_fr_ark)."""
import ctypes as C
import random

import numpy as np
import pytest

import point_cases as pc
import pyref as o
from util import from_limbs, pts_to_np, to_limbs

pytestmark = pytest.mark.gpu
P = o.P
M64 = (1 << 64) - 1
NONE64 = M64
OK, EINVAL, EDECODE, EPOINT = 0, -1, -2, -9
SIZES = [0, 1, 65, 257]
NMAX = 257


def boundary_scalars():
    """(accepted, rejected) around p, limb by limb"""
    limbs = [(P >> (64 * i)) & M64 for i in range(4)]
    join = lambda l: sum(v << (64 * i) for i, v in enumerate(l))
    acc, rej = [0, 1, P - 1], [P, P + 1, (1 << 256) - 1]
    for k in range(4):
        if limbs[k] < M64:
            rej.append(join([0] * k + [limbs[k] + 1] + limbs[k + 1:]))
        if limbs[k] > 0:
            acc.append(join([M64] * k + [limbs[k] - 1] + limbs[k + 1:]))
    assert all(v < P for v in acc) and all(P <= v < 1 << 256 for v in rej) and len(acc) == 6 and len(rej) == 7
    return acc, rej


ACCEPT, REJECT = boundary_scalars()


_ODD = []


def odd(a):
    """the same bytes at an odd address (the copy lives until the next few calls: callers pass it straight into vp())"""
    raw = np.zeros(a.nbytes + 1, dtype=np.uint8)
    v = raw[1:]
    v[:] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    assert not a.nbytes or v.ctypes.data & 1
    _ODD.append(v)
    del _ODD[:-4]
    return v


def hold(a):
    """keeps a temporary alive across the call it is passed to"""
    _ODD.append(a)
    del _ODD[:-4]
    return a


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def to_dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def dev_out(nbytes, fill=0xA5):
    import torch

    return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device="cuda")


def back(t, dtype, shape):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return t.cpu().numpy()[:n].view(dtype).reshape(shape)


@pytest.fixture(scope="module")
def data(dvp):
    """257 seeded points of E[r] (dvp_mulgen_batch_affine), their encodings, scalars whose first rows are the accepted boundary
    values, and a point of E[r] + N for strict mode: made once, never changed"""
    rnd = random.Random(4242)
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(to_limbs([rnd.randrange(1, P) for _ in range(NMAX)]))
    assert not inf.any()
    ks = to_limbs(ACCEPT + [rnd.randrange(P) for _ in range(NMAX - len(ACCEPT))])
    enc = dvp.curve.to_bytes(xy)
    rs = to_limbs([rnd.randrange(1, P) for _ in range(NMAX)])
    coset = next(q for q in pc.load() if q["cls"] == pc.COSET_N and not q["inf"] and q["x"])
    return dict(xy=xy, ks=ks, rs=rs, enc=enc, coset=pts_to_np([(coset["x"], coset["y"])])[0])


def flags(n, given):
    if not given or not n:
        return None
    f = np.zeros(n, dtype=np.uint8)
    f[n // 2] = 1
    return f


# ---- one wrapper per entry: host flavour and _dev flavour on the same arrays, both returning (status, outputs...) ----------------
def msm_host(dvp, s, xy, inf, n):
    out, fl = np.full(8, 0x5A, dtype=np.uint64), C.c_int(-7)
    rc = dvp.lib.dvp_msm_affine(vp(s), vp(xy), vp(inf), n, vp(out), C.byref(fl))
    return rc, out.tobytes(), fl.value


def msm_dev(dvp, s, xy, inf, n):
    import torch

    keep = [to_dev(s), to_dev(xy), to_dev(inf)]
    t_o, t_f = dev_out(64), dev_out(4)
    rc = dvp.lib.dvp_msm_affine_dev(dptr(keep[0]), dptr(keep[1]), dptr(keep[2]), n, dptr(t_o), dptr(t_f), None)
    torch.cuda.synchronize()
    return rc, back(t_o, np.uint64, (8,)).tobytes(), int(back(t_f, np.uint32, (1,))[0])


def pmul_host(dvp, s, ns, xy, inf, n):
    oxy, oinf = np.full((n, 8), 0x5A, dtype=np.uint64), np.full(n, 0xEE, dtype=np.uint8)
    rc = dvp.lib.dvp_points_mul(vp(s), ns, vp(xy), vp(inf), n, vp(oxy), vp(oinf))
    return rc, oxy.tobytes(), oinf.tobytes()


def pmul_dev(dvp, s, ns, xy, inf, n):
    import torch

    keep = [to_dev(s), to_dev(xy), to_dev(inf)]
    t_o, t_f, t_s = dev_out(64 * n), dev_out(n), dev_out(16)
    rc = dvp.lib.dvp_points_mul_dev(dptr(keep[0]), ns, dptr(keep[1]), dptr(keep[2]), n, dptr(t_o), dptr(t_f), dptr(t_s), None)
    torch.cuda.synchronize()
    return rc, back(t_o, np.uint64, (n, 8)).tobytes(), back(t_f, np.uint8, (n,)).tobytes(), tuple(int(v) for v in back(t_s, np.uint64, (2,)))


def seg_host(dvp, s, xy, inf, n, sp):
    ns = len(sp) - 1
    oxy, oinf = np.full((ns, 8), 0x5A, dtype=np.uint64), np.full(ns, 0xEE, dtype=np.uint8)
    rc = dvp.lib.dvp_msm_segments(vp(s), vp(xy), vp(inf), n, vp(sp), ns, vp(oxy), vp(oinf))
    return rc, oxy.tobytes(), oinf.tobytes()


def seg_dev(dvp, s, xy, inf, n, sp):
    import torch

    ns = len(sp) - 1
    wb = dvp.curve.segments_work_bytes(n, ns)
    keep = [to_dev(s), to_dev(xy), to_dev(inf)]
    t_o, t_f, t_w, t_s = dev_out(64 * ns), dev_out(ns), dev_out(wb), dev_out(16)
    rc = dvp.lib.dvp_msm_segments_dev(dptr(keep[0]) if n else None, dptr(keep[1]) if n else None, dptr(keep[2]), n, vp(sp), ns, dptr(t_o),
                                      dptr(t_f), dptr(t_w), wb, dptr(t_s), None)
    torch.cuda.synchronize()
    return rc, back(t_o, np.uint64, (ns, 8)).tobytes(), back(t_f, np.uint8, (ns,)).tobytes()


def seg_ptrs(n):
    """one segment; three with the middle one empty"""
    return [np.array([0, n], dtype=np.uint64), np.array([0, n // 3, n // 3, n], dtype=np.uint64)]


# ---- host flavour == _dev flavour ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_msm_affine(dvp, data, n, given):
    s, xy, inf = data["ks"][:n].copy(), data["xy"][:n].copy(), flags(n, given)
    h = msm_host(dvp, s, xy, inf, n)
    assert h[0] == OK and h == msm_dev(dvp, s, xy, inf, n)
    if n == 0:
        assert h[2] == 1  # the empty sum
    # the wire-format flavour is the encoding of the same sum; its scalars at an odd address
    enc, out = data["enc"][:n].copy(), np.zeros(30, dtype=np.uint8)
    if inf is not None:
        enc[n // 2] = 0
    assert dvp.lib.dvp_msm_xsk233(vp(odd(s)), vp(enc), n, vp(out)) == OK
    want = dvp.curve.to_bytes(np.frombuffer(h[1], dtype=np.uint64).reshape(1, 8), np.array([h[2]], dtype=np.uint8))
    assert out.tobytes() == want.tobytes()


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_msm_ctx_run(dvp, data, n, given):
    if n == 0:
        h = C.c_void_p()
        assert dvp.lib.dvp_msm_ctx_create(vp(data["xy"]), None, 0, 0, C.byref(h)) == EINVAL
        return
    s, xy, inf = data["ks"][:n].copy(), data["xy"][:n].copy(), flags(n, given)
    ctx = dvp.curve.FixedBaseMsm(xy, inf)
    try:
        for lo, hi in {(0, n), (n // 2, n)}:
            got = ctx.run(s[lo:hi], lo, hi)
            sub = None if inf is None else inf[lo:hi].copy()
            rc, want_xy, want_inf = msm_host(dvp, s[lo:hi].copy(), xy[lo:hi].copy(), sub, hi - lo)
            assert rc == OK and (got[0].tobytes(), int(got[1])) == (want_xy, want_inf), (lo, hi)
            assert ctx.run_ark(dvp.fr.to_ark(s[lo:hi]), lo, hi)[0].tobytes() == want_xy
    finally:
        ctx.close()


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_points_mul(dvp, data, n, given):
    xy, inf = data["xy"][:n].copy(), flags(n, given)
    for ns in sorted({1, n} - {0}):
        s = data["ks"][5:6].copy() if ns == 1 and n != 1 else data["ks"][:ns].copy()
        h = pmul_host(dvp, s, ns, xy, inf, n)
        if n == 0:  # DVP_OK, nothing touched
            assert h == (OK, b"", b"")
            continue
        d = pmul_dev(dvp, s, ns, xy, inf, n)
        assert h[0] == OK and d[0] == OK and h[1:] == d[1:3] and d[3] == (NONE64, 0), (n, ns)
        if inf is not None:
            assert h[2][n // 2] == 1
        enc = data["enc"][:n].copy()
        if inf is not None:
            enc[n // 2] = 0
        out = np.zeros((n, 30), dtype=np.uint8)
        assert dvp.lib.dvp_points_mul_xsk233(vp(odd(s)), ns, vp(enc), n, vp(out)) == OK
        oxy = np.frombuffer(h[1], dtype=np.uint64).reshape(n, 8)
        assert out.tobytes() == dvp.curve.to_bytes(oxy, np.frombuffer(h[2], dtype=np.uint8)).tobytes()


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_msm_segments(dvp, data, n, given):
    s, xy, inf = data["ks"][:n].copy(), data["xy"][:n].copy(), flags(n, given)
    for sp in seg_ptrs(n):
        ns = len(sp) - 1
        h = seg_host(dvp, s, xy, inf, n, sp)
        assert h[0] == OK and h == seg_dev(dvp, s, xy, inf, n, sp), (n, ns)
        oinf = np.frombuffer(h[2], dtype=np.uint8)
        if ns == 3:
            assert oinf[1] == 1  # the empty segment
        for j in range(ns):  # each segment is the MSM of its slice
            a, b = int(sp[j]), int(sp[j + 1])
            sub = None if inf is None else inf[a:b].copy()
            rc, mxy, minf = msm_host(dvp, s[a:b].copy(), xy[a:b].copy(), sub, b - a)
            assert rc == OK and minf == oinf[j] and (minf or h[1][64 * j:64 * j + 64] == mxy), (n, ns, j)
        enc = data["enc"][:n].copy()
        if inf is not None:
            enc[n // 2] = 0
        out = np.zeros((ns, 30), dtype=np.uint8)
        assert dvp.lib.dvp_msm_segments_xsk233(vp(odd(s)), vp(enc), n, vp(sp), ns, vp(out)) == OK
        assert out.tobytes() == dvp.curve.to_bytes(np.frombuffer(h[1], dtype=np.uint64).reshape(ns, 8), oinf).tobytes()


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_points_check_encode_decode_add(dvp, data, n, given):
    import torch

    xy, inf = data["xy"][:n].copy(), flags(n, given)
    if n > 2:
        xy[n - 1] = data["coset"]  # one bad point, last
    classes, nbad = np.full(n, 0xEE, dtype=np.uint8), C.c_size_t(77)
    rc = dvp.lib.dvp_points_check(vp(xy), vp(inf), n, vp(classes), C.byref(nbad))
    if n == 0:
        assert rc == OK and nbad.value == 77
        assert dvp.lib.dvp_points_encode(vp(xy), None, 0, None) == OK and dvp.lib.dvp_points_decode(None, 0, None, None) == OK
        return
    keep = [to_dev(xy), to_dev(inf)]
    t_c, t_s = dev_out(n), dev_out(16)
    assert dvp.lib.dvp_points_check_dev(dptr(keep[0]), dptr(keep[1]), n, dptr(t_c), dptr(t_s), None) == OK
    torch.cuda.synchronize()
    first, cnt = (int(v) for v in back(t_s, np.uint64, (2,)))
    assert classes.tobytes() == back(t_c, np.uint8, (n,)).tobytes() and nbad.value == cnt  # the classes come back with DVP_EPOINT too
    if n > 2:
        assert rc == EPOINT and dvp.lib.dvp_last_error_index() == first == n - 1 and cnt == 1 and classes[n - 1] == pc.COSET_N
        xy[n - 1] = data["xy"][n - 1]
    else:
        assert rc == OK and first == NONE64 and cnt == 0
    # encode = the encodings made once with a null mask, 30 zero bytes under a flag; decode gives the points back
    enc = dvp.curve.to_bytes(xy, inf)
    want = data["enc"][:n].copy()
    if inf is not None:
        want[n // 2] = 0
    assert enc.tobytes() == want.tobytes()
    dxy, dinf = dvp.curve.from_bytes(enc)
    live = np.ones(n, dtype=bool) if inf is None else inf == 0
    assert dinf.tobytes() == (np.zeros(n, dtype=np.uint8) if inf is None else inf).tobytes() and dxy[live].tobytes() == xy[live].tobytes()
    # a failed decode still copies its outputs back: every other lane as before, the bad one flagged
    rnd = random.Random(n)
    while True:
        junk = rnd.getrandbits(233).to_bytes(30, "little")
        if not o.xsk233_decode(junk, 0)[1]:
            break
    bad = enc.copy()
    bad[n - 1] = np.frombuffer(junk, dtype=np.uint8)
    bxy, binf = np.full((n, 8), 0x5A, dtype=np.uint64), np.full(n, 0xEE, dtype=np.uint8)
    assert dvp.lib.dvp_points_decode(vp(bad), n, vp(bxy), vp(binf)) == EDECODE and dvp.lib.dvp_last_error_index() == n - 1
    assert binf[n - 1] == 1 and binf[:n - 1].tobytes() == dinf[:n - 1].tobytes() and bxy[:n - 1][live[:n - 1]].tobytes() == dxy[:n - 1][live[:n - 1]].tobytes()
    # P + P through dvp_points_add = 2 P through dvp_points_mul; a flag on one side leaves the other operand
    two = to_limbs([2])
    sxy, sinf = dvp.curve.add(xy, xy, inf, inf)
    h = pmul_host(dvp, two, 1, xy, inf, n)
    hxy = np.frombuffer(h[1], dtype=np.uint64).reshape(n, 8)
    assert sinf.tobytes() == h[2] and sxy[live].tobytes() == hxy[live].tobytes()
    axy, ainf = dvp.curve.add(xy, xy, inf, None)
    assert ainf.tobytes() == bytes(n) and axy[~live].tobytes() == xy[~live].tobytes() and axy[live].tobytes() == sxy[live].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_mulgen_and_fr_entries(dvp, data, n):
    import torch

    lib = dvp.lib
    s = data["ks"][:n].copy()
    xy, inf = np.full((n, 8), 0x5A, dtype=np.uint64), np.full(n, 0xEE, dtype=np.uint8)
    assert lib.dvp_mulgen_batch_affine(vp(s), n, vp(xy), vp(inf)) == OK
    enc = np.full((n, 30), 0x5A, dtype=np.uint8)
    assert lib.dvp_mulgen_batch(vp(s), n, vp(enc)) == OK
    if n == 0:
        return
    assert inf[0] == 1 and not inf[1:].any()  # ks[0] = 0
    assert n == 1 or xy[1].tobytes() == pts_to_np([o.G_STD])[0].tobytes()  # ks[1] = 1
    assert enc.tobytes() == dvp.curve.to_bytes(xy, inf).tobytes()
    # k G through the fixed-base tables = k x G through dvp_points_mul
    g = pts_to_np([o.G_STD] * n)
    assert pmul_host(dvp, s, n, g, None, n) == (OK, xy.tobytes(), inf.tobytes())
    # the fr vector entries against python integers; the broadcast scalar runs through the accepted boundary values
    bl = data["rs"][:n].copy()
    a, b = from_limbs(s), from_limbs(bl)
    out = np.zeros((n, 4), dtype=np.uint64)
    assert lib.dvp_fr_vec_mul(vp(s), vp(bl), n, vp(out)) == OK and from_limbs(out) == [x * y % P for x, y in zip(a, b)]
    one = np.zeros(4, dtype=np.uint64)
    assert lib.dvp_fr_vec_dot(vp(s), vp(bl), n, vp(one)) == OK and from_limbs(one.reshape(1, 4))[0] == sum(x * y for x, y in zip(a, b)) % P
    for c in ACCEPT:
        cl = to_limbs([c])
        assert lib.dvp_fr_vec_scale(vp(s), vp(cl), n, vp(out)) == OK and from_limbs(out) == [c * x % P for x in a]
        assert lib.dvp_fr_vec_axpy(vp(s), vp(cl), vp(bl), n, vp(out)) == OK and from_limbs(out) == [(x + c * y) % P for x, y in zip(a, b)]
        assert lib.dvp_fr_vec_scalar_sub(vp(cl), vp(s), n, vp(out)) == OK and from_limbs(out) == [(c - x) % P for x in a]
    for c in REJECT:
        cl = to_limbs([c])
        assert lib.dvp_fr_vec_scale(vp(s), vp(cl), n, vp(out)) == EINVAL
        assert lib.dvp_fr_vec_axpy(vp(s), vp(cl), vp(bl), n, vp(out)) == EINVAL
        assert lib.dvp_fr_vec_scalar_sub(vp(cl), vp(s), n, vp(out)) == EINVAL
    inv = bl.copy()  # (seeded random values: none is zero)
    t = to_dev(bl)
    assert lib.dvp_fr_batch_inverse(vp(inv), n) == OK and lib.dvp_fr_batch_inverse_dev(dptr(t), n, None) == OK
    torch.cuda.synchronize()
    assert inv.tobytes() == back(t, np.uint64, (n, 4)).tobytes()
    assert all(b) and from_limbs(inv) == [pow(x, -1, P) for x in b]


# ---- the range check at p's limb boundaries, first and last index ---------------------------------------------------------------
def scalar_entries(dvp, data, n):
    """name -> call(scalars [n, 4]) -> status, for every host entry that takes a vector of n scalars"""
    lib = dvp.lib
    xy, enc = data["xy"][:n].copy(), data["enc"][:n].copy()
    sp = np.array([0, n // 3, n // 3, n], dtype=np.uint64)
    rows = max(n, 3)  # the segment entries write three rows whatever n
    oxy, oinf, oenc = np.zeros((rows, 8), dtype=np.uint64), np.zeros(rows, dtype=np.uint8), np.zeros((rows, 30), dtype=np.uint8)
    fl = C.c_int(0)
    ctx = dvp.curve.FixedBaseMsm(xy)
    t = dvp.ec_fft.FFTree(2 * n) if n >= 2 and n & (n - 1) == 0 else None
    digits = np.zeros((n, 512), dtype=np.int8)
    e = {
        "dvp_points_mul": lambda s: lib.dvp_points_mul(vp(s), n, vp(xy), None, n, vp(oxy), vp(oinf)),
        "dvp_points_mul_xsk233": lambda s: lib.dvp_points_mul_xsk233(vp(odd(s)), n, vp(enc), n, vp(oenc)),
        "dvp_msm_segments": lambda s: lib.dvp_msm_segments(vp(s), vp(xy), None, n, vp(sp), 3, vp(oxy), vp(oinf)),
        "dvp_msm_segments_xsk233": lambda s: lib.dvp_msm_segments_xsk233(vp(odd(s)), vp(enc), n, vp(sp), 3, vp(oenc)),
        "dvp_msm_affine": lambda s: lib.dvp_msm_affine(vp(s), vp(xy), None, n, vp(oxy), C.byref(fl)),
        "dvp_msm_xsk233": lambda s: lib.dvp_msm_xsk233(vp(odd(s)), vp(enc), n, vp(oenc)),
        "dvp_msm_ctx_run": lambda s: lib.dvp_msm_ctx_run(ctx._h, vp(s), 0, n, vp(oxy), C.byref(fl)),
        "dvp_mulgen_batch_affine": lambda s: lib.dvp_mulgen_batch_affine(vp(s), n, vp(oxy), vp(oinf)),
        "dvp_mulgen_batch": lambda s: lib.dvp_mulgen_batch(vp(s), n, vp(oenc)),
        "dvp_debug_recode_tnaf": lambda s: lib.dvp_debug_recode_tnaf(vp(s), n, 4, vp(digits), C.byref(fl), None),
    }
    if t is not None:  # the ECFFT entries take a power of two
        big = np.zeros((2 * n, 4), dtype=np.uint64)
        e["dvp_ecfft_extend"] = lambda s: lib.dvp_ecfft_extend(t._h, vp(s), 1, vp(big))
        e["dvp_ecfft_enter"] = lambda s: lib.dvp_ecfft_enter(t._h, vp(hold(np.concatenate([s, s]))), vp(big))
        e["dvp_ecfft_exit"] = lambda s: lib.dvp_ecfft_exit(t._h, vp(hold(np.concatenate([s, s]))), vp(big))
    return e, (ctx, t)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_scalar_range_at_first_and_last_index(dvp, data, n):
    entries, keep = scalar_entries(dvp, data, n)
    good = to_limbs((ACCEPT * (n // len(ACCEPT) + 1))[:n])
    for name, call in entries.items():
        assert call(good.copy()) == OK, name  # every accepted boundary value, in every position class
        for j in sorted({0, n - 1}):
            for r in REJECT:
                s = good.copy()
                s[j] = to_limbs([r])[0]
                assert call(s) == EINVAL and dvp.lib.dvp_last_error_index() == j, (name, j, hex(r))
    one = to_limbs([P])  # the broadcast scalar: index 0 whatever n
    oxy, oinf = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    assert dvp.lib.dvp_points_mul(vp(one), 1, vp(data["xy"]), None, n, vp(oxy), vp(oinf)) == (EINVAL if n else OK)
    assert dvp.lib.dvp_last_error_index() == 0
    keep[0].close()


def test_public_inputs_of_verify_batch(dvp):
    """the host range check of dvp_verify_batch / _rlc: the flat index of the first bad public input, before any device call; the
    accepted boundary values reach the kernels (verdicts are what they are: the proofs were made for other inputs)"""
    import test_gpu_verify_rlc as vr

    S = dvp.srs
    n = 65
    rnd = random.Random(17)
    built = vr.bulk(dvp, [[rnd.randrange(P)] for _ in range(n)], [None] * n, seed=18)
    proofs, pubs = vr.rows_of(built)
    v, rep = S.verify_batch_rlc(S.Trapdoor(*vr.TD), pubs, proofs)
    assert not v.any() and rep == S.VERIFY_RLC_COMBINED and not S.verify_batch(S.Trapdoor(*vr.TD), pubs, proofs).any()
    q = [[ACCEPT[i % len(ACCEPT)]] for i in range(n)]
    assert S.verify_batch(S.Trapdoor(*vr.TD), q, proofs).shape == (n,) and S.verify_batch_rlc(S.Trapdoor(*vr.TD), q, proofs)[0].shape == (n,)
    for j in (0, n - 1):
        for r in REJECT:
            q = [list(p) for p in pubs]
            q[j][0] = r
            for f in (S.verify_batch, S.verify_batch_rlc):
                with pytest.raises(dvp.DvpError) as ex:
                    f(S.Trapdoor(*vr.TD), q, proofs)
                assert ex.value.status == EINVAL and ex.value.index == j, (j, hex(r))


def test_trapdoor_arguments_of_setup_and_verify(dvp):
    """tau, delta and epsilon, one at a time: a null pointer and p are DVP_EINVAL for dvp_setup_scalars and for dvp_verify_batch
    (n = 0: the trapdoor is judged before anything else).  Zero is where the two DIFFER, on purpose: the setup refuses a zero
    trapdoor entry (src/srs.rs:199-201), the verifier takes it as it takes any scalar below p -- the shared loader must not unify that."""
    good = [to_limbs([v])[0] for v in (5, 6, 7)]
    rp = np.array([0, 0, 0], dtype=np.uint32)  # two empty rows per matrix, one wire, no coefficient
    mats = (C.c_void_p * 3)(*[rp.ctypes.data] * 3)
    none3 = (C.c_void_p * 3)(None, None, None)
    out = np.zeros((1 + 5 * 2, 4), dtype=np.uint64)

    def setup(td):
        return dvp.lib.dvp_setup_scalars(vp(td[0]), vp(td[1]), vp(td[2]), 1, 0, 2, 1, None, 0, mats, none3, none3, vp(out), out.shape[0])

    def verify(td):
        return dvp.lib.dvp_verify_batch(vp(td[0]), vp(td[1]), vp(td[2]), None, 0, None, 0, None)

    assert setup(good) == OK and verify(good) == OK
    for k in range(3):
        for bad, want_setup, want_verify in ((None, EINVAL, EINVAL), (to_limbs([P])[0], EINVAL, EINVAL), (to_limbs([0])[0], EINVAL, OK)):
            td = list(good)
            td[k] = bad
            assert (setup(td), verify(td)) == (want_setup, want_verify), (k, bad)


def test_strict_points_come_before_scalars(dvp, data):
    """strict mode: a bad point and a bad scalar (at a smaller index) together report the point"""
    n = 65
    xy = data["xy"][:n].copy()
    xy[41] = data["coset"]
    s = data["ks"][:n].copy()
    s[7] = to_limbs([P])[0]
    sp = np.array([0, 20, 20, n], dtype=np.uint64)
    prev = dvp.curve.strict_points()
    try:
        dvp.curve.set_strict_points(True)
        for ns in (n, 1):
            assert pmul_host(dvp, s[7:7 + ns].copy() if ns == 1 else s, ns, xy, None, n)[0] == EPOINT and dvp.lib.dvp_last_error_index() == 41
        assert seg_host(dvp, s, xy, None, n, sp)[0] == EPOINT and dvp.lib.dvp_last_error_index() == 41
        assert msm_host(dvp, s, xy, None, n)[0] == EPOINT and dvp.lib.dvp_last_error_index() == 41
        assert pmul_host(dvp, s, n, data["xy"][:n].copy(), None, n)[0] == EINVAL and dvp.lib.dvp_last_error_index() == 7
        out = np.zeros((n, 30), dtype=np.uint8)
        assert dvp.lib.dvp_points_encode(vp(xy), None, n, vp(out)) == EPOINT and dvp.lib.dvp_last_error_index() == 41
        a = data["xy"][:n].copy()
        a[50] = data["coset"]  # operand a first, whatever b holds earlier
        oxy, oinf = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        assert dvp.lib.dvp_points_add(vp(a), None, vp(xy), None, n, vp(oxy), vp(oinf)) == EPOINT and dvp.lib.dvp_last_error_index() == 50
    finally:
        dvp.curve.set_strict_points(prev)
