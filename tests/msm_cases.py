"""Inputs the MSM tests share, and the read-outs of the launch census (csrc/common.h: every kernel launch is counted per variant).
Nothing here touches a device until a function is called with the product package."""
import ctypes as C
import random

import numpy as np

import pyref as o
import c_oracle as co
from util import to_limbs, pts_to_np, rand_fr_np, np_dot_mod


def exceptional_pairs_input(n=4096):
    """bases drawn from eight points and their negatives, scalars from five values: (bases, scalars, the scalars and the bases'
    discrete logs as integers, the expected sum)"""
    rnd = random.Random(777)
    k8 = [rnd.randrange(1, o.P) for _ in range(8)]
    p8 = [co.k233_mulgen(x) for x in k8]
    vals = [rnd.randrange(o.P) for _ in range(4)] + [1]
    pts, ks, sv = [], [], []
    for i in range(n):
        j, neg = rnd.randrange(8), rnd.random() < 0.5
        pts.append(o.k233_neg(p8[j]) if neg else p8[j])
        ks.append(o.P - k8[j] if neg else k8[j])
        sv.append(rnd.choice(vals))
    return pts_to_np(pts), to_limbs(sv), sv, ks, co.k233_mulgen(sum(a * b for a, b in zip(sv, ks)) % o.P)


def random_input(dvp, n, seed):
    """n random scalars on n random bases k_i G: (bases, scalars, the oracle's point of the scalar-log dot product)"""
    k, s = rand_fr_np(n, seed), rand_fr_np(n, seed + 1)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    return bases, s, co.k233_mulgen(np_dot_mod(s, k))


def triples_input(dvp, n_groups=400, seed=9230):
    """n_groups x 3 bases, the three of a group under one common scalar: every bucket holds a multiple of three points"""
    k = rand_fr_np(3 * n_groups, seed)
    s = np.repeat(rand_fr_np(n_groups, seed + 1), 3, axis=0)
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    return bases, s, co.k233_mulgen(np_dot_mod(s, k))


def distinct_input(dvp, n=16):
    """n bases with the scalars 1 .. n: with signed binary windows wider than log2(n) + 1 (the fixed-base flavour) every bucket of the
    lowest window holds one point and all the others none; n = 1: one point, alone in its bucket of every window of any flavour"""
    k = rand_fr_np(n, 9401)
    s = to_limbs(range(1, n + 1))
    bases, inf = dvp.curve.point_scalar_mul_gen_batch(k)
    assert not inf.any()
    return bases, s, co.k233_mulgen(np_dot_mod(s, k))


# ---- the launch census --------------------------------------------------------------------------------------------------------

def launch_names(lib):
    """every "file:variant" the library can launch (dvp_debug_launch_names: no device is touched)"""
    need = lib.dvp_debug_launch_names(None, 0)
    buf = C.create_string_buffer(need)
    assert lib.dvp_debug_launch_names(buf, need) == need
    return [x for x in buf.value.decode().split("\n") if x]


def launches(dvp, name):
    """launches of one variant since the last dvp_profile_reset"""
    ms, n = C.c_double(-1), C.c_uint64(0)
    dvp.check(dvp.lib.dvp_profile_read(("launch:" + name).encode(), C.byref(ms), C.byref(n)), name)
    assert ms.value == 0
    return int(n.value)


def census(dvp, prefixes=("msm.hip:", "ecfft.hip:", "fr_ops.hip:")):
    """name -> launches since the last dvp_profile_reset, for every variant of the given files"""
    return {nm: launches(dvp, nm) for nm in launch_names(dvp.lib) if nm.startswith(tuple(prefixes))}


def rest_len(dvp):
    """entries the device put on the rest list during this thread's last MSM (dvp_debug_msm_rest_len)"""
    n = C.c_uint32(0)
    dvp.check(dvp.lib.dvp_debug_msm_rest_len(C.byref(n)))
    return int(n.value)


def assert_census(dvp, ran=(), idle=(), where=None):
    """every variant of `ran` was launched since the last reset, none of `idle` was; a name may end in '*' (all variants it prefixes:
    at least one of them ran / none of them ran)"""
    names = launch_names(dvp.lib)

    def expand(pat):
        got = [nm for nm in names if nm.startswith(pat[:-1])] if pat.endswith("*") else [nm for nm in names if nm == pat]
        assert got, f"no launch variant is called {pat}"
        return got

    for pat in ran:
        assert any(launches(dvp, nm) >= 1 for nm in expand(pat)), (pat, "did not run", where)
    for pat in idle:
        for nm in expand(pat):
            assert launches(dvp, nm) == 0, (nm, "ran", launches(dvp, nm), where)
