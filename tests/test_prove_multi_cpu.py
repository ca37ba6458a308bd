"""CPU tests of the SRS slots and prove_multi: the new entries are declared, exported and bound with the header's arity, and the Python
wrappers handle their arguments as documented.  No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvp_prover_srs_slot_add", "dvp_prover_srs_slot_select", "dvp_prover_srs_slot_active", "dvp_prover_srs_slot_count",
       "dvp_prover_srs_slot_drop", "dvp_prover_srs_slot_bytes", "dvp_prove_multi_dev", "dvp_prove_multi", "dvp_prove_multi_be32",
       "dvp_prove_multi_ark", "dvp_cache_dir_add_srs_dir", "dvp_cache_dir_slot_set_binding", "dvp_prove_cache_dir_multi",
       "dvp_prove_cache_dir_multi_ark", "dvp_prove_cache_dir_multi_witness_file"]


def prototypes():
    """name -> number of parameters, for every prototype of include/dvpari.h"""
    txt = open(os.path.join(ROOT, "include", "dvpari.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(dvp_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", txt, flags=re.S):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_new_entries_declared_exported_and_bound(nat):
    protos = prototypes()
    lib = C.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(lib, name), name
        assert name in nat._SIGS and name in nat.EXPORTED, name
        assert len(nat._SIGS[name][1]) == protos[name], (name, len(nat._SIGS[name][1]), protos[name])
    # the arity check means something: it holds for entries that were there before
    for name in ("dvp_prove", "dvp_prove_dev", "dvp_prover_msm_coverage", "dvp_cache_dir_set_binding"):
        assert len(nat._SIGS[name][1]) == protos[name], name


def test_every_new_entry_cites_the_seam():
    """include/dvpari.h names the reference's seam (SRS per Trapdoor, src/srs.rs) in the comment that introduces each new entry"""
    txt = open(os.path.join(ROOT, "include", "dvpari.h")).read()
    blocks = [(m.end(), m.group(0)) for m in re.finditer(r"/\*.*?\*/", txt, flags=re.S) if "\n" in m.group(0)]  # not the inline notes
    for name in NEW:
        at = re.search(r"^(int|uint32_t) " + name + r"\(", txt, flags=re.M).start()
        comment = [c for end, c in blocks if end <= at][-1]
        assert "src/srs.rs:31-50,177" in comment, name


def test_null_arguments_are_refused_before_any_device_work(nat):
    lib, EINVAL = nat.lib, -1
    k = C.c_uint32(0)
    b = C.c_uint64(0)
    assert lib.dvp_prover_srs_slot_add(None, C.byref(k)) == EINVAL
    assert lib.dvp_prover_srs_slot_select(None, 0) == EINVAL
    assert lib.dvp_prover_srs_slot_drop(None, 0) == EINVAL
    assert lib.dvp_prover_srs_slot_bytes(None, 0, C.byref(b), C.byref(b)) == EINVAL
    assert lib.dvp_prover_srs_slot_active(None) == 0 and lib.dvp_prover_srs_slot_count(None) == 0
    slots, out, st = np.zeros(1, dtype=np.uint32), np.zeros(118, dtype=np.uint8), np.zeros(1, dtype=np.int32)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    assert lib.dvp_prove_multi(None, nat.ptr(slots), 1, None, 0, nat.ptr(one), 1, nat.ptr(out), nat.ptr(st)) == EINVAL
    assert lib.dvp_prove_multi_ark(None, nat.ptr(slots), 1, None, 0, nat.ptr(one), 1, nat.ptr(out), nat.ptr(st)) == EINVAL
    assert lib.dvp_prove_multi_dev(None, nat.ptr(slots), 1, nat.ptr(one), nat.ptr(out), nat.ptr(st), None) == EINVAL
    assert lib.dvp_prove_multi_be32(None, nat.ptr(slots), 1, nat.ptr(out), 1, nat.ptr(out), nat.ptr(st)) == EINVAL
    assert lib.dvp_cache_dir_add_srs_dir(None, 0, b"x", C.byref(k)) == EINVAL
    assert lib.dvp_cache_dir_add_srs_dir(b"x", 0, None, C.byref(k)) == EINVAL
    assert lib.dvp_cache_dir_slot_set_binding(None, 0, 1, None, None, 0) == EINVAL
    assert lib.dvp_prove_cache_dir_multi(b"x", 0, nat.ptr(slots), 0, None, None, 0, nat.ptr(out), nat.ptr(st)) == EINVAL  # n_slots == 0
    assert lib.dvp_prove_cache_dir_multi_ark(b"x", 0, None, 1, None, None, 0, nat.ptr(out), nat.ptr(st)) == EINVAL
    assert lib.dvp_prove_cache_dir_multi_witness_file(b"x", 0, nat.ptr(slots), 0, None, nat.ptr(out), nat.ptr(st), None) == EINVAL


def test_slots_argument(dvp):
    P = dvp.proving
    assert P._expand_slots(None, [0, 2, 5]).tolist() == [0, 2, 5]
    assert P._expand_slots([2, 0, 2], [0, 1, 2]).tolist() == [2, 0, 2]  # the caller's order, repetition allowed
    assert P._expand_slots((1,), [0, 1]).dtype == np.uint32
    assert P._expand_slots([], [0, 1]).tolist() == []  # passed on: the library answers n_slots == 0
    assert P._expand_slots(np.array([1, 0]), [0, 1]).tolist() == [1, 0]
    for bad in (3, "01", b"\x00"):
        with pytest.raises(TypeError):
            P._expand_slots(bad, [0])
    for bad in ([-1], [1 << 32]):
        with pytest.raises(ValueError):
            P._expand_slots(bad, [0])


def test_result_list_shape(dvp):
    """one entry per slot, in the order asked for: a Proof where the status is DVP_OK, else that status as a DvpError (returned, not raised)"""
    P = dvp.proving
    pv = P.Prover.__new__(P.Prover)  # no handle: the faked call below stands in for the library
    pv._h, pv._borrowed = None, True
    pv.srs_slots = lambda: [0, 1, 3]
    seen = {}

    def call(slots_ptr, n, out_ptr, st_ptr):
        seen["n"] = n
        seen["slots"] = np.ctypeslib.as_array(C.cast(slots_ptr, C.POINTER(C.c_uint32)), (n,)).tolist()
        out = np.ctypeslib.as_array(C.cast(out_ptr, C.POINTER(C.c_uint8)), (n, 118))
        st = np.ctypeslib.as_array(C.cast(st_ptr, C.POINTER(C.c_int32)), (n,))
        for j in range(n):
            out[j] = j + 1
        st[1] = -8
        return 0

    got = pv._multi(None, call, "faked")
    assert seen == {"n": 3, "slots": [0, 1, 3]} and len(got) == 3
    assert got[0] == P.Proof.from_bytes(bytes([1]) * 118) and got[2] == P.Proof.from_bytes(bytes([3]) * 118)
    assert isinstance(got[1], dvp.DvpError) and got[1].status == -8 and got[1].name == "DVP_ECHALLENGE" and "faked[1]" in str(got[1])
    got = pv._multi([3, 3], lambda s, n, o_, t: 0, "faked")
    assert seen["n"] == 3 and len(got) == 2
    with pytest.raises(dvp.DvpError) as e:  # a failure of the call itself raises
        pv._multi([0], lambda s, n, o_, t: -3, "faked")
    assert e.value.status == -3
    seen.clear()
    with pytest.raises(dvp.DvpError):
        pv._multi([], lambda s, n, o_, t: seen.update(n=n, s=s) or -1, "faked")
    assert seen == {"n": 0, "s": None}


def test_directory_list_argument(dvp, tmp_path):
    P = dvp.proving
    assert P._dirs_arg([tmp_path, str(tmp_path), b"/x"]) == [os.fsencode(tmp_path), os.fsencode(tmp_path), b"/x"]
    assert P._dirs_arg((tmp_path,)) == [os.fsencode(tmp_path)]
    for bad in (str(tmp_path), os.fsencode(tmp_path), tmp_path, None, 3, {str(tmp_path)}):
        with pytest.raises(TypeError):
            P._dirs_arg(bad)
        with pytest.raises(TypeError):
            P.Proof.prove_multi(bad, [], [1])
        with pytest.raises(TypeError):
            P.Proof.prove_multi_witness_file(bad, 0)
    with pytest.raises(ValueError):
        P._dirs_arg([])
