"""CPU tests of the circuit hash's oracle side (tests/circuit_hash_cases.py) and of what the new entries answer without a device:
the stream builder against hand-derived facts about the reference's toy circuit and against the closed-form ids and offsets on
every case, the lengths the cases promise, and the argument / file / usage errors."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pyref as o
import circuit_hash_cases as cc

P = o.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EIO = -1, -6


def test_toy_stream_by_hand():
    """the toy circuit with ONE public input: 5 real rows of 8 + 5 + 5 terms, padded to m = 8; p - 1 is not among the coefficients
    [1, 2], so it is appended at index 2 = i1 and every row's C side ends in that id; k = 1 adds no Vandermonde coefficient"""
    case = cc.BY_NAME["toy-k1"]
    s, row_bytes = cc.stream(case)
    assert row_bytes == 4 * (8 + 5 + 5 + 8) == 104
    assert len(s) == 104 + 8 + 29 * 3 == 199
    words = struct.unpack("<26I", s[:104])
    assert words[0] == 0          # row 0, A = [(5, 0)]
    assert words[:4] == (0, 0, 0, 2)  # row 0: A, B, C, then i1
    assert words[-1] == 2 and words[-3:] == (2, 2, 2)  # rows 5, 6, 7 are padding: i1 alone
    assert struct.unpack("<Q", s[104:112]) == (3,)
    assert s[112:141] == (1).to_bytes(29, "little") and s[141:170] == (2).to_bytes(29, "little")
    assert s[-29:] == (P - 1).to_bytes(29, "little") and s[-1] == 0x80


def test_toy_stream_with_two_public_inputs():
    """k = 2: one Vandermonde coefficient -d_i per row behind [1, 2, p - 1], id 3 + i"""
    case = cc.BY_NAME["toy-k2"]
    s, row_bytes = cc.stream(case)
    dom = cc.domain(3)
    assert row_bytes == 4 * (18 + 2 * 8) and len(s) == row_bytes + 8 + 29 * (3 + 8)
    assert struct.unpack("<2I", s[row_bytes - 8:row_bytes]) == (2, 3 + 7)  # row 7: i1, then n1 + 7
    assert struct.unpack("<Q", s[row_bytes:row_bytes + 8]) == (11,)
    assert s[-29:] == ((-dom[7]) % P).to_bytes(29, "little")


@pytest.mark.parametrize("case", cc.CASES, ids=repr)
def test_builder_agrees_with_the_closed_form(case):
    rows2, coeffs2 = cc.oracle_instance(case)
    i1, n1, N, off = cc.closed_form(case)
    dom, k = cc.domain(case.log_m), case.k
    assert len(coeffs2) == N and coeffs2[:len(case.coeffs)] == case.coeffs
    assert coeffs2[i1] == P - 1 and P - 1 not in coeffs2[:i1]
    for i in range(case.m):
        for j in range(1, k):
            assert coeffs2[n1 + i * (k - 1) + (j - 1)] == (-pow(dom[i], j, P)) % P
    words, pos = [], 0
    for i, row in enumerate(rows2):
        assert pos == off[i], (i, pos, off[i])  # rpA[min(i, nA)] + rpB[..] + rpC[..] + k i
        ids = [cid for side in row for _, cid in side]
        own = sum(len(mt[i]) for mt in case.mats if i < len(mt))
        assert len(ids) == own + k
        assert ids[own:] == ([i1] if k else []) + [n1 + i * (k - 1) + (j - 1) for j in range(1, k)]
        words += ids
        pos += len(ids)
    assert pos == off[case.m]
    s, row_bytes = cc.stream(case)
    assert row_bytes == 4 * pos and s[:row_bytes] == struct.pack(f"<{pos}I", *words)
    assert len(s) == row_bytes + 8 + 29 * N
    assert N <= 1 << 32


def test_the_cases_are_what_they_claim():
    n = {c.name: len(cc.stream(c)[0]) for c in cc.CASES}
    assert n["toy-k0"] <= 1024 and n["toy-k1"] <= 1024  # the single-chunk ROOT path
    assert (n["bytes-1024"], n["bytes-1025"], n["bytes-2048"]) == (1024, 1025, 2048)
    assert [cc.closed_form(cc.BY_NAME[x])[0] for x in ("m1-absent", "m1-first", "m1-middle", "m1-twice")] == [3, 0, 2, 1]
    assert cc.closed_form(cc.BY_NAME["toy-k0"])[1:3] == (3, 3)  # k = 0 still appends p - 1
    assert cc.closed_form(cc.BY_NAME["toy-k1"])[2] == 3 and cc.closed_form(cc.BY_NAME["toy-k5"])[2] == 3 + 8 * 4
    rec = cc.stream(cc.BY_NAME["coeff-values"])[0]
    row_bytes = cc.stream(cc.BY_NAME["coeff-values"])[1]
    tops = {rec[row_bytes + 8 + 29 * i + 28] for i in range(6)}
    assert {0, 0x80, 0x01, 0x7F} <= tops  # the 29th byte of 0 / 1, of p - 1, of 2^224 + .., of 127 2^224
    ragged = cc.BY_NAME["ragged-rows"]
    assert [len(mt) for mt in ragged.mats] == [9, 13, 11] and ragged.m == 16
    assert any(not r for mt in ragged.mats for r in mt)  # empty rows inside a matrix
    em = cc.BY_NAME["empty-matrices"]
    assert em.mats[1] == [] and em.row_ptrs()[2] == [0] * 7
    assert max(len(r) for r in cc.BY_NAME["long-row"].mats[1]) == 300
    assert cc.straddled_edges(cc.BY_NAME["long-row"], 1)[0]  # a row crosses a window edge at window = 1 chunk
    sp = cc.BY_NAME["sparse-8"]
    s, row_bytes = cc.stream(sp)
    assert 20_000 < len(s) < 100_000 and row_bytes % 1024 != 0  # the part boundary lies strictly inside a chunk
    for w in (1, 2, 3):
        in_row, in_rec = cc.straddled_edges(sp, w)
        assert in_row and in_rec, w  # a row and a 29-byte record straddle a window edge at every tested window size
    assert cc.rows_spanned_by_256_dwords(cc.BY_NAME["ids-only"]) == 256 and cc.rows_spanned_by_256_dwords(cc.BY_NAME["mostly-empty"]) > 200
    assert cc.rows_spanned_by_256_dwords(sp) < 64
    changed = cc.toy_with_changed_coeff_id(2)
    assert cc.stream_of(*cc.oracle_instance(changed))[0] != cc.stream(cc.BY_NAME["toy-k2"])[0]


def test_entries_without_a_device(dvp, nat, tmp_path):
    """NULL arguments are DVP_EINVAL; a directory without a dump, a truncated dump and a dump whose coefficient id leaves the table
    are DVP_EIO before any device is needed"""
    lib, ptr = dvp.lib, nat.ptr
    out = np.zeros(32, dtype=np.uint8)
    assert lib.dvp_prover_circuit_hash(None, ptr(out)) == EINVAL
    assert lib.dvp_circuit_hash_cache_dir(None, 2, ptr(out)) == EINVAL
    assert lib.dvp_circuit_hash_cache_dir(os.fsencode(tmp_path), 2, None) == EINVAL
    assert lib.dvp_circuit_hash_cache_dir(os.fsencode(tmp_path / "nowhere"), 2, ptr(out)) == EIO
    assert lib.dvp_circuit_hash_cache_dir(os.fsencode(tmp_path), 2, ptr(out)) == EIO  # no r1cs_to_dvsnark in it
    dump = cc.py_dump(o.TOY_ROWS, o.TOY_COEFFS)
    name = dvp.artifacts.R1CS_CONSTRAINTS_FILE
    (tmp_path / name).write_bytes(dump[:-5])
    assert lib.dvp_circuit_hash_cache_dir(os.fsencode(tmp_path), 2, ptr(out)) == EIO
    (tmp_path / name).write_bytes(cc.py_dump([([(0, 2)], [], [])], [1, 2]))
    assert lib.dvp_circuit_hash_cache_dir(os.fsencode(tmp_path), 2, ptr(out)) == EIO
    assert not out.any()
    with pytest.raises(dvp.DvpError) as e:
        dvp.proving.circuit_hash_cache_dir(tmp_path / "nowhere", 2)
    assert e.value.status == EIO
    v = C.c_longlong(-1)
    assert lib.dvp_tune_get(b"DVP_CIRCUIT_HASH_WINDOW", C.byref(v)) == 0 and v.value == 0  # the default window
    with nat.tune(DVP_CIRCUIT_HASH_WINDOW=3):
        assert lib.dvp_tune_get(b"DVP_CIRCUIT_HASH_WINDOW", C.byref(v)) == 0 and v.value == 3
    names = nat.lib.dvp_debug_launch_names(None, 0)
    buf = C.create_string_buffer(names)
    nat.lib.dvp_debug_launch_names(buf, names)
    listed = buf.value.decode().split("\n")
    for k in ("k_ch_row_starts", "k_ch_rows", "k_ch_coeffs", "k_ch_find_minus_one"):
        assert "circuit_hash.hip:" + k in listed


def test_cli_bind_circuit_excludes_circuit_hash(tmp_path):
    """--bind-circuit together with --circuit-hash is a usage error (exit 2), said before any device or file is touched"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    libdir = os.path.join(ROOT, "dv-pari_amd")
    exe = tmp_path / "dvp_prove_cli"
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "dvp_prove_cli.cpp"), "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-pthread",
                           "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path / "nowhere"), "2", "--bind-circuit", "--circuit-hash", "ab" * 32], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2 and "exclude each other" in out.stderr and "usage:" in out.stderr, (out.returncode, out.stderr)
    out = subprocess.run([str(exe), str(tmp_path / "nowhere"), "2", "--bind-circuit"], capture_output=True, text=True, timeout=120)
    assert out.returncode in (1, 3), (out.returncode, out.stderr)  # accepted as an option: no device (3) or no such directory (1)
