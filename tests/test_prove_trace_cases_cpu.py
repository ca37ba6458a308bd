"""The prove trace without a GPU: the restated Fr-vector stream (tests/prove_trace_cases.py) is the file the Fr-vector writer produces,
the text form of a record round-trips, the ctypes mirror of dvp_prove_trace has the size the header asserts, and the library exports
the entries."""
import ctypes as C
import os
import re

import pytest

import pyref as o
import prove_trace_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", sorted(tc.LENGTHS))
def test_stream_is_the_fr_vec_file(dvp, tmp_path, n):
    vals = tc.values(n)
    path = tmp_path / f"v{n}"
    dvp.io_utils.write_fr_vec_to_file(path, dvp.fr.vec(vals) if n else dvp.fr.vec([0])[:0])
    data = path.read_bytes()
    s = tc.fr_stream(vals)
    assert len(s) == 8 + 29 * n and data == s
    assert o.blake3(s) == o.blake3(data) == tc.digest_of_values(n)


def test_lengths_hit_the_shapes_they_name():
    assert [8 + 29 * n for n in sorted(tc.LENGTHS)] == [8, 37, 66, 704, 1023, 1052, 17408, 17437]
    assert [tc.chunks_of(n) for n in (0, 35, 36, 600, 601)] == [1, 1, 2, 17, 18]
    for k in (511, 512, 513):
        n = tc.length_for_chunks(k)
        assert tc.chunks_of(n) == k and tc.chunks_of(n + 1) == k + 1


def test_format_parse_round_trip(dvp):
    rec = tc.sample_record()
    text = dvp.proving.format_prove_trace(rec)
    assert dvp.proving.parse_prove_trace(text) == rec
    assert dvp.proving.parse_prove_trace("proof = 00\n" + text + "\nnot a field line\n") == rec  # the CLI's surroundings are skipped
    names = [ln.split(" = ")[0] for ln in text.splitlines()]
    assert len(names) == len(set(names)) == 6 + 6 + 4 * 7 + 16
    for f in tc.DIGEST_NAMES + tc.SCALAR_NAMES:
        assert f in names
    for f in tc.POINT_NAMES:
        assert {f + "_x", f + "_y", f + "_inf", f + "_enc"} <= set(names)


def test_ctypes_mirror_has_the_headers_size(nat):
    hdr = open(os.path.join(ROOT, "include", "dvpari.h")).read()
    mt = re.search(r"sizeof\(dvp_trace_point\) == (\d+) && sizeof\(dvp_prove_trace\) == (\d+)", hdr)
    assert mt, "the static_assert on dvp_prove_trace is gone"
    assert (C.sizeof(nat.TracePoint), C.sizeof(nat.ProveTrace)) == (int(mt.group(1)), int(mt.group(2)))
    assert C.sizeof(nat.ProveTrace) == nat.PROVE_TRACE_BYTES
    assert tuple(name for _, name in nat.TRACE_DIGESTS) == tc.DIGEST_NAMES
    assert (nat.TRACE_SCALARS, nat.TRACE_POINTS) == (tc.SCALAR_NAMES, tc.POINT_NAMES)
    assert nat.ProveTrace.alpha.offset == 24 and nat.ProveTrace.msm_gm.offset == 216 and nat.ProveTrace.assignment.offset == 888


def test_library_exports_the_entries(nat):
    for name in ("dvp_fr_vec_digest", "dvp_fr_vec_digest_dev", "dvp_prover_trace_last"):
        assert hasattr(nat.lib, name) and name in nat.EXPORTED, name
    v = C.c_longlong(-5)
    assert nat.lib.dvp_tune_get(b"DVP_FR_DIGEST_WINDOW", C.byref(v)) == 0 and v.value == 0  # the default window
