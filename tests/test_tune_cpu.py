"""The tuning knobs by name (no GPU needed, no device call): every knob of struct Tune (csrc/common.h) is reachable through dvp_tune_get /
dvp_tune_set under its DVP_ name, starts at its default, is read from the environment variable of the same name, and dvp_tune_reset
goes back to what the environment says.  The list below is written out, not read from the library: a knob that loses its name, changes
its default or stops being read from the environment fails here.  Every case runs in a fresh child process, because the knobs are
process-wide state that other tests set and the environment is read once."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dv-pari_amd", "libdvpari_hip.so")
DVP_EINVAL = -1

KNOBS = [
    ("DVP_MSM_C", 0),
    ("DVP_MSM_K", 0),
    ("DVP_MSM_FIXED_C", 0),
    ("DVP_FX_HI", -1),
    ("DVP_MSM_PROJ", 0),
    ("DVP_MSM_AFF_MIN", 1 << 19),
    ("DVP_MSM_GATE_MIN", 1),
    ("DVP_MSM_WS_SLOTS", 2),
    ("DVP_CACHE_REPLICAS", 1),
    ("DVP_MSM_AFF_TPB", 256),
    ("DVP_MSM_AFF_BMIN", 8),
    ("DVP_MSM_AFF_SHARE_INV", 2),
    ("DVP_MSM_AFF_SHARE_MIN", 0),
    ("DVP_MSM_AFF_BMAX", 136),
    ("DVP_ECFFT_RADIX4", 3),
    ("DVP_ECFFT_FOLD", 1),
    ("DVP_MSM_ACCUM_FAST", 1),
    ("DVP_MSM_TAIL_GROUPS", 1),
    ("DVP_MSM_ACCUM_HEX_MAX", -1),
    ("DVP_GF_INV_TABS", 1),
    ("DVP_MSM_ACCUM_QUAD_MAX", 0),
    ("DVP_MSM_BUCKET_PAIRS_MAX", 12),
    ("DVP_MSM_SORT_FUSED", 1),
    ("DVP_MSM_ROUND_PIPELINE", 2),
    ("DVP_MSM_ROUND_DENSE", 0),
    ("DVP_MSM_HEX_MAX", -1),
    ("DVP_MSM_QUAD_MAX", 0),
    ("DVP_MSM_FIXED_MIN", 1 << 16),
    ("DVP_FR_BI_SHAPE", 6),
    ("DVP_HORNER_MAX_PUB", -1),
    ("DVP_PROVE_HOST_TRANSCRIPT", 0),
    ("DVP_TABLE_BUDGET_BYTES", -1),
    ("DVP_MSM_TABLE_REFUSE", 0),
    ("DVP_POINTS_MUL_W", 3),
    ("DVP_MSM_SEG_PIECE", 4),
    ("DVP_CIRCUIT_HASH_WINDOW", 0),
    ("DVP_MSM_ALIGNED_SIGNED", 1),
]
NAMES = [n for n, _ in KNOBS]
DEFAULTS = dict(KNOBS)

# argv: library, JSON list of names.  Prints every knob as the fresh process sees it, then after setting knob i to 1000 + i, then after
# dvp_tune_reset, and the status of an unknown and of a null name; "get" = [status, value], the value preset to a sentinel
CHILD = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
names = json.loads(sys.argv[2])
lib.dvp_tune_get.argtypes = [C.c_char_p, C.POINTER(C.c_longlong)]
lib.dvp_tune_set.argtypes = [C.c_char_p, C.c_longlong]
lib.dvp_tune_reset.restype = None
def get(n):
    v = C.c_longlong(0x5a5a5a5a)
    return [lib.dvp_tune_get(None if n is None else n.encode(), C.byref(v)), v.value]
out = {"first": {n: get(n) for n in names}}
out["set"] = [lib.dvp_tune_set(n.encode(), 1000 + i) for i, n in enumerate(names)]
out["after_set"] = {n: get(n) for n in names}
lib.dvp_tune_reset()
out["after_reset"] = {n: get(n) for n in names}
out["unknown"] = [get("DVP_NO_SUCH_KNOB"), lib.dvp_tune_set(b"DVP_NO_SUCH_KNOB", 1), get(None), lib.dvp_tune_set(None, 1)]
out["null_value"] = lib.dvp_tune_get(names[0].encode(), None)
print(json.dumps(out))
"""


def _child(env_knobs):
    """the child's report with exactly env_knobs as its DVP_* environment"""
    if not os.path.exists(LIB):
        pytest.skip("libdvpari_hip.so is not built")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVP_")}
    env.update({k: str(v) for k, v in env_knobs.items()})
    r = subprocess.run([sys.executable, "-c", CHILD, LIB, json.dumps(NAMES)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def bare():
    return _child({})


def test_the_list_is_the_whole_struct():
    assert len(KNOBS) == 37 and len(set(NAMES)) == 37


def test_defaults(bare):
    assert bare["first"] == {n: [0, d] for n, d in KNOBS}


def test_set_get_round_trip(bare):
    assert bare["set"] == [0] * len(NAMES)
    assert bare["after_set"] == {n: [0, 1000 + i] for i, n in enumerate(NAMES)}


def test_reset_restores_defaults(bare):
    assert bare["after_reset"] == {n: [0, d] for n, d in KNOBS}


def test_unknown_and_null_names_are_einval(bare):
    get_unknown, set_unknown, get_null, set_null = bare["unknown"]
    assert get_unknown == [DVP_EINVAL, 0x5A5A5A5A] and get_null == [DVP_EINVAL, 0x5A5A5A5A]  # nothing written
    assert set_unknown == DVP_EINVAL and set_null == DVP_EINVAL
    assert bare["null_value"] == DVP_EINVAL


def test_every_knob_is_read_from_its_environment_variable():
    want = {n: 101 + i for i, n in enumerate(NAMES)}
    got = _child({**want, "DVP_MSM_MODE": "proj"})
    want["DVP_MSM_PROJ"] = 1  # read as DVP_MSM_MODE=proj only: the variable DVP_MSM_PROJ (set to 105 here) is ignored
    assert got["first"] == {n: [0, v] for n, v in want.items()}
    assert got["after_reset"] == got["first"]  # a reset goes back to the environment, not to the defaults


def test_msm_proj_variable_alone_is_ignored():
    got = _child({"DVP_MSM_PROJ": 1})
    assert got["first"] == {n: [0, d] for n, d in KNOBS}
    assert _child({"DVP_MSM_MODE": "affine"})["first"]["DVP_MSM_PROJ"] == [0, 0]


def test_table_budget_takes_the_full_u64_range():
    def budget(text):
        return _child({"DVP_TABLE_BUDGET_BYTES": text})["first"]["DVP_TABLE_BUDGET_BYTES"]

    assert budget("18446744073709551615") == [0, -1]
    assert budget(str((1 << 63) - 1)) == [0, (1 << 63) - 1] and budget(str(1 << 63)) == [0, -1]
