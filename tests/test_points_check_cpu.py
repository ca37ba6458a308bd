"""CPU tests of the affine point check (dvp_points_check, strict mode): the case set of tests/point_cases.py against the
definitions, and the parts of the ABI that need no device."""
import os
import subprocess
import sys

import c_oracle as co
import point_cases as pc
import pyref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_mul(k, pt):
    return co.k233_mul(k, pt, frob=False)  # integer double-and-add: valid on the whole curve, no trace test anywhere


def test_case_set_holds_every_class():
    cases = pc.load()
    assert 150 <= len(cases) <= 260
    for cls in pc.CLASS_NAMES:
        assert sum(1 for c in cases if c["cls"] == cls and not c["inf"]) >= 8, pc.CLASS_NAMES[cls]
    assert sum(1 for c in cases if c["inf"]) >= 16
    assert any(c["inf"] and (c["x"] >> 233) for c in cases)  # unreduced garbage behind an infinity flag
    labels = {c["label"] for c in cases}
    assert {"N", "(0,0)", "1G", "1G+N"} <= labels


def test_record_is_what_the_generator_and_the_definitions_give():
    """the recorded list is generate() again (multiples of G through the C oracle here), and every recorded class -- written from
    pyref's double-and-add -- is the class by definition with the C oracle's double-and-add"""
    cases = pc.load()
    pts = pc.generate(mul=c_mul)
    assert [(c["label"], c["x"], c["y"], c["inf"]) for c in cases] == pts
    for c in cases:
        assert pc.class_by_definition(c["x"], c["y"], c["inf"], mul=c_mul) == c["cls"], c["label"]


def test_one_class_by_pyref_itself():
    """r P = O and r (P + N) = O with pyref's own big-int arithmetic, on one recorded point of E[r] + N (seconds per multiplication)"""
    c = next(c for c in pc.load() if c["label"].startswith("random_x") and c["cls"] == pc.COSET_N)
    assert not o.k233_in_prime_subgroup((c["x"], c["y"]))
    assert o.k233_in_prime_subgroup(o.k233_add((c["x"], c["y"]), o.N_STD))


def test_definition_equals_trace_tests_on_every_case():
    for c in pc.load():
        assert pc.class_by_trace(c["x"], c["y"], c["inf"]) == c["cls"], c["label"]
        if not c["inf"] and c["cls"] in (pc.OK, pc.COSET_N, pc.ORDER4) and c["x"]:
            assert o.k233_in_prime_subgroup_fast((c["x"], c["y"])) == (c["cls"] == pc.OK), c["label"]


def test_symbols_are_exported(nat):
    for s in ("dvp_points_check", "dvp_points_check_dev", "dvp_points_set_strict", "dvp_points_get_strict"):
        assert s in nat.EXPORTED, s
    assert nat.STATUS_NAMES[-9] == "DVP_EPOINT" and nat.EPOINT == -9


def test_empty_check_needs_no_device(dvp):
    assert dvp.lib.dvp_points_check(None, None, 0, None, None) == 0
    classes, first = dvp.curve.check_points([])
    assert classes.shape == (0,) and first is None


def test_null_points_are_invalid(dvp):
    assert dvp.lib.dvp_points_check(None, None, 3, None, None) == -1


def _strict_in_child(env_value):
    env = dict(os.environ)
    env.pop("DVP_POINTS_STRICT", None)
    if env_value is not None:
        env["DVP_POINTS_STRICT"] = env_value
    code = "import importlib, sys; sys.path.insert(0, %r); print(importlib.import_module('dv-pari_amd').lib.dvp_points_get_strict())" % ROOT
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return int(out.stdout.strip().splitlines()[-1])


def test_strict_default_and_environment(dvp):
    assert _strict_in_child(None) == 0
    assert _strict_in_child("1") == 1
    assert _strict_in_child("0") == 0


def test_strict_switch_round_trip(dvp):
    prev = dvp.curve.strict_points()
    try:
        dvp.curve.set_strict_points(True)
        assert dvp.lib.dvp_points_get_strict() == 1 and dvp.curve.strict_points()
        dvp.curve.set_strict_points(False)
        assert dvp.lib.dvp_points_get_strict() == 0
    finally:
        dvp.curve.set_strict_points(prev)


def test_status_string(dvp):
    s = dvp.lib.dvp_strerror(-9)
    assert s and s != dvp.lib.dvp_strerror(-100)
    others = [dvp.lib.dvp_strerror(k) for k in (0, -1, -2, -3, -4, -6, -7, -8)]
    assert s not in others
