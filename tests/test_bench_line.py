"""bench.py's ONE JSON line stays machine-readable: the driver keeps an 8 126-character tail of stdout, so the line must be well under
that and must carry the contract's keys (round 5's 25 KB line left BENCH_r05.json with parsed = null).  Canned input: the full
document of a real run (profiles/r05_bench_prove2p20.json, prose and per-round tables included), so no GPU is needed; only the
last test (-m gpu) runs a small plain benchmark and checks the proof it dumps."""
import copy
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (importing bench.py touches neither torch nor the GPU)

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config", "roofline", "cpu_baseline")


def _full():
    return json.load(open(os.path.join(ROOT, "profiles", "r05_bench_prove2p20.json")))


def _check(line):
    assert "\n" not in line
    assert len(line) < bench.LINE_LIMIT < 8126 - 1500, len(line)
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    assert list(d)[:7] == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step"]
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "work_model_frac"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6 * max(1.0, r["frac"])
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port")
    # a bounded tail of stdout (what the driver keeps) still holds the whole line
    tail = ("x" * 20000 + "\n" + line + "\n")[-8126:]
    assert json.loads(tail.splitlines()[-1]) == d
    return d


def test_headline_from_a_full_run_fits_and_has_the_contract_keys():
    full = _full()
    assert len(json.dumps(full)) > 20000  # the canned document really is the oversized one
    d = _check(json.dumps(bench.headline(full, "gpurun_out/bench_detail.json")))
    assert abs(d["value"] - full["value"]) / full["value"] < 1e-5
    assert abs(d["ms_per_step"] - full["ms_per_step"]) / full["ms_per_step"] < 1e-5
    assert d["detail"] == "gpurun_out/bench_detail.json"
    assert "_note" not in json.dumps(d) and '"reading"' not in json.dumps(d)


def test_headline_of_an_eight_rank_run_fits():
    full = copy.deepcopy(_full())
    full["n_gpus"] = 8
    full.pop("cpu_baseline")
    full.update({"rccl_ranks": 8, "backend": "nccl", "ms_per_step_ranks": [5.123456789] * 8, "ms_per_step_inproc": 6.54321,
                 "replicas": {"n": 8, "constraints_per_s": 4.4e8, "ms_per_proof_each": [19.1] * 8},
                 "shard_plan": [{"rank": r, "commit_msm_range": [0, 1], "k_msm_range": [0, 1], "extends": True, "pairs": 1} for r in range(8)],
                 "stages_ms_per_step_by_rank": [{"rank": r, "x" * 30: 1.0} for r in range(8)]})
    full["config"]["sharding"] = "y" * 500
    line = json.dumps(bench.headline(full, None))
    assert len(line) < bench.LINE_LIMIT
    d = json.loads(line)
    assert d["rccl_ranks"] == 8 and len(d["ms_per_step_ranks"]) == 8 and "shard_plan" not in d


def test_no_prose_keys_are_built_in_bench_py():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '_note"' not in src and '"reading"' not in src and '"note"' not in src


def test_headline_of_a_plain_run_has_the_contract_keys_and_nothing_measured_under_full():
    """a plain run (no --full) measures no roofline, stages or CPU baseline and writes no sidecar: its line carries the headline
    keys and the configuration only"""
    full = _full()
    plain = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                  "vs_baseline", "dtype", "data")}
    plain["config"] = {k: full["config"][k] for k in ("workload", "log2_constraints", "n_wires", "msm_pairs_per_proof", "sharding", "witness",
                                                      "entry", "proofs_in_flight")}
    plain["scaling_measured"] = False
    d = json.loads(json.dumps(bench.headline(plain)))
    assert list(d)[:7] == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step"]
    for k in ("higher_is_better", "dtype", "config"):
        assert d[k] == bench._sig(plain[k]), k
    for k in ("roofline", "cpu_baseline", "stages_ms_per_step", "roofline_by_config", "throughput_two_in_flight"):
        assert k not in d, k
    assert d["detail"] is None


def test_dump_outputs_writes_every_proof_byte_exactly(tmp_path):
    import types

    import numpy as np

    rng = np.random.default_rng(5)
    fields = {name: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for name, n in (("commit_p", 30), ("kzg_k", 30), ("a0", 29), ("b0", 29))}
    bench.dump_outputs(str(tmp_path / "out"), types.SimpleNamespace(**fields))
    got = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert got == ["proof_a0.npy", "proof_b0.npy", "proof_commit_p.npy", "proof_kzg_k.npy"]
    for name, raw in fields.items():
        a = np.load(tmp_path / "out" / f"proof_{name}.npy")
        assert a.dtype == np.float64 and a.shape == (len(raw),)
        assert a.astype(np.uint8).tobytes() == raw


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_timed_proof(dvp, tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1` at 2^12 constraints with --dump-outputs: one line with the headline keys, no
    sidecar, and the dumped proof is the proof of the same seeded instance computed here -- and it verifies"""
    import subprocess

    import numpy as np

    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log-m", "12",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - (1 << 12) / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-4
    assert "roofline" not in d and "cpu_baseline" not in d and d["detail"] is None
    got = b"".join(np.load(out_dir / f"proof_{n}.npy").astype(np.uint8).tobytes() for n in ("commit_p", "kzg_k", "a0", "b0"))
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(12)
    td = dvp.srs.Trapdoor(*bench.TRAPDOOR)  # the trapdoor bench.py proves with
    pv = dvp.proving.Prover(inst)
    try:
        pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, td))
        proof = pv.prove(pub, prv)
    finally:
        pv.close()
    assert got == proof.to_bytes()
    assert dvp.srs.verify(td, pub, dvp.proving.Proof.from_bytes(got))


@pytest.mark.gpu
def test_steps_sets_the_number_of_timed_proofs(dvp):
    """--steps K times K proofs, warm-up excluded: counted by the library, not echoed by bench.py.  Every MSM records one
    first-round event scope (the pair-round path and the small-input path alike) and a proof runs two MSMs, so the timed loop
    of a --full run records 2 K of them"""
    import subprocess

    steps = 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--log-m", "12", "--no-cpu-baseline", "--no-extras", "--in-flight", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == steps and d["roofline"]["launches"] == 2 * steps, d["roofline"]
