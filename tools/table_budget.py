"""ms per 2^20-constraint proof under a table budget (dvp_prover_set_table_budget): 0, 1/4, 1/2, 3/4 and all of the full table
size, plus no limit.  Every budget runs in a child process of its own under its own time limit, and the sweep stops at the first
child that does not exit with 0.  Times are device events around dvp_prove_dev, median of 5 after warm-up, with min and max.

    python tools/table_budget.py [--log-m 20] [--timeout 300] [--json out.json]

Yardsticks: "unlimited" is the default prover's figure, budget 0 the all-one-shot figure.  A budget in between that is slower
than budget 0 by more than the spread of its five repetitions is a planner defect."""
import argparse
import importlib
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
REPS, WARM = 5, 3


def one(log_m: int, budget):
    import numpy as np
    import torch

    dvp = importlib.import_module("dv-pari_amd")
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(log_m)
    td = dvp.srs.Trapdoor(0x1234567 + (1 << 200), 0x7654321 + (1 << 190), 0xABCDEF + (1 << 180))
    w = torch.from_numpy(dvp.fr.vec([1] + pub + prv).view(np.int64)).cuda()
    pv = dvp.proving.Prover(inst)
    pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, td))
    s0, s1 = pv.msm_size(0), pv.msm_size(1)
    full = sum(dvp.table_plan(s0, s1, None)[1])
    nbytes = None if budget == "unlimited" else int(round(float(budget) * full))
    pv.set_table_budget(nbytes)
    st = torch.cuda.current_stream().cuda_stream
    proof = None
    for _ in range(WARM):
        proof = pv.prove_dev(w.data_ptr(), st)
    assert dvp.srs.verify(td, pub, proof), "proof rejected"
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert pv.prove_dev(w.data_ptr(), st) == proof
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    cov = [pv.msm_coverage(k) for k in (0, 1)]
    out = {"log_m": log_m, "budget": budget, "budget_bytes": nbytes, "full_bytes": full, "ms_median": sorted(ms)[REPS // 2], "ms_min": min(ms),
           "ms_max": max(ms), "covered": [c[0] for c in cov], "total": [c[1] for c in cov], "reason": [c[2] for c in cov],
           "table_bytes": [pv.msm_table(k)[0] for k in (0, 1)], "proof": proof.to_bytes().hex()}
    pv.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per budget")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", default=None, help="(child) one budget: a fraction of the full table size, or 'unlimited'")
    a = ap.parse_args()
    if a.one is not None:
        one(a.log_m, a.one)
        return 0
    rows = []
    for budget in ("0", "0.25", "0.5", "0.75", "1", "unlimited"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--log-m", str(a.log_m), "--one", budget], capture_output=True, text=True,
                               timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"budget {budget}: no result within {a.timeout} s, stopping", flush=True)
            return 124
        if r.returncode != 0:
            print(f"budget {budget}: exit {r.returncode}, stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return r.returncode if r.returncode > 0 else 1
        row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        rows.append(row)
        print(f"budget {budget:>9}: {row['ms_median']:.2f} ms (min {row['ms_min']:.2f}, max {row['ms_max']:.2f})  MSM 1 {row['covered'][1]}/{row['total'][1]}"
              f"  MSM 0 {row['covered'][0]}/{row['total'][0]}  tables {sum(row['table_bytes']) / 2**30:.2f} GiB", flush=True)
    if len({r["proof"] for r in rows}) != 1:
        print("proof bytes differ between budgets", flush=True)
        return 1
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
