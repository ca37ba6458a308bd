"""One witness for N verifiers: N provers, one prover with its SRS set again per verifier, or dvp_prove_multi_dev over N SRS slots.

    python tools/prove_multi.py [--log-m 16,20] [--slots 1,2,4,8] [--kinds dense,sparse] [--budget BYTES] [--reps 7] [--out out.json]

Per instance (gnark_r1cs.synthetic_dense and the SP1-like synthetic_sparse_fast), size and number of verifiers N, with the assignment
resident in HBM and N SRSs from N trapdoors (srs.verifier_runs_setup):

  (a) N separate provers, one SRS each, proving back to back (dvp_prove_dev on each);
  (b) one prover whose SRS is set again for every verifier (the five setters, then dvp_prove_dev): copy, check and table build per switch;
  (c) one prover with N SRS slots, one dvp_prove_multi_dev.

Each leg is warmed up (tables and workspaces exist, (b) excepted: building them again per switch is what it measures), then timed
--reps times with the host clock around calls that end in the proof's own stream wait, the three legs alternating inside every
repetition; the median, the minimum and the maximum of the repetitions are reported per leg, in ms for all N proofs.  Every proof of
every repetition is compared with leg (a)'s.  Free HBM (hipMemGetInfo, through torch) is read before a leg's provers exist and after
its warm-up, beside the sum of dvp_prover_srs_slot_bytes over its slots; a scratch prover proves once before either, so that the
process-wide MSM workspaces exist and are charged to neither.  A last pass under dvp_profile_enable(1) -- its events cost
time, so it is not part of the timed repetitions -- reads prove_total, msm_total, msm_sort and extend_total for one single proof and
for one prove_multi: msm_sort per proof is the share a reuse of the commitment MSM's recode and sort across slots could at most
remove, and (other_N - other_1) / (N - 1), other = prove_total - msm_total, is what a slot after the first spends outside its two
MSMs: the transcript and the challenge stages."""
import argparse
import ctypes as C
import importlib
import json
import os
import random
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
import numpy as np  # noqa: E402
import torch  # noqa: E402

dvp = importlib.import_module("dv-pari_amd")
P = dvp.fr.P


def prof(name):
    ms, n = C.c_double(0), C.c_uint64(0)
    dvp.check(dvp.lib.dvp_profile_read(name.encode(), C.byref(ms), C.byref(n)), name)
    return ms.value, int(n.value)


def free_hbm():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def profile_pass(run, n_proofs):
    dvp.lib.dvp_profile_enable(1)
    dvp.lib.dvp_profile_reset()
    run()
    torch.cuda.synchronize()
    out = {k: round(prof(k)[0], 4) for k in ("prove_total", "msm_total", "msm_sort", "extend_total")}
    dvp.lib.dvp_profile_enable(0)
    out["other"] = round(out["prove_total"] - out["msm_total"], 4)
    out["msm_sort_share_of_prove"] = round(out["msm_sort"] / out["prove_total"], 4) if out["prove_total"] else None
    out["proofs"] = n_proofs
    return out


def one_config(a, kind, lg, n_list):
    g = dvp.gnark_r1cs
    inst, pub, prv = g.synthetic_dense(lg) if kind == "dense" else g.synthetic_sparse_fast(lg)
    dev = torch.device("cuda", 0)
    if isinstance(prv, np.ndarray):  # synthetic_sparse_fast hands the witness over as limbs
        w = np.concatenate([dvp.fr.vec([1]), np.asarray(pub, dtype=np.uint64).reshape(-1, 4), prv.reshape(-1, 4)])
    else:
        w = dvp.fr.vec([1] + list(pub) + list(prv))
    assignment = torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(dev)
    d_w = assignment.data_ptr()
    rnd = random.Random(1000 + lg)
    n_max = max(n_list)
    scratch = dvp.proving.Prover(inst)
    srss = [dvp.srs.verifier_runs_setup(scratch, inst, dvp.srs.Trapdoor(rnd.randrange(1, P), rnd.randrange(1, P), rnd.randrange(1, P)))
            for _ in range(n_max)]
    # one proof on the scratch prover: the MSM workspaces are the process's, not a prover's, and would otherwise be charged to
    # whichever leg proves first
    scratch.set_table_budget(a.budget)
    scratch.set_srs(srss[0])
    scratch.prove_dev(d_w)
    scratch.close()
    rows = []
    for n in n_list:
        row = {"kind": kind, "log_m": lg, "n_wires": inst.n_wires, "verifiers": n, "table_budget": a.budget}
        # (a) N provers
        f0 = free_hbm()
        provers = []
        for j in range(n):
            q = dvp.proving.Prover(inst)
            q.set_table_budget(a.budget)
            q.set_srs(srss[j])
            provers.append(q)
        ref = [q.prove_dev(d_w) for q in provers]
        assert ref == [q.prove_dev(d_w) for q in provers]
        row["a_hbm_used"] = f0 - free_hbm()
        row["a_slot_bytes"] = [sum(q.srs_slot_bytes(0)[k] for q in provers) for k in (0, 1)]
        # (c) one prover, N slots
        f0 = free_hbm()
        mp = dvp.proving.Prover(inst)
        mp.set_table_budget(a.budget)
        mp.set_srs(srss[0])
        for j in range(1, n):
            k = mp.add_srs(srss[j])
            mp.select_srs(k)
            mp.set_table_budget(a.budget)
            mp.select_srs(0)
        assert mp.prove_multi_dev(d_w) == ref and mp.prove_multi_dev(d_w) == ref
        row["c_hbm_used"] = f0 - free_hbm()
        row["c_slot_bytes"] = [sum(mp.srs_slot_bytes(j)[k] for j in mp.srs_slots()) for k in (0, 1)]
        # (b) one prover, its SRS set again per verifier
        sp = dvp.proving.Prover(inst)
        sp.set_table_budget(a.budget)

        def leg_a():
            return [q.prove_dev(d_w) for q in provers]

        def leg_b():
            out = []
            for j in range(n):
                sp.set_srs(srss[j])
                out.append(sp.prove_dev(d_w))
            return out

        def leg_c():
            return mp.prove_multi_dev(d_w)

        assert leg_b() == ref
        times = {"a": [], "b": [], "c": []}
        for _ in range(a.reps):
            for name, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = leg()
                times[name].append((time.perf_counter() - t0) * 1e3)
                assert got == ref, name
        for name in "abc":
            row[name] = stats(times[name])
        row["c_over_a"] = round(row["c"]["ms_median"] / row["a"]["ms_median"], 4)
        row["c_over_b"] = round(row["c"]["ms_median"] / row["b"]["ms_median"], 4)
        row["profile_single"] = profile_pass(lambda: provers[0].prove_dev(d_w), 1)
        row["profile_multi"] = profile_pass(leg_c, n)
        if n > 1:
            row["per_slot_outside_msm_ms"] = round((row["profile_multi"]["other"] - row["profile_single"]["other"]) / (n - 1), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        for q in provers + [mp, sp]:
            q.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-m", default="16,20")
    ap.add_argument("--slots", default="1,2,4,8")
    ap.add_argument("--kinds", default="dense,sparse")
    ap.add_argument("--budget", type=int, default=None, help="table budget in bytes per prover and per slot (default: no limit)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert dvp.lib.dvp_device_count() > 0, "no HIP device visible: nothing here can be measured without one"
    rows = []
    for kind in a.kinds.split(","):
        for lg in (int(x) for x in a.log_m.split(",")):
            rows += one_config(a, kind, lg, sorted(int(x) for x in a.slots.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
