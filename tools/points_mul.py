#!/usr/bin/env python3
"""dvp_points_mul_dev (k_points_mul<w>) against its yardstick, k_mulgen, on the same scalars and count in the same run.

    python tools/points_mul.py [--json out.json] [--min-log 10] [--max-log 20]

For n = 2^10 .. 2^20 and w = 3, 4, 5 (DVP_POINTS_MUL_W through dvp_tune_set): device events around dvp_points_mul_dev and around
k_mulgen alone (dvp_ubench_points_mul: one warm-up each, then the median of 5), the widths taken in turn WITHIN a size so that
they share whatever else the box is doing.  The inputs are seeded: points k_i G from the library's fixed-base multiplication,
scalars uniform below r.  Before anything is timed the products of the first 64 lanes are compared with the C oracle's integer
double-and-add for every w: a faster wrong kernel is not measured.  Small n is one dependent chain per lane (latency); the rate
column only means throughput once n fills the chip (2^16 lanes and up)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
REPS = 5
WIDTHS = (3, 4, 5)
KNOB = b"DVP_POINTS_MUL_W"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--min-log", type=int, default=10)
    ap.add_argument("--max-log", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch

    import c_oracle as co
    from util import np_to_pt, rand_fr_np

    dvp = importlib.import_module("dv-pari_amd")
    lib, check = dvp.lib, dvp.check
    n_max = 1 << a.max_log
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(rand_fr_np(n_max, 5))
    assert not inf.any()
    ks = rand_fr_np(n_max, 6)
    t_xy = torch.from_numpy(xy.view(np.int64)).cuda()
    t_s = torch.from_numpy(ks.view(np.int64)).cuda()
    t_scratch = torch.empty(n_max * 65, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    prev = C.c_longlong(0)
    check(lib.dvp_tune_get(KNOB, C.byref(prev)))
    rows = []
    try:
        want = [co.k233_mul(int.from_bytes(ks[i].tobytes(), "little"), np_to_pt(xy[i]), frob=False) for i in range(64)]
        for w in WIDTHS:
            check(lib.dvp_tune_set(KNOB, w))
            got_xy, got_inf = dvp.curve.point_scalar_mul(ks[:64], xy[:64])
            assert not got_inf.any() and [np_to_pt(got_xy[i]) for i in range(64)] == want, w
        for log_n in range(a.min_log, a.max_log + 1):
            n = 1 << log_n
            row = dict(log_n=log_n)
            gen = []
            for w in WIDTHS:
                check(lib.dvp_tune_set(KNOB, w))
                mul_ms, gen_ms = C.c_double(0), C.c_double(0)
                check(lib.dvp_ubench_points_mul(t_s.data_ptr(), t_xy.data_ptr(), n, t_scratch.data_ptr(), REPS, C.byref(mul_ms), C.byref(gen_ms)),
                      "dvp_ubench_points_mul")
                row[f"w{w}_ms"] = mul_ms.value
                gen.append(gen_ms.value)
            row["mulgen_ms"] = sorted(gen)[1]
            best = min(WIDTHS, key=lambda w: row[f"w{w}_ms"])
            row["best_w"] = best
            row["ratio_best"] = row[f"w{best}_ms"] / row["mulgen_ms"]
            rows.append(row)
            print(f"2^{log_n:2d}: " + "  ".join(f"w={w} {row[f'w{w}_ms']:9.3f} ms ({n / row[f'w{w}_ms'] / 1e3:7.2f} M/s)" for w in WIDTHS)
                  + f"  k_mulgen {row['mulgen_ms']:8.3f} ms ({n / row['mulgen_ms'] / 1e3:7.2f} M/s)  best w={best}, {row['ratio_best']:.2f} x k_mulgen", flush=True)
    finally:
        lib.dvp_tune_set(KNOB, prev.value)
    print(f"default DVP_POINTS_MUL_W in this build: {prev.value}; fastest at 2^{rows[-1]['log_n']}: w={rows[-1]['best_w']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows, default_w=prev.value, device=torch.cuda.get_device_name(0)), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
