#!/usr/bin/env python3
"""The affine point check (dvp_points_check_dev, k_points_check) against its yardstick, k_decode, on the same count in the same run.

    python tools/points_check.py [--json out.json] [--no-setter]

* dvp_points_check_dev at 2^20 and 2^22 valid points: device events around the entry (two 8-byte fills and the kernel), median of 5
  after a warm-up call;
* k_points_check and k_decode alone on the same counts (dvp_ubench_points_check: device events around each kernel, median of 5
  after a warm-up launch).  k_decode does strictly more per point (an inversion, two subgroup tests, four more products), so a check
  that is not faster than it means the three products are not sharing their table;
* what strict mode adds to dvp_prover_set_srs_affine for a vector of 2^20 points (host clock around the call, which copies the
  vector and waits either way; median of 5 with strict off, then on)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
REPS = 5


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-setter", action="store_true", help="skip the dvp_prover_set_srs_affine comparison (it builds a 2^20-constraint prover)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from util import rand_fr_np

    dvp = importlib.import_module("dv-pari_amd")
    lib, check = dvp.lib, dvp.check
    n0 = 1 << 20
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(rand_fr_np(n0, 5))
    enc = dvp.curve.to_bytes(xy, inf)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for log_n in (20, 22):
        n = 1 << log_n
        rep = n // n0
        t_xy = torch.from_numpy(xy.view(np.int64)).cuda().repeat(rep, 1)
        t_inf = torch.from_numpy(inf).cuda().repeat(rep)
        t_enc = torch.from_numpy(enc).cuda().repeat(rep, 1)
        t_scratch = torch.empty(n * 65, dtype=torch.uint8, device="cuda")
        t_sum = torch.empty(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ms = []
        for r in range(-1, REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib.dvp_points_check_dev(t_xy.data_ptr(), t_inf.data_ptr(), n, None, t_sum.data_ptr(), st), "dvp_points_check_dev")
            e1.record()
            e1.synchronize()
            if r >= 0:
                ms.append(e0.elapsed_time(e1))
        first, n_bad = (int(v) for v in t_sum.cpu().numpy().view(np.uint64))
        assert (first, n_bad) == ((1 << 64) - 1, 0), (first, n_bad)
        k_check, k_decode = C.c_double(0), C.c_double(0)
        check(lib.dvp_ubench_points_check(t_xy.data_ptr(), t_inf.data_ptr(), t_enc.data_ptr(), n, t_scratch.data_ptr(), REPS, C.byref(k_check),
                                          C.byref(k_decode)), "dvp_ubench_points_check")
        row = dict(log_n=log_n, check_dev_ms=median(ms), check_dev_min=min(ms), check_dev_max=max(ms), k_points_check_ms=k_check.value,
                   k_decode_ms=k_decode.value)
        rows.append(row)
        print(f"2^{log_n} points: dvp_points_check_dev {row['check_dev_ms']:.3f} ms (min {row['check_dev_min']:.3f}, max {row['check_dev_max']:.3f})"
              f"  k_points_check {k_check.value:.3f} ms  k_decode {k_decode.value:.3f} ms  check / decode {k_check.value / k_decode.value:.2f}", flush=True)
        if k_check.value >= k_decode.value:
            print("  the check is NOT faster than the decode: see tools/kernel_resources.sh for k_points_check's resource report", flush=True)
        del t_xy, t_inf, t_enc, t_scratch
    out = dict(points=rows)
    if not a.no_setter:
        inst, _, _ = dvp.gnark_r1cs.synthetic_dense(20)
        pv = dvp.proving.Prover(inst)
        prev = dvp.curve.strict_points()
        try:
            t = {}
            for on in (False, True):
                dvp.curve.set_strict_points(on)
                v = []
                for r in range(-1, REPS):
                    t0 = time.perf_counter()
                    check(lib.dvp_prover_set_srs_affine(pv._h, 1, dvp._native.ptr(xy), dvp._native.ptr(inf), n0), "dvp_prover_set_srs_affine")
                    if r >= 0:
                        v.append((time.perf_counter() - t0) * 1e3)
                t[on] = median(v)
        finally:
            dvp.curve.set_strict_points(prev)
            pv.close()
        out["set_srs_affine_2^20"] = dict(strict_off_ms=t[False], strict_on_ms=t[True], added_ms=t[True] - t[False])
        print(f"dvp_prover_set_srs_affine, 2^20 points: {t[False]:.2f} ms strict off, {t[True]:.2f} ms strict on, added {t[True] - t[False]:.2f} ms", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
