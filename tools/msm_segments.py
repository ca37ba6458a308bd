#!/usr/bin/env python3
"""dvp_msm_segments_dev against the only other way to the same results, a loop of dvp_msm_affine_dev over the segments, and against
dvp_points_mul_dev alone on the same n (stage 1: the difference is the segmented reduction's share).

    python tools/msm_segments.py [--json out.json] [--logs 16,20] [--timeout 600]

For totals of 2^16 and 2^20 points cut into equal segments of 16, 256, 4096 and 65536 points, and one skewed cut (one segment
holding half the points, the rest in segments of 8), device events around
    (a) dvp_msm_segments_dev            (b) dvp_msm_affine_dev once per segment            (c) dvp_points_mul_dev on all n
one warm-up each, then the median of 5, the variants taken in turn WITHIN a shape so that they share whatever else the box is
doing.  (b) runs at most 64 calls per repetition -- the first segments of the cut, the long one of the skewed cut among them -- and
is scaled to the whole cut where there are more (marked ~): the calls are independent and of one size.  Seeded inputs (points
k_i G, scalars uniform below r).  Before anything is timed, the first and the last segment of every cut are compared with the C
oracle's reference-shaped MSM, and every segment (b) computes with (a)'s: a faster wrong kernel is not measured.

Every total runs in a process of its own under its own time limit; the first one that fails ends the script."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
REPS = 5
B_CALLS = 64
SEG_LENS = (16, 256, 4096, 65536)


def cuts(n):
    """[(name, seg_ptr)] for a total of n points"""
    import numpy as np

    out = []
    for m in SEG_LENS:
        if m <= n:
            out.append((f"{n // m} x {m}", np.arange(0, n + 1, m, dtype=np.uint64)))
    half = n // 2
    out.append((f"1 x {half} + {half // 8} x 8", np.concatenate([[0], np.arange(half, n + 1, 8)]).astype(np.uint64)))
    return out


def median_ms(fn, torch):
    fn()  # warm-up
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[REPS // 2]


def run_total(log_n):
    import numpy as np
    import torch

    import c_oracle as co
    from util import np_to_pt, rand_fr_np

    dvp = importlib.import_module("dv-pari_amd")
    lib, check = dvp.lib, dvp.check
    n = 1 << log_n
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(rand_fr_np(n, 5))
    assert not inf.any()
    ks = rand_fr_np(n, 6)
    t_xy = torch.from_numpy(xy.view(np.int64)).cuda()
    t_s = torch.from_numpy(ks.view(np.int64)).cuda()
    t_prod = torch.empty(n * 65, dtype=torch.uint8, device="cuda")
    t_sum = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    threads = co.host_threads(16)
    rows = []
    for name, sp in cuts(n):
        n_seg = len(sp) - 1
        wb = dvp.curve.segments_work_bytes(n, n_seg)
        t_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        t_out = torch.zeros((n_seg, 8), dtype=torch.int64, device="cuda")
        t_oinf = torch.zeros(n_seg, dtype=torch.uint8, device="cuda")
        calls = min(n_seg, B_CALLS)
        b_out = torch.zeros((calls, 8), dtype=torch.int64, device="cuda")
        b_inf = torch.zeros(calls, dtype=torch.int32, device="cuda")
        bounds = [(int(sp[j]), int(sp[j + 1])) for j in range(calls)]

        def run_a():
            dvp.curve.multi_scalar_mul_segments_dev(t_s.data_ptr(), t_xy.data_ptr(), 0, n, sp, t_out.data_ptr(), t_oinf.data_ptr(), t_work.data_ptr(),
                                                    wb, t_sum.data_ptr(), st)

        def run_b():
            for j, (lo, hi) in enumerate(bounds):
                check(lib.dvp_msm_affine_dev(t_s.data_ptr() + 32 * lo, t_xy.data_ptr() + 64 * lo, None, hi - lo, b_out.data_ptr() + 64 * j,
                                             b_inf.data_ptr() + 4 * j, st), "dvp_msm_affine_dev")

        def run_c():
            dvp.curve.point_scalar_mul_dev(t_s.data_ptr(), n, t_xy.data_ptr(), 0, n, t_prod.data_ptr(), t_prod.data_ptr() + 64 * n, t_sum.data_ptr(), st)

        # ---- results first ----
        run_a()
        run_b()
        torch.cuda.synchronize()
        got = t_out.cpu().numpy().view(np.uint64)
        got_inf = t_oinf.cpu().numpy()
        assert not got_inf.any(), name
        for j in (0, n_seg - 1):
            lo, hi = int(sp[j]), int(sp[j + 1])
            assert np_to_pt(got[j]) == co.msm(ks[lo:hi], xy[lo:hi], threads=threads), (name, j)
        assert not b_inf.cpu().numpy().any() and b_out.cpu().numpy().tobytes() == t_out[:calls].cpu().numpy().tobytes(), name
        # ---- then the clock: the three variants in turn ----
        a_ms = median_ms(run_a, torch)
        skew = n_seg > 1 and bounds[0][1] - bounds[0][0] != bounds[1][1] - bounds[1][0]
        timed = list(bounds)
        long_ms = 0.0
        if skew:  # the long segment on its own, counted once; the short ones after it stand for the rest
            bounds[:] = timed[:1]
            long_ms = median_ms(run_b, torch)
            bounds[:] = timed[1:]
        b_ms = median_ms(run_b, torch)
        b_ms = long_ms + b_ms / len(bounds) * (n_seg - (1 if skew else 0))
        bounds[:] = timed
        c_ms = median_ms(run_c, torch)
        row = dict(log_n=log_n, cut=name, n_seg=n_seg, a_ms=a_ms, b_ms=b_ms, b_scaled=calls < n_seg, c_ms=c_ms, stage2_ms=a_ms - c_ms)
        rows.append(row)
        print(f"2^{log_n:2d}  {name:>24s}:  (a) segments {a_ms:9.3f} ms   (b) loop of one-shot MSMs {'~' if row['b_scaled'] else ' '}{b_ms:11.3f} ms"
              f"   (c) products alone {c_ms:9.3f} ms   stage 2 = (a) - (c) {a_ms - c_ms:8.3f} ms   (b) / (a) {b_ms / a_ms:8.2f}", flush=True)
        del t_work
    v = C.c_longlong(0)
    check(lib.dvp_tune_get(b"DVP_MSM_SEG_PIECE", C.byref(v)))
    return dict(rows=rows, piece=v.value, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--timeout", type=int, default=600, help="seconds one total may take")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)  # the child: one total, its rows to --json
    a = ap.parse_args()
    if a.one is not None:
        with open(a.json, "w") as f:
            json.dump(run_total(a.one), f)
        return 0
    rows, meta = [], {}
    for log_n in (int(x) for x in a.logs.split(",")):
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "rows.json")
            try:  # the child prints its lines itself, as they come
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(log_n), "--json", part], timeout=a.timeout).returncode
            except subprocess.TimeoutExpired:
                print(f"2^{log_n}: no result within {a.timeout} s: stopping", flush=True)
                return 1
            if rc != 0:
                print(f"2^{log_n}: exit status {rc}: stopping", flush=True)
                return 1
            with open(part) as f:
                res = json.load(f)
        rows += res.pop("rows")
        meta = res
    print(f"DVP_MSM_SEG_PIECE in this build: {meta.get('piece')}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows, **meta), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
