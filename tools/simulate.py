#!/usr/bin/env python3
"""dvp_simulate_batch_dev and dvp_verify_trace_batch_dev (csrc/simulate.hip) against their yardsticks, in one run.

    python tools/simulate.py [--json out.json] [--max-log 20] [--pool 4096]

For n = 1, 2^10, 2^16 and 2^20 proofs with two public inputs each, device events on a torch stream, one warm-up call and then the
median of 5:
  simulate      dvp_simulate_batch_dev, generic proofs, discrete logs not asked for
  mulgen 2n     k_mulgen alone on 2n scalars (dvp_ubench_points_mul's second figure): the two fixed-base multiplications a simulated
                proof contains, and so its floor
  trace         dvp_verify_trace_batch_dev on the simulated proofs
  verify        dvp_verify_batch_dev on the same proofs: the trace does the same work plus three normalisations and 488 B of output
At the largest size dvp_verify_batch_rlc_dev is timed on the distinct simulated proofs and on the first --pool of them tiled to the
same count, which is how tools/verify_bench.py fills its batches by default.  Every timed batch is checked: status 0, verdict 0,
report COMBINED, and the trace's verdicts equal the verifier's."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
REPS = 5
N_PUBLIC = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--pool", type=int, default=4096)
    a = ap.parse_args()
    import numpy as np
    import torch

    dvp = importlib.import_module("dv-pari_amd")
    lib, check, S = dvp.lib, dvp.check, dvp.srs
    rng = np.random.default_rng(5)
    td = S.Trapdoor(*(int.from_bytes(rng.bytes(28), "little") + 1 for _ in range(3)))
    keep, (t, d, e) = S._trapdoor_args(td)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    stream = C.c_void_p(st.cuda_stream)

    def timed(fn, *args):
        check(fn(*args), "warm-up")
        st.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            check(fn(*args))
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    rows = []
    logs = [lg for lg in (0, 10, 16, 20) if lg <= a.max_log]
    for lg in logs:
        n = 1 << lg
        pub = rng.integers(0, 1 << 62, size=(n, N_PUBLIC, 4), dtype=np.uint64)
        pub[:, :, 3] &= np.uint64((1 << 38) - 1)  # below 2^230
        tpub = torch.from_numpy(pub.view(np.int64)).to(dev)
        tp = torch.empty((n, 118), dtype=torch.uint8, device=dev)
        ts = torch.empty(n, dtype=torch.uint8, device=dev)
        tv = torch.empty(n, dtype=torch.uint8, device=dev)
        tt = torch.empty((n, S.VERIFY_TRACE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        row = dict(log_n=lg)
        torch.cuda.synchronize()  # the copies above ran on the default stream
        row["simulate_ms"] = timed(lib.dvp_simulate_batch_dev, t, d, e, vp(tpub), N_PUBLIC, n, None, 0, None, None, vp(tp), vp(ts), None, stream)
        assert int(ts.max().item()) == 0
        row["trace_ms"] = timed(lib.dvp_verify_trace_batch_dev, t, d, e, vp(tpub), N_PUBLIC, vp(tp), n, vp(tt), stream)
        row["verify_ms"] = timed(lib.dvp_verify_batch_dev, t, d, e, vp(tpub), N_PUBLIC, vp(tp), n, vp(tv), stream)
        assert int(tv.max().item()) == 0 and int(tt[:, 485].max().item()) == 0  # byte 485 of a record is its verdict
        # the floor: k_mulgen on 2n scalars (the entry times dvp_points_mul_dev beside it; its points are the table's own products)
        m = 2 * n
        sc = rng.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 38) - 1)
        t_sc = torch.from_numpy(sc.view(np.int64)).to(dev)
        t_xy = torch.empty((m, 64), dtype=torch.uint8, device=dev)
        t_scratch = torch.empty(m * 65, dtype=torch.uint8, device=dev)
        xy, inf = dvp.curve.point_scalar_mul_gen_batch(sc[: min(m, 1 << 12)])
        assert not inf.any()
        t_xy.view(-1)[:] = torch.from_numpy(np.resize(xy.view(np.uint8).reshape(-1), m * 64)).to(dev)
        torch.cuda.synchronize()
        mul_ms, gen_ms = C.c_double(0), C.c_double(0)
        check(lib.dvp_ubench_points_mul(vp(t_sc), vp(t_xy), m, vp(t_scratch), REPS, C.byref(mul_ms), C.byref(gen_ms)), "dvp_ubench_points_mul")
        row["mulgen_2n_ms"] = gen_ms.value
        row["simulate_over_floor"] = row["simulate_ms"] / row["mulgen_2n_ms"]
        row["trace_over_verify"] = row["trace_ms"] / row["verify_ms"]
        if lg == logs[-1]:
            trep = torch.zeros(1, dtype=torch.int32, device=dev)
            row["rlc_distinct_ms"] = timed(lib.dvp_verify_batch_rlc_dev, t, d, e, vp(tpub), N_PUBLIC, vp(tp), n, None, vp(tv), vp(trep), stream)
            assert int(tv.max().item()) == 0 and int(trep.item()) == S.VERIFY_RLC_COMBINED
            k = min(a.pool, n)
            idx = torch.arange(n, device=dev) % k
            tp2, tpub2 = tp[idx].contiguous(), tpub[idx].contiguous()
            torch.cuda.synchronize()
            row["rlc_tiled_ms"] = timed(lib.dvp_verify_batch_rlc_dev, t, d, e, vp(tpub2), N_PUBLIC, vp(tp2), n, None, vp(tv), vp(trep), stream)
            assert int(tv.max().item()) == 0 and int(trep.item()) == S.VERIFY_RLC_COMBINED
            row["rlc_distinct_over_tiled"] = row["rlc_distinct_ms"] / row["rlc_tiled_ms"]
        rows.append(row)
        print(f"2^{lg:2d}: simulate {row['simulate_ms']:9.3f} ms  mulgen 2n {row['mulgen_2n_ms']:9.3f} ms ({row['simulate_over_floor']:.2f} x)  "
              f"trace {row['trace_ms']:9.3f} ms  verify {row['verify_ms']:9.3f} ms ({row['trace_over_verify']:.2f} x)"
              + (f"  rlc distinct {row['rlc_distinct_ms']:.3f} ms, tiled {row['rlc_tiled_ms']:.3f} ms ({row['rlc_distinct_over_tiled']:.2f} x)"
                 if "rlc_tiled_ms" in row else ""), flush=True)
    out = dict(rows=rows, n_public=N_PUBLIC, reps=REPS, pool=a.pool, device=torch.cuda.get_device_name(0))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
