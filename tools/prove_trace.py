#!/usr/bin/env python3
"""What the trace of a proof costs: python tools/prove_trace.py [log_m] [--rounds N]   (default 20, 5 rounds)

On the synthetic dense circuit of bench.py (2^log_m constraints) one prover is set up and these are timed, wall clock around each call
(every one of them waits for its result), one warm-up each and then N rounds with the variants in turn, median and min .. max:

  prove     Prover.prove_dev                   one proof, witness resident in HBM (dvp_prove_dev)
  scalars   trace_last(TRACE_SCALARS)          one 320-byte copy
  digests   trace_last(TRACE_DIGESTS)          sixteen dvp_fr_vec_digest_dev over 17 m + n_wires entries
  points    trace_last(TRACE_POINTS)           five one-shot MSMs, two sums, five encodings
  all       trace_last(TRACE_ALL)

and, by device events, the digest of one 2m-entry vector (k_scalar_r's length) against dvp_blake3_dev over a buffer of the stream's byte
length: the packer's share of the digest.  The proof before and after the traces is compared byte for byte; mismatch must be 0.  The last
line is the JSON record."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAPDOOR = (0x1234567 + (1 << 200), 0x7654321 + (1 << 190), 0xABCDEF + (1 << 180))


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    log_m = int(args[0]) if args else 20
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    dvp = importlib.import_module("dv-pari_amd")
    P = dvp.proving
    t0 = time.time()
    inst, pub, prv = dvp.gnark_r1cs.synthetic_dense(log_m)
    pv = P.Prover(inst)
    pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, dvp.srs.Trapdoor(*TRAPDOOR)))
    assignment = torch.from_numpy(dvp.fr.vec([1] + pub + prv).view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    m = 1 << log_m
    print(f"2^{log_m}: setup {time.time() - t0:.1f} s, n_wires {inst.n_wires}", flush=True)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    variants = {
        "prove": lambda: pv.prove_dev(assignment.data_ptr(), stream),
        "scalars": lambda: pv.trace_last(P.TRACE_SCALARS, stream),
        "digests": lambda: pv.trace_last(P.TRACE_DIGESTS, stream),
        "points": lambda: pv.trace_last(P.TRACE_POINTS, stream),
        "all": lambda: pv.trace_last(P.TRACE_ALL, stream),
    }
    first = {k: wall(fn)[1] for k, fn in variants.items()}  # warm-up; the proof comes first, so every trace has one to describe
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms, out = wall(fn)
            times[k].append(ms)
            assert out == first[k], f"{k}: not the same result as in the warm-up round"
    rec_all = first["all"]
    assert rec_all["mismatch"] == 0 and rec_all["commit_p"]["enc"] == first["prove"].commit_p and rec_all["kzg_k"]["enc"] == first["prove"].kzg_k

    # the digest of one 2m-entry vector against the plain hash of as many bytes, by device events
    n = 2 * m
    nbytes = 8 + 29 * n
    vec = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda")
    vec[:, 3] &= (1 << 39) - 1  # below 2^231 < p
    flat = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(32, dtype=torch.uint8, device="cuda")

    def events(fn):
        ts = []
        for r in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r:
                ts.append(e0.elapsed_time(e1))
        return ts

    lib = dvp.lib
    t_dig = events(lambda: dvp.check(lib.dvp_fr_vec_digest_dev(vec.data_ptr(), n, 0, out.data_ptr(), stream), "dvp_fr_vec_digest_dev"))
    t_mont = events(lambda: dvp.check(lib.dvp_fr_vec_digest_dev(vec.data_ptr(), n, 1, out.data_ptr(), stream), "dvp_fr_vec_digest_dev"))
    t_b3 = events(lambda: dvp.check(lib.dvp_blake3_dev(flat.data_ptr(), nbytes, out.data_ptr(), stream), "dvp_blake3_dev"))

    def stat(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}

    rec = {"log_m": log_m, "n_wires": inst.n_wires, "rounds": rounds, **{k: stat(v) for k, v in times.items()},
           "digest_2m": {**stat(t_dig), "stream_bytes": nbytes, "GBps": round(nbytes / statistics.median(t_dig) / 1e6, 2)},
           "digest_2m_montgomery": {**stat(t_mont), "GBps": round(nbytes / statistics.median(t_mont) / 1e6, 2)},
           "blake3_dev_same_bytes": {**stat(t_b3), "GBps": round(nbytes / statistics.median(t_b3) / 1e6, 2)},
           "hashed_bytes_per_trace": 16 * 8 + 29 * (17 * m + inst.n_wires)}
    for k in variants:
        s = rec[k]
        print(f"  {k:8s} {s['median_ms']:9.3f} ms  ({s['min_ms']:.3f} .. {s['max_ms']:.3f})")
    for k in ("digest_2m", "digest_2m_montgomery", "blake3_dev_same_bytes"):
        s = rec[k]
        print(f"  {k:22s} {s['median_ms']:9.3f} ms  {s['GBps']:8.2f} GB/s")
    pv.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
