#!/usr/bin/env python3
"""dvp_blake3_dev (csrc/blake3_tree.hip) and dvp_prover_srs_hash: GB/s of the device hash at 2^20, 2^26 and 2^30 bytes (warm, HIP
events around `reps` back-to-back calls on one stream) with the share of the achievable HBM rate that amounts to, the SRS hash of a
2^20-constraint prover (encode + hash through the staging window, host clock around the call, which waits for its result), and beside
both the host dvp_blake3 over the same bytes on one core.  Every device digest is compared with the host's.
    python tools/blake3_tree.py [--max-log2 30] [--srs-log2 20] [--out FILE.json]"""
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
import numpy as np
import torch

dvp = importlib.import_module("dv-pari_amd")
from util import rand_fr_np

HBM_ACHIEVABLE = 6.3e12  # bytes/s a streaming read reaches on this chip; the hash reads every byte once

ap = argparse.ArgumentParser()
ap.add_argument("--max-log2", type=int, default=30)
ap.add_argument("--srs-log2", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib, ptr = dvp.lib, dvp._native.ptr
res = {"hash": [], "srs": None}


def host_hash(a: np.ndarray):
    out = np.zeros(32, dtype=np.uint8)
    t = time.perf_counter()
    dvp.check(lib.dvp_blake3(ptr(a), a.size, ptr(out)), "dvp_blake3")
    return out.tobytes(), time.perf_counter() - t


out = torch.zeros(32, dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream
for lg in (20, 26, 30):
    if lg > args.max_log2:
        continue
    n = 1 << lg
    host = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(lg))
    buf = host.cuda()
    for _ in range(3):  # warm: code objects, the stream's memory pool
        dvp.check(lib.dvp_blake3_dev(buf.data_ptr(), n, out.data_ptr(), st), "dvp_blake3_dev")
    torch.cuda.synchronize()
    reps = max(3, min(200, (1 << 33) >> lg))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dvp.check(lib.dvp_blake3_dev(buf.data_ptr(), n, out.data_ptr(), st), "dvp_blake3_dev")
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    want, host_s = host_hash(host.numpy())
    assert out.cpu().numpy().tobytes() == want, lg
    row = dict(bytes=n, reps=reps, dev_ms=ms, dev_GBps=n / ms / 1e6, hbm_fraction=n / (ms * 1e-3) / HBM_ACHIEVABLE, host_ms=host_s * 1e3,
               host_GBps=n / host_s / 1e9)
    res["hash"].append(row)
    print(f"2^{lg} bytes: device {ms:.3f} ms = {row['dev_GBps']:.1f} GB/s ({100 * row['hbm_fraction']:.1f} % of 6.3 TB/s); "
          f"host, one core {host_s * 1e3:.1f} ms = {row['host_GBps']:.3f} GB/s", flush=True)
    del buf, host

# the SRS hash of a prover with 2^srs_log2 constraints and as many wires: random bases (the hash does not care what they are)
lg = args.srs_log2
m = 1 << lg
h = C.c_void_p()
dvp.check(lib.dvp_prover_create(lg, 2, m, C.byref(h)), "dvp_prover_create")
enc = {}
for which, cnt in enumerate((m, m, m, m, 2 * m)):
    xy, inf = dvp.curve.point_scalar_mul_gen_batch(rand_fr_np(cnt, 100 + which))
    dvp.check(lib.dvp_prover_set_srs_affine(h, which, ptr(np.ascontiguousarray(xy)), ptr(np.ascontiguousarray(inf)), cnt), "set_srs")
    enc[which] = dvp.curve.to_bytes(xy, inf)
digest = np.zeros(32, dtype=np.uint8)
times = []
for _ in range(4):
    t = time.perf_counter()
    dvp.check(lib.dvp_prover_srs_hash(h, ptr(digest)), "dvp_prover_srs_hash")
    times.append(time.perf_counter() - t)
stream = np.concatenate([np.ascontiguousarray(enc[w], dtype=np.uint8).reshape(-1) for w in (2, 3, 4, 1, 0)])  # g_k_0 g_k_1 g_k_2 g_q g_m
want, host_s = host_hash(stream)
assert digest.tobytes() == want
res["srs"] = dict(log2_constraints=lg, stream_bytes=int(stream.size), first_ms=times[0] * 1e3, warm_ms=min(times[1:]) * 1e3,
                  warm_GBps=stream.size / min(times[1:]) / 1e9, host_hash_ms=host_s * 1e3)
print(f"dvp_prover_srs_hash at 2^{lg} constraints ({stream.size / 1e6:.1f} MB of encodings): first call {times[0] * 1e3:.2f} ms, warm "
      f"{min(times[1:]) * 1e3:.2f} ms (encode + hash, allocations and the wait included); host BLAKE3 of the same bytes {host_s * 1e3:.0f} ms")
lib.dvp_prover_destroy(h)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
