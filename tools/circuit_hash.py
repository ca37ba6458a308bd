#!/usr/bin/env python3
"""dvp_prover_circuit_hash (csrc/circuit_hash.hip): time of the hash on the SP1-like sparse instance (gnark_r1cs.synthetic_sparse_fast)
at 2^16, 2^20 and 2^22 constraints -- host clock around the call, which finds p - 1, generates the stream window by window, hashes
it and waits -- with the stream's byte count and the GB/s that amounts to, and beside it dvp_blake3_dev over a plain device buffer
of the same length (HIP events around back-to-back calls): what the hashing alone costs, so the difference is the generator kernels,
the allocations and the two waits.  At the smallest size the digest is compared with BLAKE3 of a stream built on the host from
pyref.r1cs_with_vandermonde (D read back from the prover).
    python tools/circuit_hash.py [--log2 16,20,22] [--out FILE.json]"""
import argparse
import importlib
import json
import os
import struct
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
import numpy as np
import torch

dvp = importlib.import_module("dv-pari_amd")
import pyref as o

ap = argparse.ArgumentParser()
ap.add_argument("--log2", default="16,20,22")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = dvp.lib
res = []


def ints(limbs):
    return [int.from_bytes(limbs[i].tobytes(), "little") for i in range(limbs.shape[0])]


def host_stream(inst, dom):
    rows = []
    for i in range(inst.n_rows):
        rows.append(tuple([(int(mt.wire[t]), int(mt.coeff[t])) for t in range(int(mt.row_ptr[i]), int(mt.row_ptr[i + 1]))] for mt in (inst.l, inst.r, inst.o)))
    rows2, coeffs2, _ = o.r1cs_with_vandermonde(rows, ints(inst.coeffs), dom, inst.num_public_inputs)
    row_part = b"".join(struct.pack("<I", cid) for row in rows2 for side in row for _, cid in side)
    return row_part + struct.pack("<Q", len(coeffs2)) + b"".join(int(c).to_bytes(29, "little") for c in coeffs2)


out32 = torch.zeros(32, dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream
sizes = [int(x) for x in args.log2.split(",")]
for lg in sizes:
    inst, _, _ = dvp.gnark_r1cs.synthetic_sparse_fast(lg)
    pv = dvp.proving.Prover(inst)
    m, k = inst.num_constraints, inst.num_public_inputs
    n0 = inst.coeffs.shape[0]
    n1 = n0 if (o.P - 1) in ints(inst.coeffs) else n0 + 1
    N = n1 + m * max(k - 1, 0)
    nnz = sum(int(mt.row_ptr[inst.n_rows]) for mt in (inst.l, inst.r, inst.o))
    nbytes = 4 * (nnz + k * m) + 8 + 29 * N
    times = []
    for _ in range(5):
        t = time.perf_counter()
        digest = pv.circuit_hash()
        times.append(time.perf_counter() - t)
    checked = False
    if lg == min(sizes) and lg <= 16:
        s = host_stream(inst, ints(pv.domains()[0]))
        assert len(s) == nbytes and dvp.proving.blake3(s) == digest
        checked = True
    pv.close()
    buf = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=torch.Generator().manual_seed(lg)).cuda()
    for _ in range(3):
        dvp.check(lib.dvp_blake3_dev(buf.data_ptr(), nbytes, out32.data_ptr(), st), "dvp_blake3_dev")
    torch.cuda.synchronize()
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dvp.check(lib.dvp_blake3_dev(buf.data_ptr(), nbytes, out32.data_ptr(), st), "dvp_blake3_dev")
    e1.record()
    torch.cuda.synchronize()
    plain_ms = e0.elapsed_time(e1) / reps
    warm = min(times[1:])
    row = dict(log2_constraints=lg, rows=inst.n_rows, terms=nnz, table_entries=N, stream_bytes=nbytes, first_ms=times[0] * 1e3, warm_ms=warm * 1e3,
               warm_GBps=nbytes / warm / 1e9, plain_hash_ms=plain_ms, plain_hash_GBps=nbytes / plain_ms / 1e6, digest=digest.hex(), checked_against_host=checked)
    res.append(row)
    print(f"2^{lg} constraints: stream {nbytes / 1e6:.1f} MB ({nnz} terms, {N} table entries); circuit hash first {times[0] * 1e3:.2f} ms, warm "
          f"{warm * 1e3:.2f} ms = {row['warm_GBps']:.1f} GB/s; dvp_blake3_dev over {nbytes} plain bytes {plain_ms:.3f} ms = {row['plain_hash_GBps']:.1f} GB/s"
          + ("; digest equals the host-built stream's" if checked else ""), flush=True)
    del buf
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
