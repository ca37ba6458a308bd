#!/usr/bin/env python3
"""dvp_prover_check_witness_dev (csrc/prove_check.cuh): what the witness check costs, on synthetic_dense(20) and on the SP1-like sparse
instance at 2^22 (gnark_r1cs.synthetic_sparse_fast), the assignment resident in HBM:
  ok        the check on the satisfying witness: k_wc_reduce + k_wc_rows and one wait (the per-term pass does not run)
  one-wire  the check on the witness with one private wire changed: the listing (16 rows, 16 wires) and the per-term pass behind the
            host's look at the count, two waits
  begin     Prover.begin(need_extend=False) of the same prover on the satisfying witness: the witness copy, k_r1cs_eval and the flag read
            -- the row pass a proof pays, measured in the same run, the three alternating
Host clock around calls that end in a stream wait; 3 warm-up rounds, then the median and the minimum of --reps rounds.  begin asks for an
SRS although it reads none with need_extend=False: the prover is given zero-filled vectors, so no setup runs.  The one-wire report is
compared with the index begin reports for the same witness.
    python tools/witness_check.py [--configs dense20,sparse22] [--reps 21] [--out FILE.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

dvp = importlib.import_module("dv-pari_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="dense20,sparse22")
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--out", default=None)
args = ap.parse_args()
g, lib = dvp.gnark_r1cs, dvp.lib
st = torch.cuda.current_stream().cuda_stream
res = []


def limbs(v):
    return v if isinstance(v, np.ndarray) else dvp.fr.vec(v)


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


for cfg in args.configs.split(","):
    kind, lg = cfg[:-2], int(cfg[-2:])
    inst, pub, prv = g.synthetic_dense(lg) if kind == "dense" else g.synthetic_sparse_fast(lg)
    m, nw = inst.num_constraints, inst.n_wires
    w = np.zeros((nw, 4), dtype=np.uint64)
    w[0, 0] = 1
    w[1:1 + len(pub)] = limbs(pub)
    w[1 + len(pub):] = limbs(prv)
    bad = w.copy()
    k_bad = nw // 2  # a private wire in the middle
    bad[k_bad, 0] ^= np.uint64(1)
    pv = dvp.proving.Prover(inst)
    zeros = torch.zeros(max(nw, 2 * m) * 8, dtype=torch.int64, device="cuda")  # begin never reads a base
    for which, n in enumerate((nw, m, m, m, 2 * m)):
        dvp.check(lib.dvp_prover_set_srs_affine_dev(pv._h, which, zeros.data_ptr(), None, n), "dvp_prover_set_srs_affine_dev")
    del zeros
    d_ok, d_bad = torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(bad.view(np.int64)).cuda()
    torch.cuda.synchronize()
    rep_bad = pv.check_witness_dev(d_bad.data_ptr(), stream=st)
    try:
        pv.begin(d_bad.data_ptr(), st, need_extend=False)
        idx = None
    except dvp.DvpError as e:
        idx = e.index
    assert rep_bad.n_unsat > 0 and rep_bad.first_unsat == idx, (rep_bad.first_unsat, idx)
    assert pv.check_witness_dev(d_ok.data_ptr(), stream=st).ok
    legs = {"ok": lambda: pv.check_witness_dev(d_ok.data_ptr(), stream=st), "one-wire": lambda: pv.check_witness_dev(d_bad.data_ptr(), stream=st),
            "begin": lambda: pv.begin(d_ok.data_ptr(), st, need_extend=False)}
    t = {k: [] for k in legs}
    for r in range(3 + args.reps):
        for k, f in legs.items():
            ms = timed(f)
            if r >= 3:
                t[k].append(ms)
    row = dict(config=cfg, constraints=m, rows=inst.n_rows, wires=nw, terms=sum(int(mt.row_ptr[inst.n_rows]) for mt in (inst.l, inst.r, inst.o)),
               n_unsat=rep_bad.n_unsat, first_unsat=rep_bad.first_unsat, n_suspect_wires=rep_bad.n_suspect_wires, changed_wire=k_bad,
               changed_wire_listed=any(wi == k_bad for wi, _ in rep_bad.wires), reps=args.reps,
               **{f"{k}_ms_median": statistics.median(v) for k, v in t.items()}, **{f"{k}_ms_min": min(v) for k, v in t.items()})
    res.append(row)
    print(f"{cfg}: m = {m}, {nw} wires, {row['terms']} terms; check ok {row['ok_ms_median']:.3f} ms (min {row['ok_ms_min']:.3f}), one wire changed "
          f"{row['one-wire_ms_median']:.3f} ms (min {row['one-wire_ms_min']:.3f}; {rep_bad.n_unsat} rows fail, first {rep_bad.first_unsat}, "
          f"{rep_bad.n_suspect_wires} suspect wires), begin(need_extend=False) {row['begin_ms_median']:.3f} ms (min {row['begin_ms_min']:.3f}); "
          f"ok / begin = {row['ok_ms_median'] / row['begin_ms_median']:.2f}", flush=True)
    pv.close()
    del d_ok, d_bad
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
