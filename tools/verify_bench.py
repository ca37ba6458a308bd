"""dvp_verify_batch_dev throughput and dvp_verify latency (csrc/verify.hip).

    python tools/verify_bench.py [--reps 5] [--pool 4096] [--max-log 20] [--rlc] [--simulate]

Valid proofs (n_public = 2) are built once without a prover (tests/verify_cases.py, library encodings and transcript), a pool of
--pool distinct proofs tiled to each batch size -- every lane does the full work of a valid proof whatever repeats.  Batches of
1, 2^10, 2^16 and 2^20 proofs are timed with device events around dvp_verify_batch_dev on a torch stream after one warm-up call
per size; the single-proof host entry dvp_verify is timed with the host clock (it ends in a copy back).  Every verdict of every
timed batch is checked to be 0.  Kernel counts and times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script (tools/README.md).

--rlc: the same batches also through dvp_verify_batch_rlc_dev (one random-linear-combination MSM, the per-lane kernel gated off), timed
the same way right after the per-lane leg of each size, every report checked to be COMBINED; then a 2^16 batch (or the largest
size run) with one invalid proof, which takes the combined check plus the per-lane fallback, for both entries.

--simulate: the proofs come from dvp_simulate_batch (srs.simulate_batch) instead: 2^max-log DISTINCT proofs, every batch a prefix of
them, nothing tiled: the combined check's MSM then runs over 2^21 distinct points (tools/README.md, "Simulated proofs", has it
beside the tiled pool)."""
import argparse
import ctypes as C
import importlib
import json
import os
import random
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
import numpy as np  # noqa: E402
import torch  # noqa: E402

dvp = importlib.import_module("dv-pari_amd")
import pyref as o  # noqa: E402
import verify_cases as vc  # noqa: E402

# GF(2^233) products per proof, counted from verify.hip: two decodes (inversion 10 + 3 + the two subgroup tests 2 = 15 each), the
# branchless complete mixed addition madd_complete = 9 (8 of the mixed addition + 1 of the doubling candidate), the final
# cross-multiplication 2.  v0 K adds for every 1-digit of the tau-adic expansion of v0 (~120 of 240 digits); u0 G takes 15 table
# additions.  The lanes of a wave follow different digits, so the wave issues an addition wherever any lane has a 1: ~240.
GF_PER_PROOF_LANE = 2 * 15 + 9 * (120 + 15) + 2
GF_PER_PROOF_ISSUED = 2 * 15 + 9 * (240 + 15) + 2


def pool(n):
    rng = random.Random(1)
    td = (rng.randrange(1, o.P), rng.randrange(1, o.P), rng.randrange(1, o.P))
    pubs = [[rng.randrange(o.P), rng.randrange(o.P)] for _ in range(n)]

    def enc(dlogs):
        s = np.frombuffer(b"".join(int(k % o.P).to_bytes(32, "little") for k in dlogs), dtype="<u8").reshape(-1, 4).copy()
        out = np.zeros((len(dlogs), 30), dtype=np.uint8)
        dvp.check(dvp.lib.dvp_mulgen_batch(dvp._native.ptr(s), len(dlogs), dvp._native.ptr(out)), "dvp_mulgen_batch")
        return [out[i].tobytes() for i in range(len(dlogs))]

    built = vc.build(td, pubs, [None] * n, seed=2, encode_many=enc, challenge=dvp.proving.transcript_challenge)
    proofs = np.frombuffer(b"".join(c["proof"] for c in built), dtype=np.uint8).reshape(n, 118)
    return td, dvp.srs._public_array(pubs, n), proofs


def simulated(n):
    """n DISTINCT valid proofs (n_public = 2) from dvp_simulate_batch: the trapdoor of pool(), public inputs below 2^230"""
    rng = random.Random(1)
    td = (rng.randrange(1, o.P), rng.randrange(1, o.P), rng.randrange(1, o.P))
    pub = np.random.default_rng(2).integers(0, 1 << 62, size=(n, 2, 4), dtype=np.uint64)
    pub[:, :, 3] &= np.uint64((1 << 38) - 1)
    proofs, status = dvp.srs.simulate_batch(dvp.srs.Trapdoor(*td), pub)
    assert not status.any()
    return td, pub, proofs


def timed(a, s, tv, trep, fn, args, n, want_report, label, lg, bad_at=None):
    """one warm-up call, then --reps calls between device events on stream s; every verdict checked (0, or EQUATION at bad_at only)
    and, for the combined check, the report word"""
    dvp.check(fn(*args), "warm-up")
    s.synchronize()
    times = []
    for _ in range(a.reps):
        tv.fill_(0xEE)
        if trep is not None:
            trep.fill_(0x7777)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        dvp.check(fn(*args), label)
        e1.record(s)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
        if bad_at is None:
            assert int(tv.max().item()) == 0, "a valid proof was rejected"
        else:
            v = tv.cpu().numpy()
            assert v[bad_at] == dvp.srs.VERIFY_EQUATION and int((v != 0).sum()) == 1, "wrong verdicts"
        if trep is not None:
            assert int(trep.item()) == want_report, (label, int(trep.item()))
    med = float(np.median(times))
    print(f"{label} 2^{lg:2d}: {med:9.3f} ms median of {a.reps} (min {min(times):.3f}, max {max(times):.3f}) = "
          f"{n / (med * 1e-3):,.0f} proofs/s", flush=True)
    return {"n": n, "ms_median": round(med, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "proofs_per_s": round(n / (med * 1e-3), 1), "gf_products_per_s_lane": round(n * GF_PER_PROOF_LANE / (med * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--rlc", action="store_true", help="time dvp_verify_batch_rlc_dev beside dvp_verify_batch_dev")
    ap.add_argument("--simulate", action="store_true", help="distinct proofs from dvp_simulate_batch instead of a tiled pool")
    a = ap.parse_args()
    if a.simulate:
        a.pool = 1 << min(20, a.max_log)  # every batch is a prefix of one run of distinct proofs
    td, pub, proofs = simulated(a.pool) if a.simulate else pool(a.pool)
    keep, (t, d, e) = dvp.srs._trapdoor_args(dvp.srs.Trapdoor(*td))
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    res = {"gf_products_per_proof_lane": GF_PER_PROOF_LANE, "gf_products_per_proof_issued": GF_PER_PROOF_ISSUED, "batch": {}}
    for lg in [0, 10, 16, 20]:
        if lg > a.max_log:
            continue
        n = 1 << lg
        reps = -(-n // a.pool)
        tp = torch.from_numpy(np.tile(proofs, (reps, 1))[:n].copy()).to(dev)
        tpub = torch.from_numpy(np.tile(pub, (reps, 1, 1))[:n].view(np.int64).copy()).to(dev)
        tv = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        args = (t, d, e, C.c_void_p(tpub.data_ptr()), pub.shape[1], C.c_void_p(tp.data_ptr()), n, C.c_void_p(tv.data_ptr()),
                C.c_void_p(s.cuda_stream))
        res["batch"][f"2^{lg}"] = timed(a, s, tv, None, dvp.lib.dvp_verify_batch_dev, args, n, 0, "verify_batch_dev", lg)
        if a.rlc:
            trep = torch.zeros(1, dtype=torch.int32, device=dev)
            args_rlc = args[:7] + (None, args[7], C.c_void_p(trep.data_ptr()), args[8])
            res.setdefault("rlc", {})[f"2^{lg}"] = timed(a, s, tv, trep, dvp.lib.dvp_verify_batch_rlc_dev, args_rlc, n,
                                                         dvp.srs.VERIFY_RLC_COMBINED, "verify_batch_rlc_dev", lg)
    if a.rlc:  # one invalid proof (a0 + 1): the combined check fails and the per-lane kernel runs over the batch
        lg = min(16, a.max_log)
        n = 1 << lg
        reps = -(-n // a.pool)
        bad = np.tile(proofs, (reps, 1))[:n].copy()
        i_bad = n * 5 // 8
        a0 = int.from_bytes(bad[i_bad, 60:89].tobytes(), "little")
        bad[i_bad, 60:89] = np.frombuffer(((a0 + 1) % o.P).to_bytes(29, "little"), dtype=np.uint8)
        tp = torch.from_numpy(bad).to(dev)
        tpub = torch.from_numpy(np.tile(pub, (reps, 1, 1))[:n].view(np.int64).copy()).to(dev)
        tv = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        trep = torch.zeros(1, dtype=torch.int32, device=dev)
        args = (t, d, e, C.c_void_p(tpub.data_ptr()), pub.shape[1], C.c_void_p(tp.data_ptr()), n, C.c_void_p(tv.data_ptr()),
                C.c_void_p(s.cuda_stream))
        args_rlc = args[:7] + (None, args[7], C.c_void_p(trep.data_ptr()), args[8])
        res["one_invalid"] = {"n": n, "index": i_bad,
                              "batch": timed(a, s, tv, None, dvp.lib.dvp_verify_batch_dev, args, n, None, "verify_batch_dev, 1 bad", lg,
                                             bad_at=i_bad),
                              "rlc": timed(a, s, tv, trep, dvp.lib.dvp_verify_batch_rlc_dev, args_rlc, n, dvp.srs.VERIFY_RLC_FALLBACK,
                                           "verify_batch_rlc_dev, 1 bad", lg, bad_at=i_bad)}
    # single proof through the host entry (copies in, one launch, copy back)
    tdo = dvp.srs.Trapdoor(*td)
    p0, pub0 = proofs[0].tobytes(), dvp.fr.to_ints(pub[0])
    assert dvp.srs.verify_device(tdo, pub0, p0)
    lat = []
    for _ in range(max(20, a.reps)):
        t0 = time.perf_counter()
        ok = dvp.srs.verify_device(tdo, pub0, p0)
        lat.append((time.perf_counter() - t0) * 1e3)
        assert ok
    res["dvp_verify_ms_median"] = round(float(np.median(lat)), 4)
    res["dvp_verify_ms_min"] = round(min(lat), 4)
    print(f"dvp_verify (one proof, host entry): {np.median(lat):.3f} ms median of {len(lat)} (min {min(lat):.3f})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
