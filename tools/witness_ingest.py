#!/usr/bin/env python3
"""What the way from gnark's witness bytes to the proof costs: python tools/witness_ingest.py [log_m ...]   (default 16 20 22)

For each size an SP1-like sparse instance (gnark_r1cs.synthetic_sparse_fast: n_wires = 7/8 x 2^log_m) is set up into a cache_dir with
its witness file, in a process of its own under its own time limit, and these are timed -- one warm-up each, then five rounds with the
variants in turn, median and min .. max:

  a  load_witness_from_file + Prover.prove     wall    dvp_file_witness_read (reduction on one host thread) + dvp_prove: the old path
  g  Prover.prove                              wall    dvp_prove from canonical limbs in (pageable) host memory
  b  Prover.prove_be32                         wall    dvp_prove_be32 from the raw bytes in (pageable) host memory
  c  Proof.prove_witness_file                  wall    dvp_prove_cache_dir_witness_file: maps the file (page cache warm) and proves
  d  Prover.prove_dev                          wall    dvp_prove_dev on a witness resident in HBM
  e  fr.from_be32_dev                          events  k_fr_from_be32 alone, n_wires elements (in place, and out of place)
  f  device-to-device copy of 32 n_wires bytes events  moves what the kernel moves: its floor

g - d is what dvp_prove pays for bringing 32 bytes per element over the link from pageable memory; b - d is the same for the new
entry, which adds one pass of the kernel over the witness.  The last line of a size is its JSON record."""
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {16: 180, 20: 420, 22: 900}  # seconds per size (setup included)
ROUNDS = 5


def unreduced_be32(w, rng):
    """canonical limbs uint64 [n, 4] -> uint8 [n, 32]: w + k p big-endian with a random k < 2^22 per element, values of ~254 bits as
    a BN254 witness holds them (the old host reducer's conditional subtractions depend on the value; the kernel does not)"""
    import numpy as np

    n = w.shape[0]
    p = 3450873173395281893717377931138512760570940988862252126328087024741343
    p32 = np.array([(p >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint64)
    k = rng.integers(0, 1 << 22, size=n, dtype=np.uint64)
    acc = np.ascontiguousarray(w).view(np.uint32).reshape(n, 8).astype(np.uint64) + k[:, None] * p32  # < 2^55 per limb
    carry = np.zeros(n, dtype=np.uint64)
    for i in range(8):
        acc[:, i] += carry
        carry = acc[:, i] >> np.uint64(32)
        acc[:, i] &= np.uint64(0xFFFFFFFF)
    assert not carry.any()
    return np.ascontiguousarray(acc.astype(np.uint32).view(np.uint8).reshape(n, 32)[:, ::-1])


def measure(log_m: int):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    dvp = importlib.import_module("dv-pari_amd")
    A, g = dvp.artifacts, dvp.gnark_r1cs
    t0 = time.time()
    inst0, pub, prv = g.synthetic_sparse_fast(log_m)
    w = np.concatenate([dvp.fr.vec([1]), pub, prv])
    n = w.shape[0]
    with tempfile.TemporaryDirectory(prefix="dvp_ingest_") as cache:
        inst0.write_dump_file(os.path.join(cache, A.R1CS_CONSTRAINTS_FILE))
        wfile = os.path.join(cache, A.R1CS_WITNESS_FILE)
        raw = unreduced_be32(w, np.random.default_rng(log_m))
        with open(wfile, "wb") as f:
            f.write(n.to_bytes(4, "big"))
            f.write(raw.tobytes())
        td = dvp.srs.Trapdoor(0x1234567 + (1 << 200), 0x7654321 + (1 << 190), 0xABCDEF + (1 << 180))
        _, pv = dvp.srs.verifier_runs_setup_cache_dir(td, cache, pub.shape[0], write_precomputes=False)
        assert np.array_equal(g.read_witness_raw(wfile), raw) and np.array_equal(g.load_witness_from_file(wfile), w)
        print(f"2^{log_m}: setup {time.time() - t0:.1f} s, n_wires {n}, witness {32 * n / 1e6:.1f} MB", flush=True)
        d_w = torch.from_numpy(w.view(np.int64)).cuda()
        d_raw = torch.from_numpy(raw).cuda()
        d_buf, d_out, d_cp = torch.empty_like(d_raw), torch.empty_like(d_raw), torch.empty_like(d_raw)
        st = torch.cuda.current_stream().cuda_stream
        proofs = {}

        def wall(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t) * 1e3, out

        def events(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), None

        def old_path():
            v = g.load_witness_from_file(wfile)
            return pv.prove(v[1:1 + pub.shape[0]], v[1 + pub.shape[0]:n])

        def kernel_in_place():
            dvp.fr.from_be32_dev(d_buf.data_ptr(), n, None, st)

        variants = [
            ("a", wall, old_path),
            ("g", wall, lambda: pv.prove(pub, prv)),
            ("b", wall, lambda: pv.prove_be32(raw)),
            ("c", wall, lambda: dvp.proving.Proof.prove_witness_file(cache, pub.shape[0])[0]),
            ("d", wall, lambda: pv.prove_dev(d_w.data_ptr(), st)),
            ("e_in_place", events, kernel_in_place),
            ("e_out_of_place", events, lambda: dvp.fr.from_be32_dev(d_raw.data_ptr(), n, d_out.data_ptr(), st)),
            ("f", events, lambda: d_cp.copy_(d_raw)),
        ]
        times = {name: [] for name, _, _ in variants}
        for rnd in range(ROUNDS + 1):  # round 0 is the warm-up (tables, workspaces, the cache_dir entry, the page cache)
            for name, how, fn in variants:
                if name == "e_in_place":
                    d_buf.copy_(d_raw)
                ms, out = how(fn)
                if rnd:
                    times[name].append(ms)
                if out is not None:
                    proofs.setdefault(name, out.to_bytes())
                    assert proofs[name] == out.to_bytes()
        assert len(set(proofs.values())) == 1 and dvp.srs.verify(td, dvp.fr.to_ints(pub), dvp.proving.Proof.from_bytes(proofs["b"]))
        assert torch.equal(d_out.cpu(), torch.from_numpy(w.view(np.uint8).reshape(n, 32)))  # the kernel's output is the witness
        dvp.proving.release_cache_dir()
        pv.close()
    rec = {"log_m": log_m, "n_wires": int(n), "rounds": ROUNDS,
           "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}}
    med = {k: statistics.median(v) for k, v in times.items()}
    rec["g_minus_d_ms"] = round(med["g"] - med["d"], 4)
    rec["b_minus_d_ms"] = round(med["b"] - med["d"], 4)
    rec["kernel_GBps"] = round(64 * n / med["e_in_place"] / 1e6, 1)  # 32 bytes read + 32 written per element
    rec["copy_GBps"] = round(64 * n / med["f"] / 1e6, 1)
    for k, v in rec["ms"].items():
        print(f"  {k:15s} {v['median']:10.3f} ms   ({v['min']:.3f} .. {v['max']:.3f})")
    print(f"  g - d {rec['g_minus_d_ms']:.3f} ms, b - d {rec['b_minus_d_ms']:.3f} ms; kernel {rec['kernel_GBps']} GB/s, copy {rec['copy_GBps']} GB/s")
    print(json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
        return 0
    sizes = [int(a) for a in sys.argv[1:]] or [16, 20, 22]
    worst = 0
    for log_m in sizes:  # a fresh process per size: this one never opens the GPU
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(log_m)], timeout=LIMITS.get(log_m, 900))
            rc = r.returncode
        except subprocess.TimeoutExpired:
            print(f"2^{log_m}: time limit of {LIMITS.get(log_m, 900)} s reached", flush=True)
            rc = 124
        if rc:
            print(f"2^{log_m}: exit {rc}; not starting the larger sizes", flush=True)
            return rc
        worst = worst or rc
    return worst


if __name__ == "__main__":
    sys.exit(main())
