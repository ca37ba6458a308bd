#!/usr/bin/env python3
"""What the way from a host buffer of arkworks-form Fr (four LE u64 of a 2^256 mod p per element, the memory of a Vec<Fr>) to the proof
costs: python tools/ark_ingest.py [log_m ...]   (default 16 20)

For each size an SP1-like sparse instance (gnark_r1cs.synthetic_sparse_fast: n_wires = 7/8 x 2^log_m) is set up in a process of its own
under its own time limit, and these are timed -- one warm-up each, then five rounds with the variants in turn, median and min .. max:

  a  fr.from_ark_host + Prover.prove           wall    dvp_debug_fr_ark_host (one Montgomery reduction per element on ONE host thread, into
                                                       fresh memory) + dvp_prove: what a host had to do before dvp_prove_ark existed
  b  Prover.prove_ark                          wall    dvp_prove_ark from the arkworks-form bytes in (pageable) host memory
  g  Prover.prove                              wall    dvp_prove from canonical limbs in (pageable) host memory: b without the kernel
  h  Prover.prove                              wall    the same from a copy of those limbs allocated the way the arkworks-form buffers
                                                       were (a result array of the library's wrapper): b - h is b - g on like memory
  b_again                                      wall    b once more, behind g and h instead of behind a's host conversion: its place in the turn
  k  fr.from_ark_dev                           events  k_fr_from_ark alone, n_wires elements (in place, and out of place)
  f  device-to-device copy of 32 n_wires bytes events  moves what the kernel moves (64 bytes per element): its floor

a / b is the gain; b - g should be about k (more would mean that a host wait crept in: tools/host_gap.py shows where), and the host
waits on the prover's stream are counted per proof for b and g (dvp_profile_read "host_waits_stream").  Every proof of a size must be
the same 118 bytes.  The last line of a size is its JSON record."""
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {16: 180, 20: 420, 22: 900}  # seconds per size (setup included)
ROUNDS = 5


def measure(log_m: int):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    dvp = importlib.import_module("dv-pari_amd")
    g = dvp.gnark_r1cs
    t0 = time.time()
    inst, pub, prv = g.synthetic_sparse_fast(log_m)
    n_pub, n = pub.shape[0], 1 + pub.shape[0] + prv.shape[0]
    td = dvp.srs.Trapdoor(0x1234567 + (1 << 200), 0x7654321 + (1 << 190), 0xABCDEF + (1 << 180))
    pv = dvp.proving.Prover(inst)
    pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, td))
    ark_pub, ark_prv = dvp.fr.to_ark(pub), dvp.fr.to_ark(prv)  # the host's Vec<Fr> memory
    pub_h, prv_h = dvp.fr.from_ark(ark_pub), dvp.fr.from_ark(ark_prv)
    assert np.array_equal(pub_h, pub) and np.array_equal(prv_h, prv) and np.array_equal(dvp.fr.from_ark_host(ark_prv[:4096]), prv[:4096])
    print(f"2^{log_m}: setup {time.time() - t0:.1f} s, n_wires {n}, witness {32 * n / 1e6:.1f} MB", flush=True)
    d_ark = torch.from_numpy(np.concatenate([ark_pub, ark_prv]).view(np.int64)).cuda()
    d_buf, d_out, d_cp = torch.empty_like(d_ark), torch.empty_like(d_ark), torch.empty_like(d_ark)
    st = torch.cuda.current_stream().cuda_stream
    proofs, waits = {}, {}

    def stream_waits():
        ms, cnt = C.c_double(0), C.c_uint64(0)
        dvp.check(dvp.lib.dvp_profile_read(b"host_waits_stream", C.byref(ms), C.byref(cnt)), "host_waits_stream")
        return int(cnt.value)

    def wall(fn):
        torch.cuda.synchronize()
        w0 = stream_waits()
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out, stream_waits() - w0

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), None, None

    def todays_way():
        return pv.prove(dvp.fr.from_ark_host(ark_pub), dvp.fr.from_ark_host(ark_prv))

    variants = [
        ("a", wall, todays_way),
        ("b", wall, lambda: pv.prove_ark(ark_pub, ark_prv)),
        ("g", wall, lambda: pv.prove(pub, prv)),
        ("h", wall, lambda: pv.prove(pub_h, prv_h)),
        ("b_again", wall, lambda: pv.prove_ark(ark_pub, ark_prv)),
        ("k_in_place", events, lambda: dvp.fr.from_ark_dev(d_buf.data_ptr(), n - 1, None, st)),
        ("k_out_of_place", events, lambda: dvp.fr.from_ark_dev(d_ark.data_ptr(), n - 1, d_out.data_ptr(), st)),
        ("f", events, lambda: d_cp.copy_(d_ark)),
    ]
    times = {name: [] for name, _, _ in variants}
    for rnd in range(ROUNDS + 1):  # round 0 is the warm-up (tables, workspaces)
        for name, how, fn in variants:
            if name == "k_in_place":
                d_buf.copy_(d_ark)
            ms, out, w = how(fn)
            if rnd:
                times[name].append(ms)
                if w is not None:
                    waits.setdefault(name, set()).add(w)
            if out is not None:
                proofs.setdefault(name, out.to_bytes())
                assert proofs[name] == out.to_bytes()
    assert len(set(proofs.values())) == 1 and dvp.srs.verify(td, dvp.fr.to_ints(pub), dvp.proving.Proof.from_bytes(proofs["b"]))
    assert d_out.cpu().numpy().tobytes() == np.concatenate([pub, prv]).tobytes()  # the kernel's output is the witness
    pv.close()
    rec = {"log_m": log_m, "n_wires": int(n), "rounds": ROUNDS,
           "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}}
    med = {k: statistics.median(v) for k, v in times.items()}
    rec["a_over_b"] = round(med["a"] / med["b"], 3)
    rec["a_minus_b_ms"] = round(med["a"] - med["b"], 4)
    rec["b_minus_g_ms"] = round(med["b"] - med["g"], 4)
    rec["b_minus_h_ms"] = round(med["b"] - med["h"], 4)
    rec["kernel_GBps"] = round(64 * (n - 1) / med["k_in_place"] / 1e6, 1)  # 32 bytes read + 32 written per element
    rec["copy_GBps"] = round(64 * (n - 1) / med["f"] / 1e6, 1)
    rec["host_waits_stream_per_proof"] = {k: sorted(v) for k, v in waits.items()}
    for k, v in rec["ms"].items():
        print(f"  {k:15s} {v['median']:10.3f} ms   ({v['min']:.3f} .. {v['max']:.3f})")
    print(f"  a / b {rec['a_over_b']:.2f}, a - b {rec['a_minus_b_ms']:.3f} ms, b - g {rec['b_minus_g_ms']:.3f} ms, b - h {rec['b_minus_h_ms']:.3f} ms; kernel {rec['kernel_GBps']} GB/s, "
          f"copy {rec['copy_GBps']} GB/s; stream waits per proof {rec['host_waits_stream_per_proof']}")
    print(json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
        return 0
    sizes = [int(a) for a in sys.argv[1:]] or [16, 20]
    for log_m in sizes:  # a fresh process per size: this one never opens the GPU
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(log_m)], timeout=LIMITS.get(log_m, 900)).returncode
        except subprocess.TimeoutExpired:
            print(f"2^{log_m}: time limit of {LIMITS.get(log_m, 900)} s reached", flush=True)
            rc = 124
        if rc:
            print(f"2^{log_m}: exit {rc}; not starting the larger sizes", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
