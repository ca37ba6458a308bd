"""dvp_srs_check_cache_dir against the only other way to answer "is this directory the SRS of this trapdoor?", running the setup
again (dvp_setup_cache_dir_ex), on the SP1-like sparse instance of tools/setup_time.py:

    python tools/srs_check.py [log_m ...]          (default 16 20; writes into a temporary directory, removed afterwards)

Four rows per size, each the median of 5 calls behind one warm-up call, timed by device events on the null stream around the whole
call (file reads and the host's waits included), with the fastest and the slowest of the five:
    combined      the check of the directory the setup wrote: five combined MSMs
    one wrong     the same with one entry of g_k_2 replaced: the combined check of every vector, then the located comparison of g_k_2
    exact         DVP_SRS_CHECK_EXACT: every point recomputed and compared
    setup         dvp_setup_cache_dir_ex into a second directory (without the precompute files)"""
import importlib, os, shutil, sys, tempfile
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
dvp = importlib.import_module("dv-pari_amd")
nat = importlib.import_module("dv-pari_amd._native")
td = dvp.srs.Trapdoor(0x1234567 + (1 << 200), 0x7654321 + (1 << 190), 0xABCDEF + (1 << 180))
REPS = 5


def timed(fn):
    fn()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[REPS // 2], ms[0], ms[-1]


for log_m in [int(x) for x in sys.argv[1:]] or [16, 20]:
    inst, pub, prv = dvp.gnark_r1cs.synthetic_sparse_fast(log_m, max_terms=8)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    tmp, tmp2 = tempfile.mkdtemp(prefix="dvp_srs_check_", dir=base), tempfile.mkdtemp(prefix="dvp_srs_check2_", dir=base)
    try:
        for d in (tmp, tmp2):
            inst.write_dump_file(os.path.join(d, dvp.artifacts.R1CS_CONSTRAINTS_FILE))
        t, d_, e = (dvp.fr.limbs(x) for x in (td.tau, td.delta, td.epsilon))
        setup = lambda where: dvp.check(dvp.lib.dvp_setup_cache_dir_ex(nat.ptr(t), nat.ptr(d_), nat.ptr(e), os.fsencode(where), len(pub), 0, None, 0, None, None), "setup")
        setup(tmp)
        m = 1 << log_m
        print(f"2^{log_m}: wires {inst.n_wires}, {inst.n_wires + 5 * m} points in five vectors", flush=True)
        rows = []
        good = dvp.srs.check_cache_dir(td, tmp, len(pub))
        assert good.ok, good
        rows.append(("combined", timed(lambda: dvp.srs.check_cache_dir(td, tmp, len(pub)))))
        k2 = os.path.join(tmp, dvp.artifacts.SRS_G_K_2)
        enc = dvp.io_utils.read_point_vec_payload(k2)
        keep, at = enc.copy(), m + 12345 % m
        enc[at] = dvp.curve.point_scalar_mul_gen_batch_bytes(dvp.fr.vec([4242]))[0]
        dvp.io_utils.write_point_vec_to_file(k2, enc)
        bad = dvp.srs.check_cache_dir(td, tmp, len(pub))
        assert bad.bad_vectors == 1 << 4 and bad["g_k_2"].first_bad == at and bad["g_k_2"].path == dvp.curve.DLOG_PATH_LOCATED, bad
        rows.append(("one wrong", timed(lambda: dvp.srs.check_cache_dir(td, tmp, len(pub)))))
        dvp.io_utils.write_point_vec_to_file(k2, keep)
        assert dvp.srs.check_cache_dir(td, tmp, len(pub), exact=True).ok
        rows.append(("exact", timed(lambda: dvp.srs.check_cache_dir(td, tmp, len(pub), exact=True))))
        rows.append(("setup", timed(lambda: setup(tmp2))))
        for name, (med, lo, hi) in rows:
            print(f"  {name:<10} {med:9.1f} ms   ({lo:.1f} .. {hi:.1f})", flush=True)
        print(f"  setup / combined = {rows[3][1][0] / rows[0][1][0]:.1f}, exact / combined = {rows[2][1][0] / rows[0][1][0]:.1f}", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        shutil.rmtree(tmp2, ignore_errors=True)
