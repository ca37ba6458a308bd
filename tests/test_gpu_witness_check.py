"""GPU tests (-m gpu) of the witness check (csrc/prove_check.cuh: dvp_prover_check_witness*, dvp_prover_row_terms, the cache-dir flavour
and dvp_prove_cli --check-witness) against the plain-Python restatement of tests/witness_check_cases.py, on synthetic_dense(8) (m = 256,
one workgroup) and synthetic_sparse(12) (3581 real rows padded to 4096, 1-8 terms per side).  tests/test_witness_check_cases_cpu.py
holds the restatement itself and what every case is meant to do."""
import ctypes as C
import os

import numpy as np
import pytest

import msm_cases as mc
import witness_cases as wc
import witness_check_cases as wcc

pytestmark = pytest.mark.gpu
P = wcc.P
EINVAL, EUNSAT = -1, -3
K_REDUCE, K_REDUCE_BE, K_ROWS = "prove.hip:k_wc_reduce<false>", "prove.hip:k_wc_reduce<true>", "prove.hip:k_wc_rows"
K_SECOND = ("prove.hip:k_wc_scan", "prove.hip:k_wc_list_rows", "prove.hip:k_wc_terms", "prove.hip:k_wc_flag_wires", "prove.hip:k_wc_list_wires")
COUNTS = ("n_unsat", "first_unsat", "n_noncanonical", "first_noncanonical", "n_suspect_wires", "constant_wire_is_one")


def census(dvp):
    return {k: mc.launches(dvp, k) for k in (K_REDUCE, K_REDUCE_BE, K_ROWS) + K_SECOND}


def assert_report(rep, exp, max_rows, max_wires):
    assert {k: getattr(rep, k) for k in COUNTS} == {k: exp[k] for k in COUNTS}
    assert rep.rows == exp["rows"][:max_rows]
    assert rep.wires == exp["wires"][:max_wires]


@pytest.fixture(scope="module")
def provers(dvp):
    """case name -> a prover over the case's instance, WITHOUT SRS (cases that share an instance share the prover)"""
    by_inst, made = {}, {}
    for c in wcc.CASES:
        if id(c.inst) not in by_inst:
            by_inst[id(c.inst)] = dvp.proving.Prover(c.inst)
        made[c.name] = by_inst[id(c.inst)]
    yield made
    for pv in by_inst.values():
        pv.close()


@pytest.fixture(scope="module")
def with_srs(dvp):
    """instance name -> a prover that can prove: the two unedited instances with an SRS"""
    made = {}
    for k, name in enumerate(("dense8-ok", "sparse12-ok")):
        inst = wcc.BY_NAME[name].inst
        pv = dvp.proving.Prover(inst)
        pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, dvp.srs.Trapdoor(3 + k, 5 + k, 7 + k)))
        made[name.split("-")[0]] = pv
    yield made
    for pv in made.values():
        pv.close()


def split(case):
    k = case.n_public
    return case.w_raw[1:1 + k], case.w_raw[1 + k:]


# ---- 1. a satisfying witness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense8-ok", "sparse12-ok"])
def test_satisfying_witness_pays_the_row_pass_only(dvp, with_srs, name):
    import torch

    case = wcc.BY_NAME[name]
    pv = with_srs[name.split("-")[0]]
    pub, prv = split(case)
    before = pv.prove(pub, prv)
    dvp.lib.dvp_profile_reset()
    rep = pv.check_witness(pub, prv)
    assert_report(rep, wcc.expected(case), 16, 16)
    assert rep.ok and rep.rows == [] and rep.wires == [] and (rep.first_unsat, rep.first_noncanonical) == (-1, -1)
    got = census(dvp)
    assert got[K_REDUCE] == 1 and got[K_ROWS] == 1 and got[K_REDUCE_BE] == 0 and all(got[k] == 0 for k in K_SECOND), got
    # the device flavour, on the caller's stream, leaves the caller's buffer alone
    d_w = torch.from_numpy(dvp._native.ints_to_limbs(case.w_raw).view(np.int64)).cuda()
    keep = d_w.clone()
    rep_dev = pv.check_witness_dev(d_w.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert rep_dev == rep and torch.equal(d_w, keep)
    assert pv.prove(pub, prv).to_bytes() == before.to_bytes()


# ---- 2. one private wire changed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse12-one-wire", "dense8-one-wire"])
def test_one_changed_wire_is_explained(dvp, with_srs, provers, name):
    case = wcc.BY_NAME[name]
    exp = wcc.expected(case)
    pub, prv = split(case)
    full_rows, full_wires = exp["n_unsat"] + 3, exp["n_suspect_wires"] + 3
    dvp.lib.dvp_profile_reset()
    rep = provers[name].check_witness(pub, prv, max_rows=full_rows, max_wires=full_wires)  # a prover without SRS
    assert_report(rep, exp, full_rows, full_wires)
    assert len(rep.rows) == exp["n_unsat"] > 0 and all(r["a"] * r["b"] % P != (r["c"] + r["i"]) % P for r in rep.rows)
    got = census(dvp)
    assert got[K_ROWS] == 1 and got["prove.hip:k_wc_terms"] == 1 and got["prove.hip:k_wc_list_rows"] == 1, got
    # the index dvp_prove reports, and the prover that proves is none the worse for a check in between
    pv = with_srs[name.split("-")[0]]
    good_pub, good_prv = split(wcc.BY_NAME[name.split("-")[0] + "-ok"])
    before = pv.prove(good_pub, good_prv)
    with pytest.raises(dvp.DvpError) as e:
        pv.prove(pub, prv)
    assert (e.value.status, e.value.index) == (EUNSAT, rep.first_unsat)
    assert pv.check_witness(pub, prv, max_rows=full_rows, max_wires=full_wires) == rep
    assert pv.prove(good_pub, good_prv).to_bytes() == before.to_bytes()


# ---- 3. targeted rows ---------------------------------------------------------------------------------------------------------------
def test_rows_at_lane_wave_and_workgroup_edges(provers):
    case = wcc.BY_NAME["sparse12-edge-rows"]
    exp = wcc.expected(case)
    rep = provers[case.name].check_witness(*split(case), max_rows=64, max_wires=64)
    assert [r["row"] for r in rep.rows] == [0, 63, 64, 255, 256, case.inst.n_rows - 1] == case.want_rows
    assert_report(rep, exp, 64, 64)


# ---- 4. dense failure, truncated lists, counts only, twice the same bytes ---------------------------------------------------------------
def raw_check(dvp, pv, case, rows_cap, wires_cap):
    """the C entry itself, on arrays filled with a pattern and one record longer than the caps: (status, report, rows bytes, wires bytes)"""
    nat = dvp._native
    pub, prv = (nat.ints_to_limbs(v) for v in split(case))
    rows, wires, rep = (nat.UnsatRow * (rows_cap + 1))(), (nat.SuspectWire * (wires_cap + 1))(), nat.WitnessReport()
    C.memset(rows, 0xAB, C.sizeof(rows))
    C.memset(wires, 0xAB, C.sizeof(wires))
    rc = dvp.lib.dvp_prover_check_witness(pv._h, nat.ptr(pub), pub.shape[0], nat.ptr(prv), prv.shape[0], rows if rows_cap else None, rows_cap,
                                          wires if wires_cap else None, wires_cap, C.byref(rep))
    return rc, rep, bytes(rows), bytes(wires)


def test_dense_failure_truncates_in_order_and_repeats_exactly(dvp, provers):
    case = wcc.BY_NAME["sparse12-dense-failure"]
    exp = wcc.expected(case)
    pv = provers[case.name]
    lo, hi = wcc.DENSE_RANGE
    assert exp["n_unsat"] == hi - lo >= 512
    rep = pv.check_witness(*split(case), max_rows=5, max_wires=5)
    assert [r["row"] for r in rep.rows] == list(range(lo, lo + 5))
    assert_report(rep, exp, 5, 5)
    full = pv.check_witness(*split(case), max_rows=hi - lo + 1, max_wires=exp["n_suspect_wires"] + 1)
    assert_report(full, exp, hi - lo + 1, exp["n_suspect_wires"] + 1)
    # counts only
    rc, r0, _, _ = raw_check(dvp, pv, case, 0, 0)
    assert rc == 0 and (r0.n_unsat, r0.first_unsat, r0.n_suspect_wires, r0.n_rows_listed, r0.n_wires_listed) == (hi - lo, lo, exp["n_suspect_wires"], 0, 0)
    # twice: identical bytes, report included, and nothing written behind the listed records
    runs = [raw_check(dvp, pv, case, 5, 3) for _ in range(2)]
    assert runs[0][0] == runs[1][0] == 0
    assert bytes(runs[0][1]) == bytes(runs[1][1]) and runs[0][2:] == runs[1][2:]
    rep5, rows_b, wires_b = runs[0][1:]
    assert (rep5.n_rows_listed, rep5.n_wires_listed) == (5, min(3, exp["n_suspect_wires"]))
    assert rows_b[5 * 136:] == b"\xab" * 136 and wires_b[8 * rep5.n_wires_listed:] == b"\xab" * (8 * (4 - rep5.n_wires_listed))


# ---- 5. entries that are not below p ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense8-p-and-p3", "sparse12-lifted"])
def test_entries_not_below_p_are_counted_and_reduced(provers, name):
    case = wcc.BY_NAME[name]
    exp = wcc.expected(case)
    assert exp["n_noncanonical"] >= 2
    rep = provers[name].check_witness(*split(case), max_rows=300, max_wires=300)
    assert_report(rep, exp, 300, 300)
    assert rep.constant_wire_is_one


def test_zeroed_constant_wire_is_reported(dvp, provers):
    import torch

    case = wcc.BY_NAME["dense8-zero-constant"]
    exp = wcc.expected(case)
    assert case.w_raw[0] == 0 and not exp["constant_wire_is_one"]
    pv = provers[case.name]
    rep = pv.check_witness_be32(wc.be32(case.w_raw), max_rows=300, max_wires=300)
    assert_report(rep, exp, 300, 300)
    d_w = torch.from_numpy(dvp._native.ints_to_limbs(case.w_raw).view(np.int64)).cuda()
    assert pv.check_witness_dev(d_w.data_ptr(), max_rows=300, max_wires=300) == rep
    # the limb flavour writes the constant wire itself, as dvp_prove does
    assert pv.check_witness(*split(case)).ok


# ---- 6. the flavours agree; the cache-dir flavour needs no SRS file ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def cache_no_srs(dvp, tmp_path_factory):
    """a directory with the dump of synthetic_sparse(12) and the one-wire witness UNREDUCED in its file: no SRS file at all"""
    A = dvp.artifacts
    case = wcc.BY_NAME["sparse12-one-wire"]
    path = tmp_path_factory.mktemp("witness_check") / "cache"
    path.mkdir()
    case.inst.write_dump_file(path / A.R1CS_CONSTRAINTS_FILE)
    lifted = list(case.w_raw)
    lifted[0] += 2 * P
    lifted[9] += P
    (path / A.R1CS_WITNESS_FILE).write_bytes(wc.witness_file_bytes(lifted))
    assert sorted(os.listdir(path)) == sorted([A.R1CS_CONSTRAINTS_FILE, A.R1CS_WITNESS_FILE])
    yield path, case, lifted
    dvp.proving.release_cache_dir()


def test_flavours_agree(dvp, provers, cache_no_srs, tmp_path):
    path, case, lifted = cache_no_srs
    exp = wcc.expected(case)
    pv = provers[case.name]
    canon = pv.check_witness(*split(case), max_rows=40, max_wires=40)
    assert_report(canon, exp, 40, 40)
    dvp.lib.dvp_profile_reset()
    assert pv.check_witness_be32(wc.be32(case.w_raw + [2**256 - 1, 5]), max_rows=40, max_wires=40) == canon  # a longer buffer is truncated
    assert mc.launches(dvp, K_REDUCE_BE) == 1 and mc.launches(dvp, K_REDUCE) == 0
    # the file holds other representatives of entries 0 and 9: the same rows, two entries counted
    want = wcc.restate(*wcc.rows_of(case.inst), case.n_public, case.inst.num_constraints, lifted, wcc.domain(case.log_m))
    assert (want["n_noncanonical"], want["first_noncanonical"]) == (2, 0) and want["rows"] == exp["rows"] and want["wires"] == exp["wires"]
    from_file = dvp.proving.check_witness_file(path, case.n_public, max_rows=40, max_wires=40)
    assert_report(from_file, want, 40, 40)
    assert pv.check_witness_be32(wc.be32(lifted), max_rows=40, max_wires=40) == from_file
    # an explicit path; a file shorter than the circuit's wires
    other = tmp_path / "elsewhere"
    other.write_bytes(wc.witness_file_bytes(case.w_raw))
    assert dvp.proving.check_witness_file(path, case.n_public, other, max_rows=40, max_wires=40) == canon
    other.write_bytes(wc.witness_file_bytes(case.w_raw[:-1]))
    with pytest.raises(dvp.DvpError) as e:
        dvp.proving.check_witness_file(path, case.n_public, other)
    assert e.value.status == EINVAL


# ---- 7. row terms, and every DVP_EINVAL before any launch ---------------------------------------------------------------------------------
def test_row_terms_and_einval(dvp, provers):
    nat = dvp._native
    case = wcc.BY_NAME["sparse12-ok"]
    pv = provers[case.name]
    rows, _ = wcc.rows_of(case.inst)
    for r in (0, 1, 255, 256, 2000, case.inst.n_rows - 1):
        for which in range(3):
            assert pv.row_terms(which, r) == rows[r][which]
    for r in (case.inst.n_rows, 4095):
        assert [pv.row_terms(which, r) for which in range(3)] == [[], [], []]
    # cap < n: the first cap terms, and n all the same
    r = max(range(64), key=lambda k: len(rows[k][0]))
    assert len(rows[r][0]) >= 2
    w2, c2, n = np.full(3, 0xABABABAB, dtype=np.uint32), np.full(3, 0xABABABAB, dtype=np.uint32), C.c_size_t(0)
    assert dvp.lib.dvp_prover_row_terms(pv._h, 0, r, nat.ptr(w2), nat.ptr(c2), 1, C.byref(n)) == 0
    assert n.value == len(rows[r][0]) and (int(w2[0]), int(c2[0])) == rows[r][0][0] and int(w2[1]) == int(c2[1]) == 0xABABABAB

    dvp.lib.dvp_profile_reset()
    lib, h = dvp.lib, pv._h
    assert lib.dvp_prover_row_terms(h, 0, 4096, None, None, 0, C.byref(n)) == EINVAL  # row = m
    assert lib.dvp_prover_row_terms(h, 3, 0, None, None, 0, C.byref(n)) == EINVAL
    assert lib.dvp_prover_row_terms(h, -1, 0, None, None, 0, C.byref(n)) == EINVAL
    assert lib.dvp_prover_row_terms(h, 0, 0, None, None, 0, None) == EINVAL
    assert lib.dvp_prover_row_terms(h, 0, 0, None, None, 4, C.byref(n)) == EINVAL
    pub, prv = (nat.ints_to_limbs(v) for v in split(case))
    rows_a, wires_a, rep = (nat.UnsatRow * 2)(), (nat.SuspectWire * 2)(), nat.WitnessReport()
    good = [h, nat.ptr(pub), pub.shape[0], nat.ptr(prv), prv.shape[0], rows_a, 2, wires_a, 2, C.byref(rep)]

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return lib.dvp_prover_check_witness(*a)

    assert call(a9=None) == EINVAL                       # no report
    assert call(a5=None) == EINVAL and call(a7=None) == EINVAL  # a NULL array with a non-zero cap
    assert call(a0=None) == EINVAL
    assert call(a2=pub.shape[0] - 1) == EINVAL and call(a2=pub.shape[0] + 1) == EINVAL  # dvp_prove's count rules
    assert call(a4=prv.shape[0] - 1) == EINVAL and call(a4=prv.shape[0] + 1) == EINVAL
    assert call(a3=None) == EINVAL and call(a1=None) == EINVAL
    raw = np.frombuffer(wc.be32(case.w_raw), dtype=np.uint8)
    assert lib.dvp_prover_check_witness_be32(h, nat.ptr(raw), len(case.w_raw) - 1, rows_a, 2, wires_a, 2, C.byref(rep)) == EINVAL
    assert lib.dvp_prover_check_witness_be32(h, None, len(case.w_raw), rows_a, 2, wires_a, 2, C.byref(rep)) == EINVAL
    assert lib.dvp_prover_check_witness_be32(h, nat.ptr(raw), len(case.w_raw), None, 2, wires_a, 2, C.byref(rep)) == EINVAL
    assert lib.dvp_prover_check_witness_dev(h, None, rows_a, 2, wires_a, 2, C.byref(rep), None) == EINVAL
    assert lib.dvp_prover_check_witness_dev(h, 256, rows_a, 2, wires_a, 2, None, None) == EINVAL
    assert lib.dvp_check_witness_cache_dir_witness_file(b"/nonexistent", 2, None, rows_a, 2, wires_a, 2, None) == EINVAL
    assert lib.dvp_check_witness_cache_dir_witness_file(b"/nonexistent", 2, None, None, 2, wires_a, 2, C.byref(rep)) == EINVAL
    # a prover that has no matrices yet
    bare = C.c_void_p()
    dvp.check(lib.dvp_prover_create(3, 2, 8, C.byref(bare)), "dvp_prover_create")
    try:
        one = nat.ints_to_limbs([1] * 7)
        assert lib.dvp_prover_check_witness(bare, nat.ptr(one), 2, nat.ptr(one[2:]), 5, rows_a, 2, wires_a, 2, C.byref(rep)) == EINVAL
        assert lib.dvp_prover_row_terms(bare, 0, 0, None, None, 0, C.byref(n)) == EINVAL
    finally:
        lib.dvp_prover_destroy(bare)
    assert all(v == 0 for v in census(dvp).values())
    # and the good call is good
    assert call() == 0 and rep.n_unsat == 0


# ---- 8. the compiled host ---------------------------------------------------------------------------------------------------------------
def test_cli_check_witness(dvp, cache_no_srs, tmp_path):
    import shutil
    import subprocess

    path, case, lifted = cache_no_srs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "no g++: the compiled host cannot be built"
    exe = tmp_path / "dvp_prove_cli"
    libdir = os.path.join(root, "dv-pari_amd")
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "dvp_prove_cli.cpp"),
                           "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-pthread", "-o", str(exe)])
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")
    want = wcc.restate(*wcc.rows_of(case.inst), case.n_public, case.inst.num_constraints, lifted, wcc.domain(case.log_m))
    out = subprocess.run([str(exe), str(path), str(case.n_public), "--check-witness", "--max-rows", "4"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr)
    lines = out.stdout.splitlines()
    head = dict(kv.split("=") for kv in lines[0].split()[1:])
    assert lines[0].startswith("witness: ") and {k: int(v) for k, v in head.items()} == {k: int(want[k]) for k in COUNTS}
    row_lines = [ln.split() for ln in lines[1:] if ln.startswith("row ")]
    got_rows = [dict(row=int(f[1]), **{kv.split("=")[0]: int(kv.split("=")[1], 16) for kv in f[2:]}) for f in row_lines]
    assert got_rows == want["rows"][:4]
    wire_lines = [ln.split() for ln in lines[1:] if ln.startswith("wire ")]
    assert [(int(f[1]), int(f[2].split("=")[1])) for f in wire_lines] == want["wires"][:4]
    assert len(lines) == 1 + len(row_lines) + len(wire_lines)
    # a satisfying, canonical witness: exit status 0 and the counts alone
    good = wcc.BY_NAME["sparse12-ok"]
    (path / dvp.artifacts.R1CS_WITNESS_FILE).write_bytes(wc.witness_file_bytes(good.w_raw))
    try:
        out = subprocess.run([str(exe), str(path), str(case.n_public), "--check-witness"], capture_output=True, text=True, env=env, timeout=120)
    finally:
        (path / dvp.artifacts.R1CS_WITNESS_FILE).write_bytes(wc.witness_file_bytes(lifted))
    assert out.returncode == 0 and out.stdout.splitlines() == [
        "witness: n_unsat=0 first_unsat=-1 n_noncanonical=0 first_noncanonical=-1 n_suspect_wires=0 constant_wire_is_one=1"], (out.returncode, out.stdout, out.stderr)
