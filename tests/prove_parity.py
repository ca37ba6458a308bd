"""Proof::prove through the C ABI against the oracle, stage for stage: the comparison test_gpu_prove.py and test_gpu_prove_edges.py
share.  Needs a GPU (it drives the product); the expected values come from oracle/pyref.py and the C oracle alone."""
import pyref as o
import c_oracle as co
from util import from_limbs

STAGE_VECTORS = ("a", "b", "c", "i", "a2", "b2", "c2", "i2", "r2", "q2", "ka", "kb", "kr")
STAGE_SCALARS = ("alpha", "a0", "b0", "i0", "r0")


def rows_of(inst):
    rows = []
    for i in range(inst.n_rows):
        row = []
        for mt in (inst.l, inst.r, inst.o):
            a, b = int(mt.row_ptr[i]), int(mt.row_ptr[i + 1])
            row.append([(int(mt.wire[k]), int(mt.coeff[k])) for k in range(a, b)])
        rows.append(tuple(row))
    return rows


def check_against_oracle(dvp, inst, pub, prv, trap, golden=None, verifies=True, oracle=None):
    """verifies: the verdict the ORACLE gives its own proof (False only where the reference itself proves what its verifier rejects: more
    public inputs than rows); the library's verifier must give the same.  oracle: (tree, setup, proof scalars) when the caller has
    them already -- what the two pyref calls below return for (inst, pub, prv, trap)."""
    pv = dvp.proving.Prover(inst)
    td = dvp.srs.Trapdoor(*trap)
    # setup scalars vs the oracle's brute-force setup
    if oracle is None:
        tree = o.FFTree(pv.log_m + 1)
        st = o.setup_srs_scalars(tree, rows_of(inst), from_limbs(inst.coeffs), inst.num_public_inputs, trap)
    else:
        tree, st, _ = oracle
    g_m, g_q, g_k = dvp.srs.srs_scalars(pv, inst, td)
    assert from_limbs(g_m) == st["g_m"] + [0] * (inst.n_wires - len(st["g_m"]))
    assert from_limbs(g_q) == st["g_q"]
    for j in range(3):
        assert from_limbs(g_k[j]) == st["g_k"][j]
    assert from_limbs(pv.debug("bar_wts")) == st["tables"]["bar_wts"]
    assert from_limbs(pv.debug("z_vals2inv")) == st["tables"]["z_vals2inv"]
    d, d2 = pv.domains()
    assert (from_limbs(d), from_limbs(d2)) == tuple(tree.both_domains())
    srs = dvp.srs.verifier_runs_setup(pv, inst, td)
    pv.set_srs(srs)
    proof = pv.prove(pub, prv)

    def alpha_fn(dl):
        return o.transcript_challenge(co.xsk233_encode(co.k233_mulgen(dl)), pub)

    pr = o.prove_scalars(tree, st, pub, prv, alpha_fn) if oracle is None else oracle[2]
    for key in STAGE_VECTORS:
        assert from_limbs(pv.debug(key)) == pr[key], key
    for key in STAGE_SCALARS:
        assert from_limbs(pv.debug(key))[0] == pr[key], key
    assert proof.commit_p == co.xsk233_encode(co.k233_mulgen(pr["dl_commit_p"]))
    assert proof.kzg_k == co.xsk233_encode(co.k233_mulgen(pr["dl_kzg"]))
    assert proof.a0_fr() == (pr["a0"], True) and proof.b0_fr() == (pr["b0"], True)
    assert o.verify_dl(trap, pub, pr["dl_commit_p"], pr["dl_kzg"], pr["a0"], pr["b0"], pr["alpha"]) == verifies
    assert dvp.srs.verify(td, pub, proof) == verifies
    assert dvp.proving.Proof.from_bits(proof.to_bits()) == proof
    assert proof.to_bits() == o.proof_to_bits(proof.commit_p, proof.kzg_k, pr["a0"], pr["b0"])
    if golden:
        assert proof.commit_p.hex() == golden["commit_p"] and proof.kzg_k.hex() == golden["kzg_k"]
        assert hex(pr["alpha"]) == golden["alpha"]
    return pv, td, proof
