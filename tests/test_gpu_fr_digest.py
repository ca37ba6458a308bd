"""GPU tests (-m gpu) of dvp_fr_vec_digest / dvp_fr_vec_digest_dev against pyref.blake3 of the restated stream
(tests/prove_trace_cases.py): the lengths at which the packer and the hash tree change shape, canonical and Montgomery input, every
staging window, the unchecked _dev entry on all-ones entries, the host entry's range check, and the Fr-vector file."""
import numpy as np
import pytest

import pyref as o
import prove_trace_cases as tc
import msm_cases as mc

pytestmark = pytest.mark.gpu
EINVAL = -1
KNOB = "DVP_FR_DIGEST_WINDOW"
PACK, PACK_M, LEAVES, TREE = ("fr_digest.hip:k_frd_pack<false>", "fr_digest.hip:k_frd_pack<true>", "blake3_tree.hip:k_b3_leaves",
                              "blake3_tree.hip:k_b3_tree")


def on_device(limbs):
    """uint64 [n, 4] -> (tensor that keeps it alive, device address or 0)"""
    import torch

    if limbs.shape[0] == 0:
        return None, 0
    t = torch.from_numpy(np.ascontiguousarray(limbs).view(np.int64)).cuda()
    return t, t.data_ptr()


def raw_limbs(vals):
    from util import to_limbs

    return to_limbs(vals) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def all_entries(dvp, vals, want, windows=(None,)):
    """host entry, _dev canonical and _dev Montgomery of one vector under every window"""
    canon, mont = raw_limbs(vals), raw_limbs(tc.to_mont(vals))
    keep_c, dc = on_device(canon)
    keep_m, dm = on_device(mont)
    n = len(vals)
    for w in windows:
        with dvp.tune(**({} if w is None else {KNOB: w})):
            assert dvp.fr.vec_digest(canon) == want, (n, w, "host")
            assert dvp.fr.vec_digest_dev(dc, n) == want, (n, w, "dev")
            assert dvp.fr.vec_digest_dev(dm, n, montgomery=True) == want, (n, w, "dev, Montgomery")


@pytest.mark.parametrize("n", sorted(tc.LENGTHS), ids=lambda n: f"n{n}")
def test_lengths_where_the_packer_changes_shape(dvp, n):
    all_entries(dvp, tc.values(n), tc.digest_of_values(n), windows=(None, 1, 2, 5))


@pytest.fixture(scope="module")
def tree_run(dvp):
    return int(dvp.lib.dvp_debug_blake3_tree_run())


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_chunk_counts_around_the_tree_run(dvp, tree_run, delta):
    """one workgroup of the tree kernel reduces tree_run chaining values: one short of it, exactly it, and one more (a second level)"""
    n = tc.length_for_chunks(tree_run + delta)
    all_entries(dvp, tc.values(n), tc.digest_of_values(n), windows=(None, 100))
    dvp.lib.dvp_profile_reset()
    keep, d = on_device(raw_limbs(tc.values(n)))
    assert dvp.fr.vec_digest_dev(d, n) == tc.digest_of_values(n)
    assert (mc.launches(dvp, PACK), mc.launches(dvp, PACK_M), mc.launches(dvp, LEAVES)) == (1, 0, 1)
    assert mc.launches(dvp, TREE) == (2 if delta == 1 else 1)


def test_window_count_and_single_chunk_route(dvp):
    n = 601  # 18 chunks
    keep, d = on_device(raw_limbs(tc.values(n)))
    for w, launches in ((1, 18), (5, 4), (18, 1), (1000, 1)):
        dvp.lib.dvp_profile_reset()
        with dvp.tune(**{KNOB: w}):
            assert dvp.fr.vec_digest_dev(d, n) == tc.digest_of_values(n)
        assert (mc.launches(dvp, PACK), mc.launches(dvp, LEAVES), mc.launches(dvp, TREE)) == (launches, launches, 1), w
    dvp.lib.dvp_profile_reset()
    keep, d = on_device(raw_limbs(tc.values(35)))
    assert dvp.fr.vec_digest_dev(d, 35) == tc.digest_of_values(35)
    assert (mc.launches(dvp, PACK), mc.launches(dvp, LEAVES), mc.launches(dvp, TREE)) == (1, 1, 0)  # the ROOT flavour of the leaves


@pytest.mark.parametrize("n", (1, 4, 37, 601))
def test_all_ones_low_29_bytes(dvp, n):
    """the _dev entry hashes the low 29 bytes of whatever it is given: entries of 2^256 - 1 and of 2^232 - 1 both give 29 x 0xff"""
    want = o.blake3(n.to_bytes(8, "little") + b"\xff" * (29 * n))
    for v in ((1 << 256) - 1, (1 << 232) - 1):
        keep, d = on_device(raw_limbs([v] * n))
        assert dvp.fr.vec_digest_dev(d, n) == want
    assert want == tc.digest([(1 << 232) - 1] * n)


@pytest.mark.parametrize("n, bad", ((1, 0), (36, 35), (601, 17), (601, 600)))
def test_host_entry_refuses_a_non_canonical_entry(dvp, n, bad):
    vals = list(tc.values(n))
    for v in (o.P, (1 << 256) - 1):
        vals[bad] = v
        with pytest.raises(dvp.DvpError) as ei:
            dvp.fr.vec_digest(raw_limbs(vals))
        assert ei.value.status == EINVAL and ei.value.index == bad
    vals[bad] = o.P - 1
    assert dvp.fr.vec_digest(raw_limbs(vals)) == tc.digest(vals)


@pytest.mark.parametrize("n", (0, 36, 601))
def test_equals_blake3_of_the_fr_vec_file(dvp, tmp_path, n):
    vals = tc.values(n)
    path = tmp_path / "vec"
    dvp.io_utils.write_fr_vec_to_file(path, raw_limbs(vals))
    data = path.read_bytes()
    assert dvp.proving.blake3(data) == dvp.fr.vec_digest(raw_limbs(vals)) == tc.digest_of_values(n)


def test_null_arguments(dvp):
    lib = dvp.lib
    out = np.zeros(32, dtype=np.uint8)
    assert lib.dvp_fr_vec_digest(None, 1, dvp._native.ptr(out)) == EINVAL
    assert lib.dvp_fr_vec_digest(None, 0, None) == EINVAL
    assert lib.dvp_fr_vec_digest_dev(None, 1, 0, None, None) == EINVAL
    assert lib.dvp_fr_vec_digest(None, 0, dvp._native.ptr(out)) == 0 and out.tobytes() == o.blake3(bytes(8))
