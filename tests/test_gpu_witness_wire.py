"""GPU tests (-m gpu) of the witness wire: k_fr_from_be32 (csrc/fr_wire.hip) against Python integers at the block-edge sizes, and the
entries that prove from gnark's witness bytes -- dvp_prove_be32, dvp_prove_cache_dir_witness_file, the compiled CLI -- against
dvp_prove on the same statement.  Every witness is presented UNREDUCED: element 0 and every other private element as x + k p < 2^256,
so an entry that skipped the reduction cannot produce the bytes of dvp_prove (it would be refused as non-canonical, or prove another
statement)."""
import os
import random
import struct

import numpy as np
import pytest

import msm_cases as mc
import pyref as o
import witness_cases as wc

pytestmark = pytest.mark.gpu
KERNEL = "fr_wire.hip:k_fr_from_be32"
EINVAL, EUNSAT = -1, -3
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, len(wc.VALUES)]  # around the wave (64) and the workgroup (256), several workgroups


def limbs_bytes(ints):
    return b"".join(x.to_bytes(32, "little") for x in ints)


@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_python_integers(dvp, n):
    import torch

    raw = np.frombuffer(wc.be32(wc.VALUES[:n]), dtype=np.uint8)
    want = limbs_bytes(wc.EXPECTED[:n])
    # host flavour, from an address that is not even 2-byte aligned (a file's payload starts at byte 4)
    odd = np.frombuffer(b"\x00" * 3 + raw.tobytes(), dtype=np.uint8)[3:]
    dvp.lib.dvp_profile_reset()
    assert dvp.fr.from_be32(odd).tobytes() == want
    assert mc.launches(dvp, KERNEL) == 1
    st = torch.cuda.current_stream().cuda_stream
    # device flavour, out of place: the input stays, and nothing is written beyond element n - 1
    src = torch.from_numpy(raw.copy()).cuda()
    dst = torch.full((32 * (n + 2),), 0xAB, dtype=torch.uint8, device="cuda")
    dvp.lib.dvp_profile_reset()
    dvp.fr.from_be32_dev(src.data_ptr(), n, dst.data_ptr(), st)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().tobytes()
    assert got[:32 * n] == want and got[32 * n:] == b"\xab" * 64
    assert src.cpu().numpy().tobytes() == raw.tobytes()
    assert mc.launches(dvp, KERNEL) == 1
    # device flavour, in place
    buf = torch.full((32 * (n + 2),), 0xCD, dtype=torch.uint8, device="cuda")
    buf[:32 * n] = src
    dvp.lib.dvp_profile_reset()
    dvp.fr.from_be32_dev(buf.data_ptr(), n, None, st)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert got[:32 * n] == want and got[32 * n:] == b"\xcd" * 64
    assert mc.launches(dvp, KERNEL) == 1


# ---- proofs ---------------------------------------------------------------------------------------------------------------------
LIFTS = (1, 3, 2**24 - 1, wc.K_MAX - 1)  # x + k p < 2^256 for every x < p and k <= K_MAX - 1


def unreduced(w, n_public):
    """the witness [1, public.., private..] with element 0 and every other private element replaced by another representative"""
    out = list(w)
    out[0] = 1 + LIFTS[2] * wc.P
    first_private = 1 + n_public
    lifted = 0
    for j, i in enumerate(range(first_private, len(w), 2)):
        out[i] = w[i] + LIFTS[j % 4] * wc.P
        lifted += 1
    assert 4 * lifted >= len(w) - first_private and all(0 <= x < 2**256 for x in out)
    assert [x % wc.P for x in out] == [x % wc.P for x in w] and out != list(w)
    return out


@pytest.fixture(scope="module")
def statements(dvp):
    """name -> (prover, trapdoor, public, private): the toy circuit (config #1) and synthetic_sparse(10), with two public inputs and
    with none (the toy circuit's public wires are then private ones)"""
    g = dvp.gnark_r1cs
    made = {}
    rnd = random.Random(0xBE32)
    toy_w = list(g.TOY_PUBLIC) + list(g.TOY_PRIVATE)
    sp2 = g.synthetic_sparse(10)
    sp0 = g.synthetic_sparse(10, n_public=0)
    for name, inst, pub, prv in (("toy", g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 2), toy_w[:2], toy_w[2:]),
                                 ("toy-nopub", g.R1CSInstance.from_rows(g.TOY_ROWS, g.TOY_COEFFS, 0), [], toy_w),
                                 ("sparse10", *sp2), ("sparse10-nopub", *sp0)):
        td = dvp.srs.Trapdoor(rnd.randrange(1, o.P), rnd.randrange(1, o.P), rnd.randrange(1, o.P))
        pv = dvp.proving.Prover(inst)
        pv.set_srs(dvp.srs.verifier_runs_setup(pv, inst, td))
        made[name] = (pv, td, list(pub), list(prv))
    yield made
    for pv, *_ in made.values():
        pv.close()


@pytest.mark.parametrize("devices", [[], [0, 0]], ids=["one-device", "devices-0-0"])
@pytest.mark.parametrize("name", ["toy", "toy-nopub", "sparse10", "sparse10-nopub"])
def test_prove_be32_same_bytes_as_prove(dvp, statements, name, devices):
    pv, td, pub, prv = statements[name]
    raw = wc.be32(unreduced([1] + pub + prv, len(pub)))
    try:
        dvp.set_devices(devices)
        ref = pv.prove(pub, prv)
        dvp.lib.dvp_profile_reset()
        got = pv.prove_be32(raw)
        assert mc.launches(dvp, KERNEL) == 1
    finally:
        dvp.set_devices([])
    assert got.to_bytes() == ref.to_bytes()
    assert dvp.srs.verify(td, pub, got)


def test_prove_be32_errors(dvp, statements):
    pv, _, pub, prv = statements["sparse10"]
    w = unreduced([1] + pub + prv, len(pub))
    ref = pv.prove(pub, prv)
    # a longer buffer: only the first n_wires elements are read (garbage behind them, an unreduced maximum included)
    assert pv.prove_be32(wc.be32(w + [2**256 - 1, 0, 12345])).to_bytes() == ref.to_bytes()
    # a shorter one
    with pytest.raises(dvp.DvpError) as e:
        pv.prove_be32(wc.be32(w[:-1]))
    assert e.value.status == EINVAL
    with pytest.raises(dvp.DvpError) as e:
        pv.prove_be32(b"")
    assert e.value.status == EINVAL
    # element 0 must be the constant 1: refused on the host, index 0, and the kernel never ran
    for e0 in (0, 2, wc.P, 2 + 5 * wc.P):
        dvp.lib.dvp_profile_reset()
        with pytest.raises(dvp.DvpError) as e:
            pv.prove_be32(wc.be32([e0] + w[1:]))
        assert (e.value.status, e.value.index) == (EINVAL, 0), e0
        assert mc.launches(dvp, KERNEL) == 0
    # an unsatisfied witness: DVP_EUNSAT with the row dvp_prove reports
    bad = list(prv)
    bad[100] = (bad[100] + 1) % o.P
    with pytest.raises(dvp.DvpError) as e1:
        pv.prove(pub, bad)
    with pytest.raises(dvp.DvpError) as e2:
        pv.prove_be32(wc.be32(unreduced([1] + pub + bad, len(pub))))
    assert e1.value.status == e2.value.status == EUNSAT and e1.value.index == e2.value.index >= 0
    # and the prover is fine afterwards
    assert pv.prove_be32(wc.be32(w)).to_bytes() == ref.to_bytes()


# ---- the file entry and the compiled host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cache(dvp, tmp_path_factory):
    """a cache_dir for synthetic_sparse(10) whose witness file holds the unreduced witness; (path, trapdoor, public, private, the Python
    host's proof from canonical limbs)"""
    A, g = dvp.artifacts, dvp.gnark_r1cs
    inst0, pub, prv = g.synthetic_sparse(10)
    path = tmp_path_factory.mktemp("witness_wire") / "cache"
    path.mkdir()
    inst0.write_dump_file(path / A.R1CS_CONSTRAINTS_FILE)
    (path / A.R1CS_WITNESS_FILE).write_bytes(wc.witness_file_bytes(unreduced([1] + pub + prv, len(pub))))
    td = dvp.srs.Trapdoor(31, 41, 59)
    _, pv = dvp.srs.verifier_runs_setup_cache_dir(td, path, len(pub), write_precomputes=False)
    pv.close()
    n_wires = struct.unpack("<Q", (path / A.SRS_G_M).read_bytes()[:8])[0]
    assert n_wires == 1 + len(pub) + len(prv)
    ref = dvp.proving.Proof.prove(path, pub, prv)
    assert dvp.srs.verify(td, pub, ref)
    yield path, td, pub, prv, ref
    dvp.proving.release_cache_dir()


def test_file_entry_same_bytes_as_python_host(dvp, cache, tmp_path):
    import threading

    path, _, pub, prv, ref = cache
    prove_file = dvp.proving.Proof.prove_witness_file
    dvp.lib.dvp_profile_reset()
    got, got_pub = prove_file(path, len(pub))  # NULL path: <cache_dir>/witness_to_dvsnark
    assert mc.launches(dvp, KERNEL) == 1
    assert got.to_bytes() == ref.to_bytes()
    assert got_pub.shape == (len(pub), 4) and dvp.fr.to_ints(got_pub) == pub
    # explicit path; a file with extra elements behind the witness (the reference's zip drops them as well)
    other = tmp_path / "elsewhere"
    w = unreduced([1] + pub + prv, len(pub))
    other.write_bytes(wc.witness_file_bytes(w + [2**256 - 1, 7]))
    got2, pub2 = prove_file(path, len(pub), other)
    assert got2.to_bytes() == ref.to_bytes() and dvp.fr.to_ints(pub2) == pub
    # the Python host on the raw payload: read_witness_raw + fr.from_be32 is load_witness_from_file
    raw = dvp.gnark_r1cs.read_witness_raw(other)
    assert raw.shape == (len(w) + 2, 32)
    assert np.array_equal(dvp.fr.from_be32(raw), dvp.gnark_r1cs.load_witness_from_file(other))
    # a file shorter than the commitment key
    other.write_bytes(wc.witness_file_bytes(w[:-1]))
    with pytest.raises(dvp.DvpError) as e:
        prove_file(path, len(pub), other)
    assert e.value.status == EINVAL
    # two host threads on one cache_dir at once
    bad = []

    def loop():
        try:
            for _ in range(4):
                p, pi = prove_file(path, len(pub))
                if p.to_bytes() != ref.to_bytes() or dvp.fr.to_ints(pi) != pub:
                    bad.append("bytes")
        except Exception as ex:  # noqa: BLE001 -- report from the main thread
            bad.append(repr(ex))

    th = [threading.Thread(target=loop) for _ in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, bad


def test_cli_default_and_host_witness_print_the_same_bytes(dvp, cache, tmp_path):
    import shutil
    import subprocess

    path, _, pub, _, ref = cache
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "no g++: the compiled host cannot be built"
    exe = tmp_path / "dvp_prove_cli"
    libdir = os.path.join(root, "dv-pari_amd")
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "dvp_prove_cli.cpp"),
                           "-L" + libdir, "-ldvpari_hip", "-Wl,-rpath," + libdir, "-pthread", "-o", str(exe)])
    env = dict(os.environ, DVP_NO_TORCH_PRELOAD="1")
    outs = []
    for extra in ([], ["--host-witness"]):
        out = subprocess.run([str(exe), str(path), str(len(pub))] + extra, capture_output=True, text=True, env=env, timeout=120)
        assert out.returncode == 0, (extra, out.stderr)
        outs.append(out.stdout)
    assert outs[0] == outs[1] and bytes.fromhex(outs[0].strip()) == ref.to_bytes()
