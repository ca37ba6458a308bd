"""GPU tests (-m gpu) of the chunk-parallel BLAKE3 over a device buffer (csrc/blake3_tree.hip: dvp_blake3_dev): the oracle's long
vectors at every byte alignment, the chunk counts at which the leaf and tree launches change shape against the host BLAKE3 (which
tests/test_binding_cpu.py pins to the same vectors), a stream hashed piecewise, and the argument rules."""
import ctypes as C

import numpy as np
import pytest

import binding_cases as bc

pytestmark = pytest.mark.gpu
PAD = 64  # guard bytes in front of and behind every input


def dev_hash(dvp, data: bytes, off: int = 0, stream: int = 0) -> bytes:
    """dvp_blake3_dev of `data` placed `off` bytes past a 64-byte boundary, 0xA5 everywhere around it: an over-read or a slip of the
    alignment handling changes the digest"""
    import torch

    host = np.full(PAD + off + len(data) + PAD, 0xA5, dtype=np.uint8)
    host[PAD + off:PAD + off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 64 == 0
    return dvp.proving.blake3_dev(buf.data_ptr() + PAD + off, len(data), stream)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_long_vectors_at_every_alignment(dvp, off):
    for n, h in bc.B3_LONG.items():
        assert dev_hash(dvp, bc.b3_input(n), off).hex() == h, (n, off)


def test_chunk_counts_where_the_launches_change_shape(dvp):
    """63 / 64 / 65 chunks (one wave of the leaf kernel), 255 / 256 / 257, and one below / at / above the run one workgroup of the
    tree kernel reduces (a second tree launch), those three also with a ragged last chunk of 1 and of 1023 bytes"""
    run = int(dvp.lib.dvp_debug_blake3_tree_run())
    rng = np.random.default_rng(233)
    data = rng.integers(0, 256, size=(run + 1) * 1024, dtype=np.uint8).tobytes()
    lens = [1024 * k for k in (63, 64, 65, 255, 256, 257, run - 1, run, run + 1)]
    lens += [1024 * (k - 1) + tail for k in (run - 1, run, run + 1) for tail in (1, 1023)]
    for i, n in enumerate(lens):
        assert dev_hash(dvp, data[:n], i % 4) == dvp.proving.blake3(data[:n]), n


def test_more_than_2_16_chunks(dvp):
    """64 MiB + 1025 bytes: 65538 chunks, three tree launches, a one-byte last chunk"""
    import torch

    n = (64 << 20) + 1025
    g = torch.Generator(device="cpu").manual_seed(64)
    host = torch.randint(0, 256, (n + 2 * PAD,), dtype=torch.uint8, generator=g)
    host[:PAD + 1] = 0xA5
    host[PAD + 1 + n:] = 0xA5
    buf = host.cuda()
    got = dvp.proving.blake3_dev(buf.data_ptr() + PAD + 1, n)
    assert got == dvp.proving.blake3(host[PAD + 1:PAD + 1 + n].numpy().tobytes())


def test_piecewise_with_a_counter_base(dvp):
    """a 300 KB stream cut at multiples of 15360 bytes (whole 30-byte records AND whole chunks, the SRS hash's window rule): the
    leaves of every piece, hashed from a buffer of its own with the piece's chunk offset as the counter base, reduce to the digest of
    one call over the whole stream"""
    import torch

    lib = dvp.lib
    n = 300_000
    rng = np.random.default_rng(300)
    stream_bytes = rng.integers(0, 256, size=n, dtype=np.uint8)
    want = dvp.proving.blake3(stream_bytes.tobytes())
    assert dev_hash(dvp, stream_bytes.tobytes(), 2) == want
    nchunks = (n + 1023) // 1024
    cvs = torch.zeros(nchunks * 32, dtype=torch.uint8, device="cuda")
    tmp = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(32, dtype=torch.uint8, device="cuda")
    cuts = [0] + [15360 * k for k in (1, 4, 5, 12, 19)] + [n]
    keep = []
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        host = np.full(PAD + 3 + (hi - lo) + PAD, 0xA5, dtype=np.uint8)
        off = PAD + i % 4
        host[off:off + hi - lo] = stream_bytes[lo:hi]
        piece = torch.from_numpy(host).cuda()
        keep.append(piece)
        assert lo % 1024 == 0
        dvp.check(lib.dvp_debug_blake3_leaves_dev(piece.data_ptr() + off, hi - lo, lo // 1024, cvs.data_ptr() + 32 * (lo // 1024), None), "leaves")
    dvp.check(lib.dvp_debug_blake3_reduce_dev(cvs.data_ptr(), nchunks, tmp.data_ptr(), out.data_ptr(), None), "reduce")
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want
    # without the counter base the second piece hashes as if it began the stream: the digest must differ
    lo, hi = cuts[1], cuts[2]
    dvp.check(lib.dvp_debug_blake3_leaves_dev(keep[0].data_ptr() + PAD, cuts[1], 0, cvs.data_ptr(), None), "leaves")
    dvp.check(lib.dvp_debug_blake3_leaves_dev(keep[1].data_ptr() + PAD + 1, hi - lo, 0, cvs.data_ptr() + 32 * (lo // 1024), None), "leaves")
    dvp.check(lib.dvp_debug_blake3_reduce_dev(cvs.data_ptr(), hi // 1024, tmp.data_ptr(), out.data_ptr(), None), "reduce")
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() != dvp.proving.blake3(stream_bytes[:hi].tobytes())


def test_arguments_and_no_wait(dvp):
    import torch

    lib = dvp.lib
    out = torch.zeros(32, dtype=torch.uint8, device="cuda")
    # len = 0: one empty chunk, the pointer may be NULL
    dvp.check(lib.dvp_blake3_dev(None, 0, out.data_ptr(), None), "dvp_blake3_dev")
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes().hex() == bc.B3_LONG[0]
    assert lib.dvp_blake3_dev(None, 1, out.data_ptr(), None) == -1
    assert lib.dvp_blake3_dev(out.data_ptr(), 32, None, None) == -1
    assert lib.dvp_blake3_dev(out.data_ptr(), (1 << 40) + 1, out.data_ptr(), None) == -1
    # the call enqueues and returns: behind a few ms of device-side spinning on its stream (5 M ticks: 2.5 ms of a 2 GHz counter, 50 ms
    # of a 100 MHz one) it comes back while the stream is still busy
    data = torch.from_numpy(np.frombuffer(bc.b3_input(102400), dtype=np.uint8).copy()).cuda()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda._sleep(5_000_000)
        dvp.check(lib.dvp_blake3_dev(data.data_ptr(), 102400, out.data_ptr(), C.c_void_p(st.cuda_stream)), "dvp_blake3_dev")
        returned_while_busy = not st.query()
    st.synchronize()
    assert out.cpu().numpy().tobytes().hex() == bc.B3_LONG[102400]
    assert returned_while_busy
