"""-m gpu: the Blosc-lz4 decoder (tm_blosc_decompress_dev, tm_blosc_decompress_tiles) on the case table of
tests/blosc_decode_cases.py.

Every good frame -- the encoder's cases, the ten real c-blosc frames, streams longer than the 64 KiB history ring -- must
decode to its plain bytes from an unaligned source, all in one batch, into destinations with guard bytes on both sides, and
twice alike.  The corrupt streams (refused by the host decoder in tests/test_blosc_decode_cases_host.py and run through the
same walk under the sanitizers by tools/blosc_decode_check.cpp before they come here) must set their frame's status and
leave the good frames of the call and every guard alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import blosc_cases as bc
import blosc_decode_cases as dc
from teramind_amd import _lib, formats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, GAP = 0xA5, 48
TM_DTYPE_F32, TM_DTYPE_F16 = 0, 2


def decode_batch(frames, shift=3, dst_shift=1):
    """frames back to back `shift` bytes into an allocation -> (plain bytes per frame or None, status list); asserts the guards
    between, before and after the destinations, and the destination of a frame with a status, are untouched."""
    L = _lib.lib()
    n = len(frames)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    offs += shift
    host = np.full(int(offs[n]), 0x5A, np.uint8)
    for k, f in enumerate(frames):
        host[offs[k]:offs[k + 1]] = np.frombuffer(f, np.uint8)
    sizes = [int.from_bytes(f[4:8], "little") for f in frames]
    dst_offs = np.zeros(n, np.int64)
    at = GAP + dst_shift
    for k, sz in enumerate(sizes):
        dst_offs[k] = at
        at += sz + GAP + (k % 5)                                    # destinations at every alignment
    dev = torch.from_numpy(host).to(DEV)
    dst = torch.full((at,), GUARD, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.tm_blosc_decompress_dev(_lib.ptr(dev), host.ctypes.data, offs.ctypes.data, n, _lib.ptr(dst), dst.numel(), dst_offs.ctypes.data,
                                         _lib.ptr(status), _lib.current_stream_ptr()), "tm_blosc_decompress_dev")
    status = status.cpu().tolist()
    got = dst.cpu().numpy()
    keep = np.ones(at, bool)
    out = []
    for k, sz in enumerate(sizes):
        o = int(dst_offs[k])
        if status[k] == 0:
            keep[o:o + sz] = False
            out.append(got[o:o + sz].tobytes())
        else:
            out.append(None)                                        # nothing of a refused frame is delivered
    assert (got[keep] == GUARD).all(), "bytes outside the destinations of the decoded frames were written"
    return out, status


@pytest.fixture(scope="module")
def good_frames():
    return [dc.good(n) for n in dc.GOOD_NAMES]


def test_every_good_frame_in_one_batch(good_frames):
    frames = [f for f, _ in good_frames]
    got, status = decode_batch(frames)
    assert status == [0] * len(frames)
    for name, (_, plain), g in zip(dc.GOOD_NAMES, good_frames, got):
        assert g == plain, name
    again, status2 = decode_batch(frames, shift=0, dst_shift=0)      # twice, and from an aligned source too
    assert status2 == status and again == got


@pytest.mark.parametrize("name", ["long/far_match", "long/wrap_straddle", "long/overlap_wrap", "long/big_chunk", "fixture/f16_default",
                                  "fixture/f16_clevel0_memcpy", "fixture/f16_noshuffle", "case/half_background", "case/n1_ts2"])
@pytest.mark.parametrize("shift", [1, 2])
def test_single_frames_unaligned(name, shift):
    frame, plain = dc.good(name)
    got, status = decode_batch([frame], shift=shift, dst_shift=shift + 4)
    assert status == [0] and got[0] == plain


def test_compress_then_decompress_is_the_identity():
    L = _lib.lib()
    frames, plains = [], []
    for name, (make, ts, bs, _why) in bc.CASES.items():
        data = make()
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
        bound = L.tm_blosc_bound(len(data), ts, bs)
        buf = torch.empty(bound, dtype=torch.uint8, device=DEV)
        n = torch.zeros(1, dtype=torch.int64, device=DEV)
        _lib.check(L.tm_blosc_compress(_lib.ptr(src), len(data), ts, bs, _lib.ptr(buf), bound, _lib.ptr(n), _lib.current_stream_ptr()),
                   "tm_blosc_compress")
        frames.append(buf[:int(n.item())].cpu().numpy().tobytes())
        plains.append(data)
    got, status = decode_batch(frames)
    assert status == [0] * len(frames)
    for name, g, p in zip(bc.CASES, got, plains):
        assert g == p, name


@pytest.mark.parametrize("name", list(dc.CORRUPT_STREAMS))
def test_corrupt_stream_in_a_batch_with_good_frames(name):
    picks = ["case/block_plus3_ts4", "long/overlap_wrap", "fixture/f16_small_default"]
    good = [dc.good(n) for n in picks]
    frames = [good[0][0], dc.corrupt_stream_frame(name), good[1][0], good[2][0]]
    got, status = decode_batch(frames)
    assert status[1] != 0 and [status[0], status[2], status[3]] == [0, 0, 0], status
    assert [got[0], got[2], got[3]] == [g[1] for g in good]
    print(f"blosc decode {name}: status {status[1]}")


def test_two_corrupt_frames_keep_their_own_status():
    frames = [dc.corrupt_stream_frame("offset_zero"), dc._host_frame()[0], dc.corrupt_stream_frame("ends_short")]
    got, status = decode_batch(frames)
    assert status == [6, 0, 1] and got[1] == dc._host_frame()[1]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("name", list(dc.GRID_CASES))
def test_canvas_sink_places_the_chunk_grid(name, dtype, tmp_path):
    """The chunks of a zarr array land in a box of a pitched canvas as read_zarr_zip assembles them; nothing around it changes."""
    shape, chunks = dc.GRID_CASES[name]
    path = tmp_path / "a.zip"
    dc.write_grid_zip(path, shape, chunks)
    want = torch.from_numpy(formats.read_zarr_zip(path)).to(DEV)
    C_, H, W = shape[0] + 2, shape[1] + 5, shape[2] + 11              # an odd pitch, rows and channels around the box
    canvas = torch.full((C_, H, W), 7.0, dtype=dtype, device=DEV)
    ref = canvas.clone()
    y0, x0 = 3, 9 if name.endswith("clipped") else 8
    meta, members = formats.read_zarr_zip_frames(path)
    origin = 1 * canvas.stride(0) + y0 * canvas.stride(1) + x0
    jobs = formats.gpu_chunk_jobs(path, meta, members, origin, canvas.stride(0), canvas.stride(1))
    assert formats.decode_chunks_dev(canvas, jobs) == [0] * len(jobs)
    ref[1:1 + shape[0], y0:y0 + shape[1], x0:x0 + shape[2]] = want.to(dtype)
    assert torch.equal(canvas.view(torch.int16 if dtype == torch.float16 else torch.int32), ref.view(torch.int16 if dtype == torch.float16 else torch.int32))


def test_canvas_sink_takes_the_big_chunk_and_unshuffled_frames():
    """A [25, 64, 128] chunk at block size 262144 (the reference's chunking) and c-blosc's unshuffled / memcpyed frames into a canvas."""
    for name, chunk in (("long/big_chunk", (25, 64, 128)), ("fixture/f16_noshuffle", (3, 100, 100)), ("fixture/f16_clevel0_memcpy", (3, 10, 100)),
                        ("fixture/f16_default", (3, 1000, 100))):
        frame, plain = dc.good(name)
        assert len(plain) == 2 * int(np.prod(chunk))
        for dtype in (torch.float16, torch.float32):
            canvas = torch.zeros((chunk[0], chunk[1] + 1, chunk[2] + 8), dtype=dtype, device=DEV)
            assert formats.decode_chunks_dev(canvas, [(frame, 0, chunk, chunk)]) == [0]
            want = torch.from_numpy(np.frombuffer(plain, "<f2").reshape(chunk).copy()).to(DEV)
            assert torch.equal(canvas[:, :chunk[1], :chunk[2]], want.to(dtype)) and not canvas[:, chunk[1]:].any() and not canvas[:, :, chunk[2]:].any()
