"""CPU: the case table of the GPU Blosc decoder (tests/blosc_decode_cases.py) against the host readers, and the host half of
the new entry points -- tm_blosc_frame_info and the frame walk that tm_blosc_decompress_dev / _tiles run before any device
call (null device pointers are enough: the walk comes first)."""
import ctypes as C
import os

import numpy as np
import pytest

import blosc_cases as bc
import blosc_decode_cases as dc
import util
from teramind_amd import _lib, formats

TM_ERR_ARG = -1


def host_decode(frame: bytes):
    """tm_blosc_decompress -> (return code, plain bytes or None)"""
    L = _lib.lib()
    n = C.c_size_t(0)
    if L.tm_blosc_decompress(frame, len(frame), None, 0, C.byref(n)) != 0:
        return TM_ERR_ARG, None
    out = (C.c_char * max(1, n.value))()
    rc = L.tm_blosc_decompress(frame, len(frame), out, n.value, C.byref(n))
    return rc, bytes(out[:n.value]) if rc == 0 else None


@pytest.mark.parametrize("name", dc.GOOD_NAMES)
def test_good_frames_decode_on_the_host(name):
    frame, plain = dc.good(name)
    if name == "fixture/f16_clevel0_memcpy":                       # the strict parser knows no memcpyed frames
        with pytest.raises(bc.BloscError, match="memcpyed"):
            bc.decode_frame(frame)
    else:
        assert bc.decode_frame(frame) == plain
    assert host_decode(frame) == (0, plain)
    info = formats.blosc_frame_info(frame)
    streams, _sh, ts, _bs = dc.walk_frame(frame)
    assert info.gpu == 1 and info.nbytes == len(plain) and info.typesize == ts
    assert info.nstreams == len(streams) and info.longest == max(s[2] for s in streams)


def test_long_cases_are_what_they_claim():
    info = formats.blosc_frame_info(dc.good("long/big_chunk")[0])
    assert (info.nbytes, info.blocksize, info.nstreams, info.longest) == (409600, 262144, 3, 147456)
    streams = dc.walk_frame(dc.good("long/big_chunk")[0])[0]
    assert [s[2] for s in streams] == [131072, 131072, 147456] and streams[2][1] != streams[2][2]      # the leftover is an LZ4 stream
    for n in dc.LONG_CASES:
        frame, plain = dc.good(f"long/{n}")
        (j, sp, ne, data, stored), = bc.parse_frame(frame)["streams"]
        assert not stored and ne == len(plain) > 2 * dc.RING
        _, seqs = bc.lz4_sequences(data, ne)
        pos, far, across, lit_across = 0, False, set(), False
        for ll, off, ml in seqs:
            lit_across |= pos // dc.RING != (pos + ll - 1) // dc.RING if ll else False
            pos += ll
            if off:
                far |= off == 65535 and pos - off > dc.RING
                if pos // dc.RING != (pos + ml - 1) // dc.RING:
                    across.add(off if off < ml else 0)
                pos += ml
        if n == "far_match":
            assert far
        if n == "wrap_straddle":
            assert lit_across and 0 in across
        if n == "overlap_wrap":
            assert {1, 3, 63} <= across and any(ml > dc.RING for _, _, ml in seqs)


@pytest.mark.parametrize("name", list(dc.CORRUPT_STREAMS))
def test_host_decoder_refuses_the_corrupt_streams(name):
    """The list is one the reference reader itself rejects -- only then do these frames go to the GPU."""
    frame = dc.corrupt_stream_frame(name)
    rc, _ = host_decode(frame)
    assert rc == TM_ERR_ARG and b"lz4 stream" in _lib.lib().tm_last_error()
    info = formats.blosc_frame_info(frame)                          # the frame itself is sound: the GPU decoder takes it
    assert info.gpu == 1 and info.nstreams == 9
    good, plain = dc._host_frame()
    assert host_decode(good) == (0, plain)


def test_flipped_stream_byte_is_refused_on_the_host():
    good, _ = dc._host_frame()
    bad = dc.flipped_stream_byte(good)
    assert len(bad) == len(good) and sum(a != b for a, b in zip(good, bad)) == 1
    assert host_decode(bad)[0] == TM_ERR_ARG


def _entry_points(frame: bytes):
    """The two device entry points on one frame with null device pointers -> their return codes and texts."""
    L = _lib.lib()
    offs = (C.c_int64 * 2)(0, len(frame))
    dst_off = (C.c_int64 * 1)(0)
    box = _lib.TmBloscBox()
    out = []
    rc = L.tm_blosc_decompress_dev(None, frame, offs, 1, None, 1 << 30, dst_off, None, None)
    out.append((rc, L.tm_last_error()))
    rc = L.tm_blosc_decompress_tiles(None, frame, offs, 1, None, 2, 1 << 30, 1 << 20, 1 << 10, C.byref(box), None, None)
    out.append((rc, L.tm_last_error()))
    return out


@pytest.mark.parametrize("name", list(dc.corrupt_frames()))
def test_corrupt_and_host_only_frames_are_answered_before_any_device_call(name):
    frame, kind = dc.corrupt_frames()[name]
    L = _lib.lib()
    info = _lib.TmBloscFrame()
    rc = L.tm_blosc_frame_info(frame, len(frame), C.byref(info))
    if kind == "refused":
        assert rc == TM_ERR_ARG and L.tm_last_error()
        with pytest.raises(ValueError):
            formats.blosc_frame_info(frame)
        for rc, text in _entry_points(frame):
            assert rc == TM_ERR_ARG and b"frame 0" in text and b"null" not in text
    else:
        assert rc == 0 and info.gpu == 0 and info.nstreams == 0     # a distinct answer, not an error
        for rc, text in _entry_points(frame):
            assert rc == TM_ERR_ARG and b"host only" in text


def test_entry_points_check_their_arguments_without_device():
    L = _lib.lib()
    frame, plain = dc._host_frame()
    for rc, text in _entry_points(frame):                           # a sound frame: the null device pointers are found next
        assert rc == TM_ERR_ARG and b"null" in text
    offs = (C.c_int64 * 2)(0, len(frame))
    dst_off = (C.c_int64 * 1)(0)
    p = C.c_void_p(16)                                              # never dereferenced: the checks come first
    assert L.tm_blosc_decompress_dev(p, frame, offs, 1, p, len(plain) - 1, dst_off, p, None) == TM_ERR_ARG
    assert b"leave the destination" in L.tm_last_error()
    assert L.tm_blosc_decompress_dev(p, frame, offs, 0, p, len(plain), dst_off, p, None) == TM_ERR_ARG
    bad = (C.c_int64 * 2)(8, 0)
    assert L.tm_blosc_decompress_dev(p, frame, bad, 1, p, len(plain), dst_off, p, None) == TM_ERR_ARG
    assert b"decrease" in L.tm_last_error()
    # the canvas sink: the chunk must be the frame's float16 elements, the box must lie inside the canvas
    n = len(plain) // 2
    box = _lib.TmBloscBox()
    box.origin, box.chunk[:], box.clip[:] = 0, (1, 1, n), (1, 1, n)
    args = lambda canvas_elems, pitch=n: (p, frame, offs, 1, p, 2, canvas_elems, n, pitch, C.byref(box), p, None)
    assert L.tm_blosc_decompress_tiles(*args(n - 1)) == TM_ERR_ARG and b"leaves the canvas" in L.tm_last_error()
    assert L.tm_blosc_decompress_tiles(*args(n, pitch=n - 1)) == TM_ERR_ARG and b"pitch" in L.tm_last_error()
    box.chunk[:] = (1, 1, n - 1)
    box.clip[:] = (1, 1, n - 1)
    assert L.tm_blosc_decompress_tiles(*args(n)) == TM_ERR_ARG and b"float16 of its chunk" in L.tm_last_error()
    box.chunk[:], box.clip[:] = (1, 1, n), (1, 2, n)
    assert L.tm_blosc_decompress_tiles(*args(n)) == TM_ERR_ARG and b"clip" in L.tm_last_error()


@pytest.mark.parametrize("name", ["io_state_tile_blosc.zip"])
def test_read_zarr_zip_frames_agrees_with_read_zarr_zip(name):
    path = os.path.join(util.ROOT, "tests", "golden", name)
    meta, members = formats.read_zarr_zip_frames(path)
    want = formats.read_zarr_zip(path)
    assert tuple(meta["shape"]) == want.shape == (6, 40, 48) and sorted(members) == ["0.0.0", "1.0.0"]
    c0 = meta["chunks"][0]
    for key, raw in members.items():
        i = int(key.split(".")[0])
        blk = np.frombuffer(formats._decode_chunk(raw, meta["compressor"]), "<f2").reshape(meta["chunks"])
        assert np.array_equal(blk.view(np.uint16), want[i * c0:(i + 1) * c0].view(np.uint16))
        assert formats.blosc_frame_info(raw).gpu == 1
    jobs = formats.gpu_chunk_jobs(path, meta, members, 7, 40 * 48, 48)
    assert [(j[1], j[2], j[3]) for j in jobs] == [(7, (3, 40, 48), (3, 40, 48)), (7 + 3 * 40 * 48, (3, 40, 48), (3, 40, 48))]


def test_grid_cases_read_back_on_the_host(tmp_path):
    """The chunk-grid files of the GPU tests are what read_zarr_zip reads (edge chunks stored full size and clipped)."""
    for name, (shape, chunks) in dc.GRID_CASES.items():
        path = tmp_path / f"{name}.zip"
        a = dc.write_grid_zip(path, shape, chunks)
        assert np.array_equal(formats.read_zarr_zip(path).view(np.uint16), a.view(np.uint16))
        meta, members = formats.read_zarr_zip_frames(path)
        jobs = formats.gpu_chunk_jobs(path, meta, members, 0, shape[1] * shape[2], shape[2])
        assert len(jobs) == len(members) == int(np.prod([(s + c - 1) // c for s, c in zip(shape, chunks)]))
        assert all(j[3] == tuple(min(c, s) for c, s in zip(chunks, shape)) for j in jobs[:1])
    # zlib and raw files are the host route's
    arr = dc.grid_array((4, 8, 8))
    for comp in (None, "zlib"):
        formats.write_zarr_zip(tmp_path / "t.zip", arr, comp)
        meta, members = formats.read_zarr_zip_frames(tmp_path / "t.zip")
        assert formats.gpu_chunk_jobs("t.zip", meta, members, 0, 64, 8) is None
