"""CPU: the numpy restatement of baseline JPEG (jpeg_cases.py) against libjpeg through Pillow, byte for byte; the tables
datastream of the library; the argument checks of the export entry points (before any device call)."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
from teramind_amd import _lib, ometiff


def _segments(data):
    """[(marker, payload)] of a JPEG datastream up to SOS, and the entropy-coded bytes between SOS and EOI."""
    segs, i = [], 2
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    while True:
        assert data[i] == 0xFF
        marker, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        segs.append((marker, data[i + 4:i + 2 + n]))
        i += 2 + n
        if marker == 0xDA:
            return segs, data[i:-2]
        if data[i:i + 2] == b"\xff\xd9":
            return segs, b""


def _pillow(img, quality):
    buf = io.BytesIO()
    Image.fromarray(img, mode="L").save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


@pytest.mark.parametrize("quality", jc.QUALITIES)
@pytest.mark.parametrize("name", list(jc.FULL_CASES))
def test_restatement_equals_libjpeg(name, quality):
    _, scan = _segments(_pillow(jc.image(name), quality))
    ours, = jc.reference_scans(name, quality)
    assert ours == scan


def test_noise_at_quality_100_outgrows_its_pixels():
    assert len(jc.reference_scans("noise", 100)[0]) > 256 * 256          # the too-small-slot case is reachable


@pytest.mark.parametrize("quality", jc.QUALITIES + (50, 49))
def test_tables_datastream_equals_pillows(quality):
    segs, _ = _segments(_pillow(jc.image("smooth"), quality))
    want = [(m, p) for m, p in segs if m in (0xDB, 0xC4)]
    ours, rest = _segments(ometiff.jpeg_tables(quality))
    assert rest == b"" and ours == want
    assert [m for m, _ in ours] == [0xDB, 0xC4, 0xC4]
    # and they are the tables of the restatement
    assert ours[0][1] == bytes([0]) + bytes(jc.quant_table(quality)[jc.ZIGZAG].tolist())
    assert ours[1][1] == bytes([0x00] + jc.DC_BITS + jc.DC_VALS)
    assert ours[2][1] == bytes([0x10] + jc.AC_BITS + jc.AC_VALS)


def test_tile_stream_decodes_with_the_tables():
    """tables + abbreviated stream are one valid JPEG: Pillow decodes the merged datastream to libjpeg's own decode."""
    img, q = jc.image("smooth"), 75
    tables, stream = ometiff.jpeg_tables(q), ometiff.jpeg_tile_stream(jc.reference_scans("smooth", q)[0])
    merged = tables[:-2] + stream[2:]
    got = np.asarray(Image.open(io.BytesIO(merged)))
    want = np.asarray(Image.open(io.BytesIO(_pillow(img, q))))
    assert got.shape == (256, 256) and np.array_equal(got, want)


def test_argument_checks_without_device():
    L = _lib.lib()
    buf = (C.c_uint8 * 512)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_size_t(0)
    ARG = -1
    # tm_jpeg_tables
    assert L.tm_jpeg_tables(0, p, 512, C.byref(n)) == ARG and b"quality" in L.tm_last_error()
    assert L.tm_jpeg_tables(101, p, 512, C.byref(n)) == ARG
    assert L.tm_jpeg_tables(75, None, 0, None) == ARG
    assert L.tm_jpeg_tables(75, p, 100, C.byref(n)) == ARG and n.value == 289
    assert L.tm_jpeg_tables(75, None, 0, C.byref(n)) == 0 and n.value == 289
    # tm_u8_shrink2(src, H, W, src_pitch, dst, dst_pitch, stream)
    assert L.tm_u8_shrink2(None, 4, 4, 4, p, 2, None) == ARG and b"null" in L.tm_last_error()
    assert L.tm_u8_shrink2(p, 4, 4, 4, None, 2, None) == ARG
    assert L.tm_u8_shrink2(p, 0, 4, 4, p, 2, None) == ARG
    assert L.tm_u8_shrink2(p, 4, 0, 4, p, 2, None) == ARG
    assert L.tm_u8_shrink2(p, 4, 5, 4, p, 3, None) == ARG and b"pitch" in L.tm_last_error()
    assert L.tm_u8_shrink2(p, 4, 5, 5, p, 2, None) == ARG and b"pitch" in L.tm_last_error()
    # tm_jpeg_encode_tiles(plane, H, W, pitch, quality, tile0, ntiles, slots, slot_bytes, need, packed, offsets, stream)
    enc = L.tm_jpeg_encode_tiles
    assert enc(None, 8, 8, 8, 75, 0, 1, p, 64, p, None, None, None) == ARG and b"null" in L.tm_last_error()
    assert enc(p, 8, 8, 8, 75, 0, 1, None, 64, p, None, None, None) == ARG
    assert enc(p, 8, 8, 8, 75, 0, 1, p, 64, None, None, None, None) == ARG
    assert enc(p, 8, 8, 8, 75, 0, 1, p, 64, p, p, None, None) == ARG and b"both" in L.tm_last_error()
    assert enc(p, 0, 8, 8, 75, 0, 1, p, 64, p, None, None, None) == ARG
    assert enc(p, 8, 0, 8, 75, 0, 1, p, 64, p, None, None, None) == ARG
    assert enc(p, 8, 8, 7, 75, 0, 1, p, 64, p, None, None, None) == ARG and b"pitch" in L.tm_last_error()
    assert enc(p, 8, 8, 8, 0, 0, 1, p, 64, p, None, None, None) == ARG and b"quality" in L.tm_last_error()
    assert enc(p, 8, 8, 8, 101, 0, 1, p, 64, p, None, None, None) == ARG
    assert enc(p, 8, 8, 8, 75, 1, 1, p, 64, p, None, None, None) == ARG and b"grid" in L.tm_last_error()
    assert enc(p, 8, 8, 8, 75, -1, 1, p, 64, p, None, None, None) == ARG
    assert enc(p, 8, 8, 8, 75, 0, 0, p, 64, p, None, None, None) == ARG
    assert enc(p, 264, 520, 520, 75, 4, 3, p, 64, p, None, None, None) == ARG and b"grid" in L.tm_last_error()
    assert enc(p, 8, 8, 8, 75, 0, 1, p, 0, p, None, None, None) == ARG and b"slot_bytes" in L.tm_last_error()
