"""CPU: the BigTIFF pyramid container of teramind_amd.ometiff around host-made tiles (raw, and JPEG scans of the numpy
restatement), read back through Pillow."""
import io
import struct
import xml.etree.ElementTree as ET

import numpy as np
import pytest
from PIL import Image, features

import jpeg_cases as jc
from teramind_amd import ometiff

H, W, Q = 600, 520, 75
needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="Pillow was built without libtiff: it cannot read JPEG-in-TIFF")


def shrink2(a):
    """The numpy 2 x 2 rule: (a + b + c + d + 2) >> 2, an odd last row / column repeated."""
    h, w = a.shape
    ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    b = a[np.ix_(ys, xs)].astype(np.int32)
    return ((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(a):
    out = [a]
    for _ in ometiff.pyramid_sizes(*a.shape)[1:]:
        out.append(shrink2(out[-1]))
    return out


@pytest.fixture(scope="module")
def plane():
    y, x = np.mgrid[0:H, 0:W]
    a = 127.5 + 70 * np.sin(x / 29.0) * np.cos(y / 41.0) + np.random.default_rng(5).normal(0, 12, (H, W))
    a = np.clip(a, 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


def libjpeg_roundtrip(a):
    """What a decoder must return for the level: every full tile through Pillow's own JPEG encode + decode at Q (the scans
    are libjpeg's bytes, so the decoded pixels are libjpeg's too), cropped to the level."""
    out = np.empty_like(a)
    gy, gx = jc.grid_of(*a.shape)
    for ty in range(gy):
        for tx in range(gx):
            buf = io.BytesIO()
            Image.fromarray(jc.tile_of(a, ty, tx), mode="L").save(buf, format="JPEG", quality=Q)
            t = np.asarray(Image.open(buf))
            y0, x0 = ty * 256, tx * 256
            out[y0:y0 + 256, x0:x0 + 256] = t[:a.shape[0] - y0, :a.shape[1] - x0]
    return out


def write_host(path, a, compression):
    """The file of `a` from host-made tiles: raw, or scans of the restatement."""
    levels = pyramid(a)

    def tiles(lv, h, w):
        assert levels[lv].shape == (h, w)
        gy, gx = jc.grid_of(h, w)
        for ty in range(gy):
            for tx in range(gx):
                t = jc.tile_of(levels[lv], ty, tx)
                yield t.tobytes() if compression == "none" else ometiff.jpeg_tile_stream(jc.encode_tile(t, Q))
    ometiff.write_tiles(path, a.shape[0], a.shape[1], tiles, compression, ometiff.jpeg_tables(Q) if compression == "jpeg" else None)
    return levels


def test_pyramid_sizes():
    assert ometiff.pyramid_sizes(600, 520) == [(600, 520), (300, 260), (150, 130)]
    assert ometiff.pyramid_sizes(256, 256) == [(256, 256)]
    assert ometiff.pyramid_sizes(257, 3) == [(257, 3), (129, 2)]
    whole = ometiff.pyramid_sizes(73216, 105984)
    assert whole[-1] == (143, 207) and len(whole) == 10


def test_uncompressed_pyramid_reads_back_bit_for_bit(tmp_path, plane):
    levels = write_host(tmp_path / "n.tif", plane, "none")
    raw = open(tmp_path / "n.tif", "rb").read()
    assert struct.unpack("<2sHHH", raw[:8]) == (b"II", 43, 8, 0)
    with Image.open(tmp_path / "n.tif") as im:
        assert im.n_frames == 3
        for lv, want in enumerate(levels):
            im.seek(lv)
            assert im.size == (want.shape[1], want.shape[0])
            assert im.tag_v2[254] == (1 if lv else 0) and im.tag_v2[259] == 1
            assert im.tag_v2[322] == 256 and im.tag_v2[323] == 256 and im.tag_v2[262] == 1
            assert (270 in im.tag_v2) == (lv == 0)
            assert np.array_equal(np.asarray(im), want)
    assert [lv.shape for lv in levels] == [(600, 520), (300, 260), (150, 130)]


@needs_libtiff
def test_jpeg_pyramid_reads_back(tmp_path, plane):
    levels = write_host(tmp_path / "j.tif", plane, "jpeg")
    with Image.open(tmp_path / "j.tif") as im:
        assert im.n_frames == 3
        for lv, want in enumerate(levels):
            im.seek(lv)
            assert im.size == (want.shape[1], want.shape[0])
            assert im.tag_v2[254] == (1 if lv else 0) and im.tag_v2[259] == 7
            assert np.array_equal(np.asarray(im), libjpeg_roundtrip(want))
    # same tiles, same bytes
    write_host(tmp_path / "j2.tif", plane, "jpeg")
    assert open(tmp_path / "j.tif", "rb").read() == open(tmp_path / "j2.tif", "rb").read()


def test_description_is_the_ome_xml(tmp_path, plane):
    write_host(tmp_path / "n.tif", plane, "none")
    with Image.open(tmp_path / "n.tif") as im:
        text = im.tag_v2[270]
    assert text == ometiff.ome_xml(W, H)
    root = ET.fromstring(text.encode())
    ns = {"o": "http://www.openmicroscopy.org/Schemas/OME/2016-06"}
    px = root.find("o:Image/o:Pixels", ns)
    assert px.get("SizeX") == str(W) and px.get("SizeY") == str(H) and px.get("SizeC") == "1" and px.get("Type") == "uint8"


def test_ifd_encoder_writes_offsets_above_4_gib_whole():
    big = (1 << 32) + 12345
    # one tile: the LONG8 offset sits in the entry itself
    ifd = ometiff.encode_ifd([(324, 16, [big]), (325, 16, [777])], (1 << 33) + 8, 0)
    assert struct.unpack("<Q", ifd[:8]) == (2,)
    tag, typ, cnt, val = struct.unpack("<HHQQ", ifd[8:28])
    assert (tag, typ, cnt, val) == (324, 16, 1, big)
    assert struct.unpack("<Q", ifd[48:56]) == (0,)
    # two tiles: the array goes behind the IFD, and the pointer to it (an offset above 2^33) is whole too
    at = (1 << 33) + 8
    ifd = ometiff.encode_ifd([(324, 16, [big, big + 5])], at, at + 4096)
    tag, typ, cnt, ptr = struct.unpack("<HHQQ", ifd[8:28])
    assert (tag, typ, cnt) == (324, 16, 2) and ptr == at + 8 + 20 + 8
    assert struct.unpack("<Q", ifd[28:36]) == (at + 4096,)
    assert struct.unpack("<2Q", ifd[36:52]) == (big, big + 5)


def test_write_tiles_rejects_a_wrong_tile_count(tmp_path):
    with pytest.raises(RuntimeError):
        ometiff.write_tiles(tmp_path / "x.tif", 300, 300, lambda lv, h, w: [b"\0" * 65536], "none")
    with pytest.raises(ValueError):
        ometiff.write_tiles(tmp_path / "x.tif", 300, 300, lambda lv, h, w: [], "jpeg")
