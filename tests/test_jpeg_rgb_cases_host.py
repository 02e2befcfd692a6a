"""CPU: the numpy restatement of the colour composite and its 4:4:4 JPEG (jpeg_rgb_cases.py) against libjpeg through Pillow,
byte for byte; the colour tables datastream and tile stream of the library; the colour BigTIFF pages read back by libtiff; the
compose rules on hand-computed pixels; the argument checks of the three colour entry points (before any device call)."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image, ImageEnhance, features

import jpeg_cases as jc
import jpeg_rgb_cases as rc
from teramind_amd import _lib, ometiff, stitch


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


def _pillow(rgb, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb), mode="RGB").save(buf, format="JPEG", quality=quality, subsampling=0)
    return buf.getvalue()


@pytest.mark.parametrize("quality", rc.QUALITIES)
@pytest.mark.parametrize("name", list(rc.FULL_CASES))
def test_restatement_equals_libjpeg(name, quality):
    _, scan = _segments(_pillow(rc.image(name), quality))
    ours, = rc.reference_scans(name, quality)
    assert ours == scan


def test_noise_at_quality_100_outgrows_three_grey_slots():
    assert len(rc.reference_scans("noise3", 100)[0]) > 3 * ometiff.SLOT_BYTES      # the oversize path of the default slot is reachable


@pytest.mark.parametrize("quality", rc.QUALITIES + (50, 49))
def test_tables_datastream_equals_pillows(quality):
    segs, _ = _segments(_pillow(rc.image("stains"), quality))
    want = [(m, p) for m, p in segs if m in (0xDB, 0xC4)]
    ours, rest = _segments(ometiff.jpeg_tables_rgb(quality))
    assert rest == b"" and ours == want
    assert [(m, p[0]) for m, p in ours] == [(0xDB, 0), (0xDB, 1), (0xC4, 0x00), (0xC4, 0x10), (0xC4, 0x01), (0xC4, 0x11)]
    # and they are the tables of the restatement
    assert ours[0][1][1:] == bytes(rc.quant_table(quality, False)[jc.ZIGZAG].tolist())
    assert ours[1][1][1:] == bytes(rc.quant_table(quality, True)[jc.ZIGZAG].tolist())
    assert ours[4][1][1:] == bytes(rc.DC_BITS_C + jc.DC_VALS)
    assert ours[5][1][1:] == bytes(rc.AC_BITS_C + rc.AC_VALS_C)
    # the grey datastream is what it was
    assert len(ometiff.jpeg_tables(quality)) == 289


def test_tile_stream_has_pillows_frame_and_scan_headers():
    segs, _ = _segments(_pillow(rc.image("stains"), 75))
    ours, _ = _segments(ometiff.jpeg_tile_stream_rgb(b"\x00"))
    assert ours == [(m, p) for m, p in segs if m in (0xC0, 0xDA)]


@pytest.mark.parametrize("name", ["stains", "rnone"])
def test_tile_stream_decodes_with_the_tables(name):
    """tables + abbreviated stream are one valid JPEG: Pillow decodes the merged datastream to libjpeg's own decode."""
    q = 75
    tables, stream = ometiff.jpeg_tables_rgb(q), ometiff.jpeg_tile_stream_rgb(rc.reference_scans(name, q)[0])
    im = Image.open(io.BytesIO(tables[:-2] + stream[2:]))
    want = Image.open(io.BytesIO(_pillow(rc.image(name), q)))
    got, want = np.asarray(im.convert("RGB")), np.asarray(want.convert("RGB"))
    assert got.shape == (256, 256, 3) and np.array_equal(got, want)


# ---- the composite -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 0.5, 1.3, 2, 2.7])
def test_brightness_formula_is_pillows(f):
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = np.asarray(ImageEnhance.Brightness(Image.fromarray(np.stack([v, v, v], -1), mode="RGB")).enhance(f))[..., 0]
    assert np.array_equal(rc.brighten(v, f), want)
    assert np.array_equal(rc.compose((v, None, v), bright=f)[..., 2], want)
    assert not rc.compose((v, None, v), bright=f)[..., 1].any()


def test_overlay_rule_on_hand_computed_pixels():
    """H x W = 5 x 7 under a 2 x 3 overlay: rows 0 .. 2 take overlay row 0 ((y 2) // 5), rows 3, 4 row 1; columns 0 .. 2 take
    overlay column 0 ((x 3) // 7), 3, 4 column 1, 5, 6 column 2."""
    g = np.full((5, 7), 100, dtype=np.uint8)
    b = np.full((5, 7), 255, dtype=np.uint8)
    ov = np.zeros((2, 3, 3), dtype=np.uint8)
    ov[0, 0] = (255, 0, 0)
    ov[0, 2] = (0, 0, 1)
    ov[1, 1] = (10, 20, 30)
    out = rc.compose((None, g, b), overlay=ov, alpha=100)
    plain = (0, 100, 255)
    assert tuple(out[4, 0]) == plain and tuple(out[0, 3]) == plain and tuple(out[3, 6]) == plain      # black overlay: untouched
    # (ov 100 + v 155 + 127) // 255
    assert tuple(out[0, 0]) == tuple(out[2, 2]) == ((25500 + 127) // 255, (15500 + 127) // 255, (39525 + 127) // 255) == (100, 61, 155)
    assert tuple(out[1, 5]) == ((0 + 127) // 255, (15500 + 127) // 255, (100 + 39525 + 127) // 255) == (0, 61, 155)
    assert tuple(out[3, 3]) == tuple(out[4, 4]) == ((1000 + 127) // 255, (2000 + 15500 + 127) // 255, (3000 + 39525 + 127) // 255)
    assert (out[:3, :3] == out[0, 0]).all() and (out[3:, 3:5] == out[3, 3]).all()
    # alpha 0 leaves the image, alpha 255 puts the overlay where it is not black
    assert np.array_equal(rc.compose((None, g, b), overlay=ov, alpha=0), rc.compose((None, g, b)))
    full = rc.compose((None, g, b), overlay=ov, alpha=255)
    assert tuple(full[0, 0]) == (255, 0, 0) and tuple(full[4, 3]) == (10, 20, 30) and tuple(full[0, 6]) == (0, 0, 1)
    assert tuple(full[4, 0]) == plain
    # brightness comes first: the blend sees the brightened pixel
    out2 = rc.compose((None, g, b), bright=2, overlay=ov, alpha=100)
    assert tuple(out2[0, 0]) == ((25500 + 127) // 255, (200 * 155 + 127) // 255, (255 * 155 + 127) // 255)
    assert tuple(out2[4, 0]) == (0, 200, 255)


def test_every_region_keeps_its_part_of_the_overlay():
    ov = np.arange(1, 1 + 5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    keep = {"all": np.ones((5, 7), bool), "half": np.zeros((5, 7), bool), "rhalf": np.zeros((5, 7), bool),
            "thalf": np.zeros((5, 7), bool), "bhalf": np.zeros((5, 7), bool), "quarter": np.zeros((5, 7), bool),
            "3quarter": np.ones((5, 7), bool)}
    keep["half"][:, :3] = True
    keep["rhalf"][:, 3:] = True
    keep["thalf"][:2] = True
    keep["bhalf"][2:] = True
    keep["quarter"][:2, :3] = True
    keep["3quarter"][:2, 3:] = False
    assert set(keep) == set(stitch.REGIONS)
    for region, m in keep.items():
        got = stitch.overlay_region(ov, region)
        assert np.array_equal(got, ov * m[:, :, None]), region
    assert np.array_equal(ov, np.arange(1, 1 + 5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3))          # the input is not written
    with pytest.raises(ValueError, match="region"):
        stitch.overlay_region(ov, "left")
    with pytest.raises(ValueError, match="uint8"):
        stitch.overlay_region(ov.astype(np.float32), "all")


# ---- the container -----------------------------------------------------------------------------------------------------
def test_rgb_bigtiff_of_restatement_tiles_opens_as_rgb(tmp_path):
    if not features.check("libtiff"):
        pytest.fail("Pillow without libtiff cannot read the pages back")
    q = 75
    top = np.ascontiguousarray(rc.image("p264x520")[:, :500])      # 264 x 500: two levels, 2 x 2 tiles and one
    half = np.ascontiguousarray(top[::2, ::2])                     # any 132 x 250 image serves as the second level
    levels = [top, half]
    decoded = {}

    def tiles(lv, h, w):
        assert (h, w) == levels[lv].shape[:2]
        gy, gx = jc.grid_of(h, w)
        for ty in range(gy):
            for tx in range(gx):
                scan = rc.encode_tile(rc.tile_of(levels[lv], ty, tx), q)
                merged = ometiff.jpeg_tables_rgb(q)[:-2] + ometiff.jpeg_tile_stream_rgb(scan)[2:]
                decoded[lv, ty, tx] = np.asarray(Image.open(io.BytesIO(merged)).convert("RGB"))
                yield ometiff.jpeg_tile_stream_rgb(scan)
    ometiff.write_tiles(tmp_path / "c.tif", 264, 500, tiles, "jpeg", ometiff.jpeg_tables_rgb(q), samples=3)
    assert len(decoded) == 5
    with Image.open(tmp_path / "c.tif") as im:
        assert im.n_frames == 2
        for lv, (h, w) in enumerate([(264, 500), (132, 250)]):
            im.seek(lv)
            assert im.mode == "RGB" and im.size == (w, h)
            got = np.asarray(im)
            assert got.shape == (h, w, 3)
            for (l, ty, tx), t in decoded.items():
                if l == lv:
                    part = got[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
                    assert np.array_equal(part, t[:part.shape[0], :part.shape[1]]), (lv, ty, tx)
    data = open(tmp_path / "c.tif", "rb").read()
    assert b'SizeC="3"' in data and b'<Channel ID="Channel:0:0" SamplesPerPixel="3"/>' in data


def test_colour_pages_are_jpeg_only_and_grey_pages_are_unchanged(tmp_path):
    with pytest.raises(ValueError, match="samples"):
        ometiff.write_tiles(tmp_path / "x.tif", 8, 8, lambda lv, h, w: [b"\0" * 65536 * 3], "none", None, samples=3)
    with pytest.raises(ValueError, match="samples"):
        ometiff.write_tiles(tmp_path / "x.tif", 8, 8, lambda lv, h, w: [b""], "jpeg", b"t", samples=2)
    # samples = 1 is the default: the same bytes either way
    t = ometiff.jpeg_tile_stream(jc.reference_scans("p8x8", 75)[0])
    ometiff.write_tiles(tmp_path / "a.tif", 8, 8, lambda lv, h, w: [t], "jpeg", ometiff.jpeg_tables(75))
    ometiff.write_tiles(tmp_path / "b.tif", 8, 8, lambda lv, h, w: [t], "jpeg", ometiff.jpeg_tables(75), samples=1)
    assert open(tmp_path / "a.tif", "rb").read() == open(tmp_path / "b.tif", "rb").read()
    assert b'SizeC="1"' in open(tmp_path / "a.tif", "rb").read() and b"Channel" not in open(tmp_path / "a.tif", "rb").read()


# ---- argument checks ---------------------------------------------------------------------------------------------------
def test_argument_checks_without_device():
    L = _lib.lib()
    buf = (C.c_uint8 * 1024)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_size_t(0)
    ARG = -1
    # tm_jpeg_tables_rgb
    assert L.tm_jpeg_tables_rgb(0, p, 1024, C.byref(n)) == ARG and b"quality" in L.tm_last_error()
    assert L.tm_jpeg_tables_rgb(101, p, 1024, C.byref(n)) == ARG
    assert L.tm_jpeg_tables_rgb(75, None, 0, None) == ARG and b"null" in L.tm_last_error()
    size = 2 + 2 * 69 + 2 * 33 + 2 * 183 + 2
    assert L.tm_jpeg_tables_rgb(75, p, 100, C.byref(n)) == ARG and n.value == size and b"buffer" in L.tm_last_error()
    assert L.tm_jpeg_tables_rgb(75, None, 0, C.byref(n)) == 0 and n.value == size

    def src(planes=(None, p, p), pitches=(0, 8, 8)):
        return (C.c_void_p * 3)(*planes), (C.c_int64 * 3)(*pitches)

    ok, pit = src()
    # tm_jpeg_encode_tiles_rgb(planes, pitches, H, W, bright, overlay, oh, ow, alpha, quality, tile0, ntiles, slots,
    #                          slot_bytes, need, packed, offsets, stream)
    enc = L.tm_jpeg_encode_tiles_rgb
    tail = (75, 0, 1, p, 64, p, None, None, None)
    assert enc(None, pit, 8, 8, 1.0, None, 0, 0, 0, *tail) == ARG and b"null" in L.tm_last_error()
    assert enc(ok, None, 8, 8, 1.0, None, 0, 0, 0, *tail) == ARG and b"null" in L.tm_last_error()
    assert enc(src((None, None, None))[0], pit, 8, 8, 1.0, None, 0, 0, 0, *tail) == ARG and b"all three" in L.tm_last_error()
    assert enc(ok, pit, 0, 8, 1.0, None, 0, 0, 0, *tail) == ARG
    assert enc(ok, pit, 8, 0, 1.0, None, 0, 0, 0, *tail) == ARG and b"positive" in L.tm_last_error()
    assert enc(ok, src(pitches=(0, 8, 7))[1], 8, 8, 1.0, None, 0, 0, 0, *tail) == ARG and b"pitch" in L.tm_last_error()
    assert enc(ok, src(pitches=(0, 7, 8))[1], 8, 8, 1.0, None, 0, 0, 0, *tail) == ARG and b"pitch" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, -0.5, None, 0, 0, 0, *tail) == ARG and b"bright" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, float("nan"), None, 0, 0, 0, *tail) == ARG and b"bright" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, float("inf"), None, 0, 0, 0, *tail) == ARG and b"bright" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, p, 0, 4, 100, *tail) == ARG and b"overlay" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, p, 4, 0, 100, *tail) == ARG and b"overlay" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, p, 4, 4, -1, *tail) == ARG and b"alpha" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, p, 4, 4, 256, *tail) == ARG and b"alpha" in L.tm_last_error()
    big = src(pitches=(0, 70000, 70000))[1]
    assert enc(ok, big, 8, 70000, 1.0, p, 4, 40000, 100, *tail) == ARG and b"2^31" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 0, 1, None, 64, p, None, None, None) == ARG and b"null" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 0, 1, p, 64, None, None, None, None) == ARG
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 0, 1, p, 64, p, p, None, None) == ARG and b"both" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 0, 1, p, 64, p, None, p, None) == ARG
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 0, 0, 1, p, 64, p, None, None, None) == ARG and b"quality" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 101, 0, 1, p, 64, p, None, None, None) == ARG
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 1, 1, p, 64, p, None, None, None) == ARG and b"grid" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, -1, 1, p, 64, p, None, None, None) == ARG
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 0, 0, p, 64, p, None, None, None) == ARG
    wide = src(pitches=(0, 520, 520))[1]
    assert enc(ok, wide, 264, 520, 1.0, None, 0, 0, 0, 75, 4, 3, p, 64, p, None, None, None) == ARG and b"grid" in L.tm_last_error()
    assert enc(ok, pit, 8, 8, 1.0, None, 0, 0, 0, 75, 0, 1, p, 0, p, None, None, None) == ARG and b"slot_bytes" in L.tm_last_error()
    # tm_rgb_compose(planes, pitches, H, W, bright, overlay, oh, ow, alpha, dst, dst_pitch, stream)
    cmp_ = L.tm_rgb_compose
    assert cmp_(None, pit, 8, 8, 1.0, None, 0, 0, 0, p, 24, None) == ARG and b"null" in L.tm_last_error()
    assert cmp_(src((None, None, None))[0], pit, 8, 8, 1.0, None, 0, 0, 0, p, 24, None) == ARG and b"all three" in L.tm_last_error()
    assert cmp_(ok, pit, 8, 0, 1.0, None, 0, 0, 0, p, 24, None) == ARG
    assert cmp_(ok, src(pitches=(0, 8, 7))[1], 8, 8, 1.0, None, 0, 0, 0, p, 24, None) == ARG and b"pitch" in L.tm_last_error()
    assert cmp_(ok, pit, 8, 8, -1.0, None, 0, 0, 0, p, 24, None) == ARG and b"bright" in L.tm_last_error()
    assert cmp_(ok, pit, 8, 8, 1.0, p, 4, 4, 300, p, 24, None) == ARG and b"alpha" in L.tm_last_error()
    assert cmp_(ok, pit, 8, 8, 1.0, p, 0, 4, 100, p, 24, None) == ARG and b"overlay" in L.tm_last_error()
    assert cmp_(ok, pit, 8, 8, 1.0, None, 0, 0, 0, None, 24, None) == ARG and b"destination" in L.tm_last_error()
    assert cmp_(ok, pit, 8, 8, 1.0, None, 0, 0, 0, p, 23, None) == ARG and b"pitch" in L.tm_last_error()
