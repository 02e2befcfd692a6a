"""-m gpu: stitch.save_composites_pyramid end to end: the colour files it writes from a resident two-stain state are
byte-identical to the ones the container writer builds from the numpy restatement's tiles (jpeg_rgb_cases.py), Pillow reads
every level back as RGB, and the quicklook JPEG is the level's composite."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

import jpeg_cases as jc
import jpeg_rgb_cases as rc
from teramind_amd import ometiff, stitch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, SLC, Q = 264, 520, 2, 75


def shrink2_ref(a):
    h, w = a.shape
    ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    b = a[np.ix_(ys, xs)].astype(np.int32)
    return ((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid_ref(a):
    out = [a]
    for _ in ometiff.pyramid_sizes(*a.shape)[1:]:
        out.append(shrink2_ref(out[-1]))
    return out


def host_file(path, polyt, dapi, quality=Q, **kw):
    """The file from restatement tiles: each stain's own pyramid, every level composed (R = 0, G = PolyT, B = DAPI) with the
    settings applied at that level.  Returns the levels' composites."""
    pg, pb = pyramid_ref(polyt), pyramid_ref(dapi)
    levels = [rc.compose((None, g, b), **kw) for g, b in zip(pg, pb)]

    def tiles(lv, h, w):
        gy, gx = jc.grid_of(h, w)
        for ty in range(gy):
            for tx in range(gx):
                yield ometiff.jpeg_tile_stream_rgb(rc.encode_tile(rc.tile_of(levels[lv], ty, tx), quality))
    ometiff.write_tiles(path, polyt.shape[0], polyt.shape[1], tiles, "jpeg", ometiff.jpeg_tables_rgb(quality), samples=3)
    return levels


@pytest.fixture(scope="module")
def state():
    """[(c s), H, W] with c = 2 stains, s = 2 slices: smooth fields in [-1, 1], a different one per plane, plus noise."""
    g = torch.Generator().manual_seed(5)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    planes = [0.6 * torch.sin(x / (20.0 + 7 * k)) * torch.cos(y / (31.0 - 3 * k)) + 0.1 * torch.randn(H, W, generator=g) for k in range(4)]
    return torch.stack(planes).clamp_(-1, 1).to(DEV)


@pytest.fixture(scope="module")
def planes(state):
    """stitch_state's uint8 '(s c)' planes on the host: the reference for every test here (not to be changed)."""
    a = stitch.stitch_state(state, SLC).cpu().numpy()
    a.setflags(write=False)
    return a


def same(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def test_files_equal_the_ones_built_from_restatement_tiles(tmp_path, state, planes):
    stitch.save_composites_pyramid(state, tmp_path / "g", slc=SLC, quality=Q, page=1)
    assert sorted(os.listdir(tmp_path / "g")) == ["rgb_0.jpg", "rgb_0.tif", "rgb_1.jpg", "rgb_1.tif"]
    for s in range(SLC):                     # '(s c)' planes of slice s: DAPI (c = 0) at 2 s, PolyT (c = 1) at 2 s + 1
        levels = host_file(tmp_path / f"h{s}.tif", planes[2 * s + 1], planes[2 * s])
        assert same(tmp_path / "g" / f"rgb_{s}.tif", tmp_path / f"h{s}.tif"), f"slice {s}"
        with Image.open(tmp_path / "g" / f"rgb_{s}.jpg") as im:
            assert im.mode == "RGB" and im.size == (260, 132)
            buf = io.BytesIO()
            Image.fromarray(levels[1], mode="RGB").save(buf, format="JPEG")
            assert np.array_equal(np.asarray(im), np.asarray(Image.open(buf)))              # level 1's composite, as Pillow writes it
    assert not np.array_equal(planes[1], planes[3])
    if features.check("libtiff"):
        with Image.open(tmp_path / "g" / "rgb_1.tif") as im:
            assert im.n_frames == 3
            for lv, (h, w) in enumerate(ometiff.pyramid_sizes(H, W)):
                im.seek(lv)
                assert im.mode == "RGB" and im.size == (w, h) and np.asarray(im).shape == (h, w, 3)


def test_slices_and_host_mosaic(tmp_path, state, planes):
    stitch.save_composites_pyramid(state, tmp_path / "a", slc=SLC, slices=[1], quality=Q)
    assert os.listdir(tmp_path / "a") == ["rgb_1.tif"]
    # the uint8 '(s c)' mosaic goes the same way and gives the same file
    stitch.save_composites_pyramid(np.array(planes), tmp_path / "b", slc=SLC, slices=[1], quality=Q)
    assert same(tmp_path / "a" / "rgb_1.tif", tmp_path / "b" / "rgb_1.tif")
    host_file(tmp_path / "h.tif", planes[3], planes[2])
    assert same(tmp_path / "a" / "rgb_1.tif", tmp_path / "h.tif")


@pytest.mark.parametrize("region", ["all", "quarter"])
def test_brightness_and_overlay_are_applied_at_every_level(tmp_path, state, planes, region):
    ov = rc.overlay_case()
    Image.fromarray(ov, mode="RGB").save(tmp_path / "onto.png")
    stitch.save_composites_pyramid(state, tmp_path / "g", slc=SLC, slices=[0], quality=Q, bright=2.0, overlay=tmp_path / "onto.png",
                                   alpha=100, region=region)
    host_file(tmp_path / "h.tif", planes[1], planes[0], bright=2.0, overlay=stitch.overlay_region(ov, region), alpha=100)
    assert same(tmp_path / "g" / "rgb_0.tif", tmp_path / "h.tif")
    if region == "all":                                            # the array form of the overlay gives the same file
        stitch.save_composites_pyramid(state, tmp_path / "a", slc=SLC, slices=[0], quality=Q, bright=2.0, overlay=ov, alpha=100)
        assert same(tmp_path / "a" / "rgb_0.tif", tmp_path / "h.tif")


def test_oversize_tile_is_encoded_again_with_a_sized_slot(tmp_path):
    """A batch slot smaller than the scan: write_pyramid_rgb takes the size from need and encodes the tile again; the file is
    the one a large slot gives, and the one built from restatement tiles."""
    g, b = rc.planes("noise3")[1:]
    dev = [torch.from_numpy(p.copy()).to(DEV) for p in (g, b)]
    ometiff.write_pyramid_rgb(tmp_path / "o.tif", (None, dev[0], dev[1]), quality=Q, slot_bytes=16384, batch_tiles=4)
    ometiff.write_pyramid_rgb(tmp_path / "l.tif", (None, dev[0], dev[1]), quality=Q, batch_tiles=4)
    host_file(tmp_path / "h.tif", g, b)
    assert same(tmp_path / "o.tif", tmp_path / "l.tif") and same(tmp_path / "o.tif", tmp_path / "h.tif")


def test_one_stain_state_raises_and_says_why(tmp_path, state):
    with pytest.raises(ValueError, match="two stains"):
        stitch.save_composites_pyramid(state[:2], tmp_path / "x", slc=SLC)
    with pytest.raises(ValueError, match="region"):
        stitch.save_composites_pyramid(state, tmp_path / "x", slc=SLC, region="left")
    with pytest.raises(ValueError, match="samples"):
        ometiff.write_tiles(tmp_path / "x.tif", 8, 8, lambda lv, h, w: [], "none", None, samples=3)
