"""-m gpu: stitch.save_slices_pyramid end to end: the files it writes from a resident state are byte-identical to the ones
the container writer builds from the numpy restatement's tiles, and Pillow reads every level back."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

import jpeg_cases as jc
from teramind_amd import ometiff, stitch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, SLC, Q = 600, 520, 2, 75


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


def host_file(path, a, compression):
    levels = pyramid_ref(a)

    def tiles(lv, h, w):
        gy, gx = jc.grid_of(h, w)
        for ty in range(gy):
            for tx in range(gx):
                t = jc.tile_of(levels[lv], ty, tx)
                yield t.tobytes() if compression == "none" else ometiff.jpeg_tile_stream(jc.encode_tile(t, Q))
    ometiff.write_tiles(path, a.shape[0], a.shape[1], tiles, compression, ometiff.jpeg_tables(Q) if compression == "jpeg" else None)
    return levels


@pytest.fixture(scope="module")
def state():
    """[(c s), H, W] with c = 2 stains, s = 2 slices: smooth fields in [-1, 1], a different one per plane, plus noise."""
    g = torch.Generator().manual_seed(3)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    planes = [0.6 * torch.sin(x / (20.0 + 7 * k)) * torch.cos(y / (31.0 - 3 * k)) + 0.1 * torch.randn(H, W, generator=g) for k in range(4)]
    return torch.stack(planes).clamp_(-1, 1).to(DEV)


@pytest.fixture(scope="module")
def planes(state):
    """stitch_state's uint8 '(s c)' planes on the host: the reference for every test here (not to be changed)."""
    a = stitch.stitch_state(state, SLC).cpu().numpy()
    a.setflags(write=False)
    return a


def test_files_equal_the_ones_built_from_restatement_tiles(tmp_path, state, planes):
    stitch.save_slices_pyramid(state, tmp_path / "g", slc=SLC, quality=Q, page=1)
    assert sorted(os.listdir(tmp_path / "g")) == sorted([f"all_{k}.tif" for k in range(4)] + [f"all_{k}.jpg" for k in range(4)])
    for k in range(4):                       # plane k of '(s c)': slice k // 2, stain k % 2
        levels = host_file(tmp_path / f"h{k}.tif", planes[k], "jpeg")
        assert open(tmp_path / "g" / f"all_{k}.tif", "rb").read() == open(tmp_path / f"h{k}.tif", "rb").read(), f"plane {k}"
        with Image.open(tmp_path / "g" / f"all_{k}.jpg") as im:
            assert im.size == (260, 300)
            buf = io.BytesIO()
            Image.fromarray(levels[1], mode="L").save(buf, format="JPEG")
            assert np.array_equal(np.asarray(im), np.asarray(Image.open(buf)))              # level 1 of this plane, as Pillow writes it
    # '(s c)' order: file 1 is stain 1 of slice 0 = state plane c * SLC + s = 2, not state plane 1
    assert not np.array_equal(planes[1], planes[2])
    assert np.array_equal(planes[1], stitch.to_uint8(state[2]).cpu().numpy())
    if features.check("libtiff"):
        with Image.open(tmp_path / "g" / "all_3.tif") as im:
            assert im.n_frames == 3
            for lv, (h, w) in enumerate(ometiff.pyramid_sizes(H, W)):
                im.seek(lv)
                assert im.size == (w, h) and np.asarray(im).shape == (h, w)


def test_slices_names_and_host_mosaic(tmp_path, state, planes):
    stitch.save_slices_pyramid(state, tmp_path / "a", slc=SLC, slices=[1, 2], names=[10, 20], quality=Q)
    assert sorted(os.listdir(tmp_path / "a")) == ["all_10.tif", "all_20.tif"]
    # the uint8 mosaic stitch_dir returns goes the same way and gives the same files
    stitch.save_slices_pyramid(np.array(planes), tmp_path / "b", slc=SLC, slices=[1, 2], names=[10, 20], quality=Q)
    for n in ("all_10.tif", "all_20.tif"):
        assert open(tmp_path / "a" / n, "rb").read() == open(tmp_path / "b" / n, "rb").read()
    host_file(tmp_path / "h.tif", planes[2], "jpeg")
    assert open(tmp_path / "a" / "all_20.tif", "rb").read() == open(tmp_path / "h.tif", "rb").read()


def test_uncompressed_file_decodes_to_the_pyramid_of_the_plane(tmp_path, state, planes):
    stitch.save_slices_pyramid(state, tmp_path / "n", slc=SLC, slices=[3], compression="none")
    want = pyramid_ref(planes[3])
    with Image.open(tmp_path / "n" / "all_3.tif") as im:
        assert im.n_frames == 3
        for lv in range(3):
            im.seek(lv)
            assert np.array_equal(np.asarray(im), want[lv])
    host_file(tmp_path / "h.tif", planes[3], "none")
    assert open(tmp_path / "n" / "all_3.tif", "rb").read() == open(tmp_path / "h.tif", "rb").read()


def test_oversize_tile_is_encoded_again_with_a_sized_slot(tmp_path):
    """A batch slot smaller than the scan: write_pyramid takes the size from need and encodes the tile again."""
    img = jc.image("noise")
    ometiff.write_pyramid(tmp_path / "o.tif", torch.from_numpy(img.copy()).to(DEV), quality=Q, slot_bytes=16384, batch_tiles=4)
    host_file(tmp_path / "h.tif", np.array(img), "jpeg")
    assert open(tmp_path / "o.tif", "rb").read() == open(tmp_path / "h.tif", "rb").read()
