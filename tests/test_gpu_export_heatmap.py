"""-m gpu: stitch.save_attn_heatmaps_pyramid end to end.  The colour pyramids it writes from an attention mosaic are
byte-identical to the ones the container writer builds on the host from the GPU's own field pushed through the numpy render
restatement (heatmap_cases.render_ref), 2 x 2 reductions and restatement JPEG tiles (jpeg_rgb_cases), the scheme of
test_gpu_export_rgb.py; Pillow reads every level back as RGB; the `under=` file is the restatement's PolyT / DAPI composite with
the heat map blended over it; tools/run_attn_roi.py writes what it wrote before unless --heatmap is given."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image, features

import heatmap_cases as hc
import jpeg_cases as jc
import jpeg_rgb_cases as rc
from teramind_amd import formats, heatmap, ometiff, stitch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, VMAX, SCALE, Q = 2, 2.0, 4, 90
SLC, UH, UW = 2, 200, 330                      # the two-stain state under the map: its own size, one level below it


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


def host_file(path, planes, quality=Q, **kw):
    """The file from restatement tiles: each given plane's own pyramid, every level composed with the settings applied at that
    level.  Returns the levels' composites."""
    pyr = [None if p is None else pyramid_ref(p) for p in planes]
    n = len(next(p for p in pyr if p is not None))
    levels = [rc.compose(tuple(None if p is None else p[lv] for p in pyr), **kw) for lv in range(n)]
    H, W = levels[0].shape[:2]

    def tiles(lv, h, w):
        gy, gx = jc.grid_of(h, w)
        for ty in range(gy):
            for tx in range(gx):
                yield ometiff.jpeg_tile_stream_rgb(rc.encode_tile(rc.tile_of(levels[lv], ty, tx), quality))
    ometiff.write_tiles(path, H, W, tiles, "jpeg", ometiff.jpeg_tables_rgb(quality), samples=3)
    return levels


def same(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def mosaic():
    return torch.from_numpy(np.array(hc.export_mosaic())).to(DEV)


@pytest.fixture(scope="module")
def gpu_fields(mosaic):
    """The GPU's own att_all field of each slice, on the host (shared; not to be changed); held to the float64 model here."""
    out = []
    for s in range(mosaic.shape[0]):
        f = heatmap.field(mosaic[s], K, "att_all", hc.WEI, 2.0).cpu().numpy()
        sum0, nsum, mask0, nmask = hc.mode_ranges(K, "att_all")
        taps = hc.gaussian_taps(2.0)[1]
        src = hc.export_mosaic()[s]
        assert np.abs(f - hc.field_model(src, sum0, nsum, hc.WEI, mask0, nmask, taps)).max() <= hc.field_bound(src, sum0, nsum, hc.WEI, mask0, nmask, taps)
        f.setflags(write=False)
        out.append(f)
    return out


def test_files_equal_the_ones_built_from_the_restatement(tmp_path, mosaic, gpu_fields):
    stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "g", K, vmax=VMAX, wei=hc.WEI, scale=SCALE, quality=Q, page=1)
    assert sorted(os.listdir(tmp_path / "g")) == ["heat_att_all_0.jpg", "heat_att_all_0.tif", "heat_att_all_1.jpg", "heat_att_all_1.tif"]
    H, W = hc.EXPORT_SHAPE[2] * SCALE, hc.EXPORT_SHAPE[3] * SCALE
    sizes = ometiff.pyramid_sizes(H, W)
    assert len(sizes) == 2
    for s in range(2):
        img = hc.render_ref(gpu_fields[s], heatmap.INFERNO, 0.0, VMAX, SCALE, floor=1)
        assert img.shape == (H, W, 3) and len(np.unique(img.reshape(-1, 3), axis=0)) > 50, "the map has structure"
        levels = host_file(tmp_path / f"h{s}.tif", [np.ascontiguousarray(img[..., c]) for c in range(3)])
        assert same(tmp_path / "g" / f"heat_att_all_{s}.tif", tmp_path / f"h{s}.tif"), f"slice {s}"
        with Image.open(tmp_path / "g" / f"heat_att_all_{s}.jpg") as im:
            assert im.mode == "RGB" and im.size == (sizes[1][1], sizes[1][0])
            buf = io.BytesIO()
            Image.fromarray(levels[1], mode="RGB").save(buf, format="JPEG")
            assert np.array_equal(np.asarray(im), np.asarray(Image.open(buf)))
        if features.check("libtiff"):
            with Image.open(tmp_path / "g" / f"heat_att_all_{s}.tif") as im:
                assert im.n_frames == len(sizes)
                for lv, (h, w) in enumerate(sizes):
                    im.seek(lv)
                    assert im.mode == "RGB" and im.size == (w, h) and np.asarray(im).shape == (h, w, 3)
    assert not np.array_equal(gpu_fields[0], gpu_fields[1])


def test_host_mosaic_slices_palette_and_pathway_defaults(tmp_path, mosaic, gpu_fields):
    stitch.save_attn_heatmaps_pyramid(np.array(hc.export_mosaic()), tmp_path / "a", K, slices=[1], path="GLUT", wei=hc.WEI, scale=SCALE, quality=Q)
    assert os.listdir(tmp_path / "a") == ["heat_att_all_1.tif"]               # vmax from PATHWAY_VMAX['GLUT']['att_all'] = 2
    img = hc.render_ref(gpu_fields[1], heatmap.INFERNO, 0.0, VMAX, SCALE, floor=1)
    host_file(tmp_path / "h.tif", [np.ascontiguousarray(img[..., c]) for c in range(3)])
    assert same(tmp_path / "a" / "heat_att_all_1.tif", tmp_path / "h.tif")
    # expr of gene 1 through the pathway's two-colour palette and scale, at scale 2 and floor 0
    stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "e", K, mode="expr", gene=1, slices=[0], path="GLUT", scale=2, quality=Q, floor=0)
    assert os.listdir(tmp_path / "e") == ["heat_expr_0.tif"]
    f = heatmap.field(mosaic[0], K, "expr", gene=1).cpu().numpy()
    lut = hc.two_colour(heatmap.PATHWAY_COLOURS["GLUT"][1])
    img = hc.render_ref(f, lut, 0.0, heatmap.PATHWAY_VMAX["GLUT"]["expr"][1], 2, floor=0)
    host_file(tmp_path / "he.tif", [np.ascontiguousarray(img[..., c]) for c in range(3)])
    assert same(tmp_path / "e" / "heat_expr_0.tif", tmp_path / "he.tif")
    with pytest.raises(ValueError, match="vmax"):
        stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "x", K, mode="att_up")
    with pytest.raises(ValueError, match="4K"):
        stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "x", 3, vmax=2.0)


def test_map_over_the_two_stain_composite(tmp_path, mosaic, gpu_fields):
    g = torch.Generator().manual_seed(9)
    y, x = torch.meshgrid(torch.arange(UH, dtype=torch.float32), torch.arange(UW, dtype=torch.float32), indexing="ij")
    state = torch.stack([0.6 * torch.sin(x / (20.0 + 7 * k)) * torch.cos(y / (31.0 - 3 * k)) + 0.1 * torch.randn(UH, UW, generator=g)
                         for k in range(2 * SLC)]).clamp_(-1, 1).to(DEV)
    planes = stitch.stitch_state(state, SLC).cpu().numpy()                     # '(s c)': DAPI (c = 0) at 2 s, PolyT (c = 1) at 2 s + 1
    stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "g", K, vmax=VMAX, wei=hc.WEI, scale=SCALE, quality=Q, under=state, slc=SLC,
                                      alpha=160, slices=[1], page=0)
    assert sorted(os.listdir(tmp_path / "g")) == ["heat_over_att_all_1.jpg", "heat_over_att_all_1.tif"]
    ov = hc.render_ref(gpu_fields[1], heatmap.INFERNO, 0.0, VMAX, SCALE, floor=1)
    assert (ov == 0).all(-1).any() and (ov != 0).any(-1).any(), "the floor leaves transparent cells and painted ones"
    levels = host_file(tmp_path / "h.tif", (None, planes[3], planes[2]), overlay=ov, alpha=160)
    assert same(tmp_path / "g" / "heat_over_att_all_1.tif", tmp_path / "h.tif")
    plain = rc.compose((None, planes[3], planes[2]))
    assert (levels[0] != plain).any() and (levels[0] == plain).all(-1).any()
    with Image.open(tmp_path / "g" / "heat_over_att_all_1.jpg") as im:
        assert im.mode == "RGB" and im.size == (UW, UH)
    # the uint8 '(s c)' mosaic under it gives the same file
    stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "b", K, vmax=VMAX, wei=hc.WEI, scale=SCALE, quality=Q, under=np.array(planes),
                                      slc=SLC, alpha=160, slices=[1])
    assert same(tmp_path / "b" / "heat_over_att_all_1.tif", tmp_path / "h.tif")
    with pytest.raises(ValueError, match="two stains"):
        stitch.save_attn_heatmaps_pyramid(mosaic, tmp_path / "x", K, vmax=VMAX, under=state[:2], slc=SLC)


def _run_tool(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_attn_roi.py"), "--synthetic", "--hnm", "1", "--wnm", "2", "--out_dir", str(out_dir),
           *extra]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_tool_writes_pyramids_with_the_flag_and_what_it_wrote_before_without(tmp_path):
    plain = _run_tool(tmp_path / "p")
    heat = _run_tool(tmp_path / "h", "--heatmap", "att_all", "--heat_scale", "2")
    before = {"what", "tiles", "rank0_tiles", "n_gpus", "glst", "fused", "batch_tiles", "genes", "prefetched", "tile_files_written", "seconds",
              "rank0_sweep_s", "tiles_per_s", "bytes_written_rank0", "stitch_s", "mosaic_shape", "out_dir"}
    assert set(plain) == before and set(heat) == before | {"heatmap", "heatmap_s", "heatmap_files"}
    assert sorted(os.listdir(tmp_path / "p")) == ["attn_GLUT", "attn_GLUT_all"]
    assert sorted(os.listdir(tmp_path / "h")) == ["attn_GLUT", "attn_GLUT_all", "heat_GLUT_att_all"]
    for sub in ("attn_GLUT", "attn_GLUT_all"):                                 # the files of before
        names = sorted(os.listdir(tmp_path / "p" / sub))
        assert names == sorted(os.listdir(tmp_path / "h" / sub)) and names
        for n in names:
            if sub == "attn_GLUT":                                             # tile files carry a fixed date: byte for byte
                assert same(tmp_path / "p" / sub / n, tmp_path / "h" / sub / n), n
            else:                                                              # save_attn_slices stamps the wall clock: the arrays
                a, b = (formats.read_zarr_zip(tmp_path / d / sub / n) for d in ("p", "h"))
                assert a.dtype == b.dtype == np.float16 and np.array_equal(a, b), n
    S, C4, H, W = heat["mosaic_shape"]
    files = sorted(os.listdir(tmp_path / "h" / "heat_GLUT_att_all"))
    assert heat["heatmap_files"] == len(files) == S and files[0] == "heat_att_all_0.tif"
    for n in files[:3]:
        with Image.open(tmp_path / "h" / "heat_GLUT_att_all" / n) as im:
            assert im.mode == "RGB" and im.size == (2 * W, 2 * H)
            if features.check("libtiff"):
                assert np.asarray(im).shape == (2 * H, 2 * W, 3)
