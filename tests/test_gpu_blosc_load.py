"""-m gpu: step directories read through the GPU Blosc decoder -- TileSweep.load_step(decoder="gpu") against the host route bit
for bit in both canvas layouts, the visible fall-back for zlib / raw tiles, a corrupt tile file, read_state_tile_dev,
stitch_dir(decoder="gpu"), and tools/run_roi.py --cur_epoch."""
import json
import os
import shutil
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch

import blosc_cases as bc
import blosc_decode_cases as dc
import util
from teramind_amd import formats, stitch, tiles
from teramind_amd.brain import PAD, TileSweep
from teramind_amd.config import PathConfig
from teramind_amd.diffusion import SpacedDiffusionBeatGans

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLC, T = 4, 3


def model_free_sweep(state, seed=11):
    """A 2 x 2-tile sweep without a model, its canvas seeded: half of every tile background, the rest noise."""
    sw = TileSweep(PathConfig(), SpacedDiffusionBeatGans(T, "ddim"), None, None, hst=512, wst=768, hnm=2, wnm=2, total_epochs=T, total_slc=SLC,
                   device=DEV, init="device", state=state)
    g = torch.Generator(device=DEV).manual_seed(seed)
    inner = torch.randn((sw.chn, 2 * tiles.TILE, 2 * tiles.TILE), generator=g, device=DEV)
    inner[:, :, 64:192] = -1.0
    inner[:, :, 300:420] = -1.0
    sw.cur[:, PAD:-PAD, PAD:-PAD].copy_(inner.half().to(sw.cur.dtype))
    sw.epoch = 2
    return sw


def fresh(state):
    return TileSweep(PathConfig(), SpacedDiffusionBeatGans(T, "ddim"), None, None, hst=512, wst=768, hnm=2, wnm=2, total_epochs=T, total_slc=SLC,
                     device=DEV, init="device", state=state)


@pytest.mark.parametrize("state,per", [("fp16", 64), ("fp32x2", 64), ("fp16", 1)])
@pytest.mark.parametrize("comp", ["blosc", "zlib", None])
def test_load_step_gpu_equals_host(state, per, comp, tmp_path):
    src = model_free_sweep(state)
    src.save_step(tmp_path / "out", compressor=comp)
    a, b = fresh(state), fresh(state)
    a.load_step(tmp_path / "out", 2, decoder="host")
    b.snapshot_tiles = per
    b.load_step(tmp_path / "out", 2, decoder="gpu")
    assert a.epoch == b.epoch == 2
    view = torch.int16 if a.cur.dtype == torch.float16 else torch.int32
    assert torch.equal(a.cur.view(view), b.cur.view(view))
    assert torch.equal(b.local_state().half(), src.local_state().half())
    assert b.decode_fallbacks == (0 if comp == "blosc" else 4) and a.decode_fallbacks == 0


def test_unknown_decoder_is_refused(tmp_path):
    sw = fresh("fp16")
    with pytest.raises(ValueError, match="decoder"):
        sw.load_step(tmp_path / "out", 1, decoder="cuda")


def test_flipped_byte_in_a_stream_names_the_file(tmp_path):
    src = model_free_sweep("fp16")
    d = src.save_step(tmp_path / "out", compressor="blosc")
    name = tiles.state_tile_name(src.row0 + 1, src.col0 + 0) + ".zip"
    path = os.path.join(d, name)
    with zipfile.ZipFile(path) as z:
        frame = z.read("0.0.0")
    formats.write_zarr_zip_blosc(path, (src.chn, tiles.TILE, tiles.TILE), "<f2", dc.flipped_stream_byte(frame))
    with pytest.raises(RuntimeError):                               # the host route refuses the file too
        formats.read_state_tile(path)
    sw = fresh("fp16")
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        sw.load_step(tmp_path / "out", 2, decoder="gpu")
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        formats.read_state_tile_dev(path, DEV)


def test_read_state_tile_dev_equals_read_state_tile():
    path = os.path.join(util.ROOT, "tests", "golden", "io_state_tile_blosc.zip")
    want = formats.read_state_tile(path)
    got = formats.read_state_tile_dev(path, DEV)
    assert got.dtype == torch.float16 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))
    assert formats.read_zarr_zip_dev(path, DEV)[1] is True          # decoded on the device, not copied


def test_stitch_dir_gpu_equals_host(tmp_path):
    src = model_free_sweep("fp16")
    d = src.save_step(tmp_path / "out", compressor="blosc")
    for slices in (None, [0, 3, 7]):
        host = stitch.stitch_dir(d, 512, 768, 2, 2, SLC, slices=slices)
        dev = stitch.stitch_dir(d, 512, 768, 2, 2, SLC, slices=slices, decoder="gpu", device=DEV)
        assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), host)
    with pytest.raises(ValueError, match="decoder"):
        stitch.stitch_dir(d, 512, 768, 2, 2, SLC, decoder="device")


def test_stitch_real_dir_gpu_equals_host(tmp_path):
    r = np.random.default_rng(5)
    size, p = 32, 16
    os.makedirs(tmp_path / "real")
    for pw in range(2):
        r0, c0 = 64, 96 + pw * size
        a = r.integers(0, 256, (2 * SLC, size + 2 * p, size + 2 * p)).astype(np.float16)
        name = f"{r0}_{r0 + size}_{c0}_{c0 + size}_{r0 - p}_{r0 + size + p}_{c0 - p}_{c0 + size + p}.zip"
        if pw:                                                      # one tile as Blosc chunks, one raw: the host route's
            formats.write_zarr_zip(tmp_path / "real" / name, a)
        else:
            formats.write_zarr_zip_blosc(tmp_path / "real" / name, a.shape, "<f2", bc.encode_frame(a.tobytes(), 2, 65536, lz4=dc.lz4_runs))
    host = stitch.stitch_real_dir(tmp_path / "real", 64, 96, 1, 2, SLC, size=size)
    dev = stitch.stitch_real_dir(tmp_path / "real", 64, 96, 1, 2, SLC, size=size, decoder="gpu", device=DEV)
    assert np.array_equal(dev.cpu().numpy(), host)


def _run_roi(*args):
    cmd = [sys.executable, os.path.join(util.ROOT, "tools", "run_roi.py"), "--hnm", "1", "--wnm", "2", "--tot_epoch", "2", *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=util.ROOT)


def test_run_roi_resumes_from_a_step_directory(tmp_path):
    """tools/run_roi.py --cur_epoch 1 of T = 2 from the directory a straight run left after step 1: the same tiles after step 2."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _run_roi("--out_dir", a, "--save_steps", "--tile_compressor", "blosc")
    assert r.returncode == 0, r.stderr[-2000:]
    os.makedirs(b)
    shutil.copytree(os.path.join(a, "timestep_1"), os.path.join(b, "timestep_1"))
    r = _run_roi("--out_dir", b, "--cur_epoch", "1", "--tile_decoder", "gpu", "--tile_compressor", "blosc")
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["resumed_from_step"] == 1 and rep["steps_measured"] == 2 and len(rep["step_s"]) == 1
    names = sorted(os.listdir(os.path.join(a, "timestep_2")))
    assert len(names) == 2 and names == sorted(os.listdir(os.path.join(b, "timestep_2")))
    for n in names:
        x = formats.read_state_tile(os.path.join(a, "timestep_2", n))
        y = formats.read_state_tile(os.path.join(b, "timestep_2", n))
        assert np.array_equal(x.view(np.uint16), y.view(np.uint16)), n
        assert not np.array_equal(x.view(np.uint16), formats.read_state_tile(os.path.join(a, "timestep_1", n)).view(np.uint16))


def test_run_roi_refuses_a_missing_step_directory(tmp_path):
    r = _run_roi("--out_dir", str(tmp_path / "none"), "--cur_epoch", "1")
    assert r.returncode != 0 and "no step directory" in r.stderr
    r = _run_roi("--out_dir", str(tmp_path / "none"), "--cur_epoch", "3")
    assert r.returncode != 0 and "outside 1 .. tot_epoch" in r.stderr
