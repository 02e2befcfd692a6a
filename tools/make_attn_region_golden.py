#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- mints tests/golden/attn_readout_k4.npz from the REAL reference (CPU).

    python tools/make_attn_region_golden.py

The K = 4 companion of the G7 block of oracle/make_golden.py: the reference's own test_attn.Tester._run_batch
(imported through oracle/ref_harness.py, never copied) on one seeded gene tile with a 4-gene `glst`, the
gene count of the MROI regions (utils/__init__.py:73-89).  Only the recorded result is written
([50, 16, 16, 16] float16); the inputs are regenerated at test time from (tag, seed) by teramind_amd.synth and
teramind_amd.weights.
"""
import contextlib
import importlib
import io
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import teramind_amd  # noqa: E402,F401
from oracle import ref_harness as rh  # noqa: E402
from teramind_amd import synth  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GLST = [191, 180, 67, 57]          # four distinct indices < 229; tests/test_gpu_attn_readout.py uses the same list
TAG, SEED, DENSITY = "attn/tile_k4", 0, 0.05


def main():
    if not rh.available():
        raise SystemExit("the reference checkout is not available")
    rh.load()
    cfg = PathConfig()
    mv = rh.make_model(rh.make_conf(method="ours_vis"))
    mv.load_state_dict(hashed_state_dict(cfg, 0, vis_only=True), strict=False)
    for name in ("pyvips", "seaborn"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    with contextlib.redirect_stdout(io.StringIO()):
        ta = importlib.import_module("test_attn")
    saved = {}
    ta.zarr.save_array = lambda p, a: saved.__setitem__(str(p), a)
    tt = ta.Tester.__new__(ta.Tester)
    tt.gpu_id = "cpu"
    tt.conf = types.SimpleNamespace(patch_size=64, gn_sz=4, fp16=True)
    tt.z_size, tt.tot_slc, tt.tot_rna, tt.n_stn, tt.glst = 4, 50, 500, 2, list(GLST)
    tt.model = mv
    tile = synth.gene_counts(TAG, (1, 20, 20, 26000), SEED, density=DENSITY)
    dat, crd, ssz = synth.dense_to_coo(tile)
    with torch.inference_mode():
        tt._run_batch((torch.zeros(1, 320, 320, 100), torch.tensor([[256, 512, 512, 768]]), dat, crd, ssz,
                       torch.tensor([0])), 0, Path("o"))
    arr = list(saved.values())[0]
    assert arr.shape == (50, 16, 16, 16) and arr.dtype == np.float16, (arr.shape, arr.dtype)
    path = os.path.join(OUT, "attn_readout_k4.npz")
    np.savez_compressed(path, out=arr)
    print(f"attn_readout_k4.npz written {arr.shape} {arr.dtype} {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
