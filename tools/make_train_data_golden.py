#!/usr/bin/env python3
"""Mints tests/golden/train_data_ref.npz FROM THE REFERENCE (test infrastructure; runs where the reference is, like
tools/make_train_dropout_golden.py; no GPU test runs it): what the reference's own training dataset returns for an image.

The real `utils.MBADataset` module is imported through oracle.ref_harness (whose stubs stand in for the absent `zarr`, `sparse`
and `torchvision` packages).  The dataset object is built without `__init__` (it reads csv lists that are not shipped); only
the attributes `_getimg` reads are set.  `zarr.load` is patched to return the seeded tile of tests/train_data_cases.py.
Recorded: `MBADataset._getimg(path, top, left, snm) / 127.5 - 1` for every stain x snum x draw, and for one stain / snum the
reference's `_trans` (torch.rot90, then hflip) over every rot x flip, driven with pinned `random.randint` / `torch.rand` and a
placeholder gene object (the gene half needs the real `sparse` package and is not recorded).  torchvision is absent: its
`hflip` is taken as `im.flip(-1)` (what torchvision's tensor path does); that one boundary is unpinned.
Run:  python tools/make_train_data_golden.py"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import teramind_amd  # noqa: E402,F401
from oracle import ref_harness as rh  # noqa: E402
from teramind_amd import synth  # noqa: E402
import train_data_cases as tc  # noqa: E402


class PlaceholderGene:
    """Stands in for the COO `_trans` also turns; only its calls are absorbed."""

    def __init__(self, n):
        self.shape, self.coords = (n, n, 1), np.zeros((3, 1), dtype=np.int64)

    def transpose(self, axes):
        return self


def main():
    rh.load()
    import zarr
    import torchvision.transforms.functional as TF
    if not hasattr(TF, "hflip"):
        TF.hflip = lambda im: im.flip(-1)
    from utils.MBADataset import MBADataset
    tile = synth.image_tile(tc.REF_TAG, tc.REF_SHAPE, tc.REF_SEED)
    zarr.load = lambda pth: tile
    out = {}
    for stain in tc.STAINS:
        for snum in tc.SNUMS:
            ds = MBADataset.__new__(MBADataset)
            ds.sdim, ds.stain, ds.snum, ds.spad = tc.REF_SDIM, stain, snum, tc.SPAD[snum]
            draws = tc.ref_draws(snum)
            res = [ds._getimg("gene/t.npz", top, left, snm) / 127.5 - 1 for top, left, snm in draws]
            out[f"img/{stain}/{snum}/draws"] = np.array(draws, dtype=np.int32)
            out[f"img/{stain}/{snum}/out"] = torch.stack(res).numpy()
            assert out[f"img/{stain}/{snum}/out"].dtype == np.float32
            if (stain, snum) == (tc.TRANS_STAIN, tc.TRANS_SNUM):
                top, left, snm = draws[2]
                for rot in range(4):
                    for flip in (0, 1):
                        im = ds._getimg("gene/t.npz", top, left, snm)
                        real_ri, real_rand = random.randint, torch.rand
                        random.randint = lambda a, b: rot
                        torch.rand = lambda n: torch.tensor([0.25 if flip else 0.75])
                        try:
                            im2, _ = ds._trans(im, PlaceholderGene(tc.REF_SDIM // 16), None, False)
                        finally:
                            random.randint, torch.rand = real_ri, real_rand
                        out[f"trans/{rot}/{flip}"] = (im2 / 127.5 - 1).contiguous().numpy()
                out["trans/draw"] = np.array([top, left, snm], dtype=np.int32)
    p = os.path.join(ROOT, "tests", "golden", "train_data_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
