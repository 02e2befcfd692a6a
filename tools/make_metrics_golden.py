#!/usr/bin/env python3
"""Mints tests/golden/metrics_ref.npz FROM THE REFERENCE (test infrastructure; runs on the CPU where the reference is; no GPU
test runs it): what the reference's own utils/metrics.py returns in float64 for the seeded cases of tests/metrics_cases.py.

`utils/metrics.py` is imported as it is; its `from cellpose import plot` (used only by the figure helpers) is met by an empty
stub module in sys.modules.  Recorded per case '{kind}-{H}x{W}' (inputs are not stored: they come from the seeds):
  /ssim_pc, /cs   `_ssim(X, Y, data_range=255, win=...)`: per-channel ssim and cs, [N, C]
  /ssim           `ssim(X, Y, size_average=False)`, [N]
  /psnr           `PSNR()(X, Y)`, [N]
  /ms_ssim        `ms_ssim(X, Y, size_average=False)`, [N]   (the 176 x 163 cases)
Run:  python tools/make_metrics_golden.py   (TERAMIND_REFERENCE names the reference's directory)"""
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_cases as mc  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402


def load_reference_metrics():
    if "cellpose" not in sys.modules:
        cp = types.ModuleType("cellpose")
        cp.plot = types.ModuleType("cellpose.plot")
        sys.modules["cellpose"], sys.modules["cellpose.plot"] = cp, cp.plot
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, rh.REF_ROOT)
    from utils import metrics
    return metrics


def main():
    rm = load_reference_metrics()
    out = {}
    with torch.inference_mode(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kind, shape in mc.CASES:
            Xu, Yu = mc.pair(kind, shape)
            X, Y = torch.from_numpy(Xu.astype(np.float64)), torch.from_numpy(Yu.astype(np.float64))
            key = mc.case_id(kind, shape)
            win = rm._fspecial_gauss_1d(mc.WIN, mc.SIGMA).repeat([mc.C, 1, 1, 1])
            assert np.array_equal(win[0].reshape(-1).numpy(), mc.taps())
            s, cs = rm._ssim(X, Y, data_range=255, win=win, size_average=False, K=mc.K)
            out[key + "/ssim_pc"], out[key + "/cs"] = s.numpy(), cs.numpy()
            out[key + "/ssim"] = rm.ssim(X, Y, data_range=255, size_average=False).numpy()
            out[key + "/psnr"] = rm.PSNR()(X, Y).numpy()
            if shape == mc.MS_SHAPE:
                out[key + "/ms_ssim"] = rm.ms_ssim(X, Y, data_range=255, size_average=False).numpy()
            for k, v in out.items():
                assert v.dtype == np.float64, k
    path = os.path.join(ROOT, "tests", "golden", "metrics_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
