#!/usr/bin/env python3
"""Mints tests/golden/metrics3d_ref.npz FROM THE REFERENCE (test infrastructure; runs on the CPU where the reference is; no GPU
test runs it): what the reference's own utils/metrics.py returns in float64 for the seeded 5-D cases of
tests/metrics3d_cases.py.  Results only: the inputs come from the seeds.

`utils/metrics.py` is imported as tools/make_metrics_golden.py imports it (the cellpose stub, TERAMIND_REFERENCE naming the
reference's directory).  Recorded per case '{kind}-{D}x{H}x{W}':
  /ssim_pc, /cs   `_ssim(X, Y, data_range=255, win=...)` with the [C, 1, 1, 1, n] window: per-channel ssim and cs, [N, C]
  /ssim           `ssim(X, Y, size_average=False)`, [N]
  /ssim_module    `SSIM(channel=C, spatial_dims=3)(X, Y)`, a scalar
and for the two MS cases (N = 1)
  /ms_ssim        `ms_ssim(X, Y, size_average=False)`, [N]
  /ms_module      `MS_SSIM(channel=C, spatial_dims=3)(X, Y)`, a scalar
Run:  python tools/make_metrics3d_golden.py"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import metrics3d_cases as m3  # noqa: E402
from make_metrics_golden import load_reference_metrics  # noqa: E402


def main():
    rm = load_reference_metrics()
    out = {}
    with torch.inference_mode(), warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # the reference warns at every level it does not smooth in depth
        win = rm._fspecial_gauss_1d(m3.WIN, m3.SIGMA).repeat([m3.C, 1, 1, 1, 1])
        assert np.array_equal(win[0].reshape(-1).numpy(), m3.taps())
        for kind, shape in m3.CASES:
            Xu, Yu = m3.pair(kind, shape)
            X, Y = torch.from_numpy(Xu.astype(np.float64)), torch.from_numpy(Yu.astype(np.float64))
            key = m3.case_id(kind, shape)
            s, cs = rm._ssim(X, Y, data_range=255, win=win, size_average=False, K=m3.K)
            out[key + "/ssim_pc"], out[key + "/cs"] = s.numpy(), cs.numpy()
            out[key + "/ssim"] = rm.ssim(X, Y, data_range=255, size_average=False).numpy()
            out[key + "/ssim_module"] = rm.SSIM(channel=m3.C, spatial_dims=3)(X, Y).numpy()
        for kind, shape in m3.MS_CASES:
            Xu, Yu = m3.pair(kind, shape, n=1)
            X, Y = torch.from_numpy(Xu.astype(np.float64)), torch.from_numpy(Yu.astype(np.float64))
            key = m3.case_id(kind, shape)
            out[key + "/ssim"] = rm.ssim(X, Y, data_range=255, size_average=False).numpy()
            out[key + "/ms_ssim"] = rm.ms_ssim(X, Y, data_range=255, size_average=False).numpy()
            out[key + "/ms_module"] = rm.MS_SSIM(channel=m3.C, spatial_dims=3)(X, Y).numpy()
        for k, v in out.items():
            assert v.dtype == np.float64, k
    path = os.path.join(ROOT, "tests", "golden", "metrics3d_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
