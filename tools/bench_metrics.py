#!/usr/bin/env python3
"""`metrics.ssim` on one MI355X: uint8 plane pairs of 4096^2 and 8192^2 (the 16 x 16- and 32 x 32-tile ROI slices of
profiles/export_pyramid.txt), 11 taps at sigma 1.5.

End to end (default mode, profiler off): milliseconds per call of `metrics.ssim` (tm_ssim_planes: one pass over the uint8
pixels), alternated run by run in the same process with the baseline a user without the kernel would run on the same GPU:
the reference's formula composed from torch ops, i.e. float32 copies of both planes and the grouped `F.conv2d` composition of
`_ssim` (utils/metrics.py:236-305, restated below).  A run is --iters calls between two synchronisations; median of --reps
runs after a warm-up of both routes, spread = max - min.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_metrics.py --profile OUT
    python tools/bench_metrics.py --summarize OUT
--summarize joins the trace with the work computed from the shapes: bytes = the pixels of X and Y read once, operations =
five quantities x n taps x two passes per output pixel (one FMA = 2 FLOP), and reports the share of the larger of the two
bounds (8.0 TB/s, 157.3 TFLOP/s fp32 vector: the specification figures) and which one binds.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4096, 8192)
WIN, SIGMA = 11, 1.5
PEAK_BYTES, PEAK_FLOPS = 8.0e12, 157.3e12


def synthetic_pair(n, device):
    """Two uint8 planes [1, 1, n, n]: a smooth field plus noise, and the same field with other noise (seeded)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(n)
    y, x = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    base = 127.5 + 90 * torch.sin(x / 61.0) * torch.cos(y / 47.0)
    a = (base + 6 * torch.randn(n, n, generator=g)).clamp_(0, 255).to(torch.uint8)
    b = (base + 12 * torch.randn(n, n, generator=g)).clamp_(0, 255).to(torch.uint8)
    return a[None, None].to(device), b[None, None].to(device)


def torch_ssim(X, Y, win, data_range=255.0, K=(0.01, 0.03)):
    """The reference's `ssim(..., size_average=False)` composed from torch ops: float copies, ten grouped conv2d calls."""
    import torch.nn.functional as F
    X, Y = X.float(), Y.float()
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2

    def filt(t):
        t = F.conv2d(t, weight=win.transpose(2, -1), stride=1, padding=0, groups=t.shape[1])
        return F.conv2d(t, weight=win, stride=1, padding=0, groups=t.shape[1])
    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = filt(X * X) - mu1_sq, filt(Y * Y) - mu2_sq, filt(X * Y) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1).mean(1)


def work(n):
    out = (n - WIN + 1) ** 2
    return {"bytes": 2 * n * n, "flop": 2 * 5 * WIN * 2 * out}


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, r


def end_to_end(reps, iters, out):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import metrics
    assert torch.cuda.is_available(), "bench_metrics needs a GPU"
    res = {"what": "metrics.ssim against the torch composition of the reference's _ssim, ms per call, profiler off",
           "taps": WIN, "reps": reps, "iters_per_run": iters, "planes": []}
    for n in SIZES:
        X, Y = synthetic_pair(n, "cuda:0")
        win = metrics._fspecial_gauss_1d(WIN, SIGMA).repeat(1, 1, 1, 1).to("cuda:0")
        fused = lambda: metrics.ssim(X, Y, size_average=False)                      # noqa: E731
        base = lambda: torch_ssim(X, Y, win)                                        # noqa: E731
        _, a = timed(fused, 2)                                                      # warm-up of both routes
        _, b = timed(base, 2)
        tf, tb = [], []
        for _ in range(reps):                                                       # alternated
            tf.append(timed(fused, iters)[0])
            tb.append(timed(base, max(1, iters // 4))[0])
        r = {"plane": f"{n} x {n}", "ssim_fused": a.item(), "ssim_torch": b.item(), "abs_diff": abs(a.item() - b.item()),
             "fused_ms_median": round(statistics.median(tf), 4), "fused_ms_spread": round(max(tf) - min(tf), 4),
             "torch_ms_median": round(statistics.median(tb), 4), "torch_ms_spread": round(max(tb) - min(tb), 4),
             "torch_peak_alloc_MB": None}
        r["torch_over_fused"] = round(r["torch_ms_median"] / r["fused_ms_median"], 2)
        torch.cuda.reset_peak_memory_stats()
        base0 = torch.cuda.memory_allocated()
        timed(base, 1)
        r["torch_peak_alloc_MB"] = round((torch.cuda.max_memory_allocated() - base0) / 2 ** 20, 1)
        res["planes"].append(r)
        del X, Y
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def profile(out_dir, reps):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import metrics
    assert torch.cuda.is_available(), "bench_metrics needs a GPU"
    for n in SIZES:
        X, Y = synthetic_pair(n, "cuda:0")
        for _ in range(1 + reps):
            metrics.ssim(X, Y, size_average=False)
        torch.cuda.synchronize()
        del X, Y
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "metrics_meta.json"), "w") as f:
        json.dump({"calls": 1 + reps, "sizes": list(SIZES)}, f)


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    meta = json.load(open(os.path.join(d, "metrics_meta.json")))
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        for key in ("ssim_planes_kernel", "ssim_sum_kernel"):
            if key in name:
                per.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    print("kernel times per metrics.ssim call (rocprofv3 --kernel-trace; median over the calls after the warm-up)")
    print(f"{'plane':>6s} {'kernel':20s} {'us':>9s} {'spread us':>10s} {'MB read':>8s} {'GB/s':>8s} {'GFLOP':>7s} {'TFLOP/s':>8s} "
          f"{'bytes bound us':>14s} {'flop bound us':>13s} {'share':>6s} binds")
    for name in per:
        per[name].sort()
    k = meta["calls"]
    for i, n in enumerate(meta["sizes"]):
        w = work(n)
        for name, calls in per.items():
            runs = [c[1] for c in calls[i * k + 1:(i + 1) * k]]
            if not runs:
                print(f"{n:6d} {name:20s} not in the trace")
                continue
            us = statistics.median(runs)
            if name != "ssim_planes_kernel":
                print(f"{n:6d} {name:20s} {us:9.1f} {max(runs) - min(runs):10.1f}")
                continue
            tb, tf = w["bytes"] / PEAK_BYTES * 1e6, w["flop"] / PEAK_FLOPS * 1e6
            print(f"{n:6d} {name:20s} {us:9.1f} {max(runs) - min(runs):10.1f} {w['bytes'] / 1e6:8.1f} {w['bytes'] / us / 1e3:8.1f} "
                  f"{w['flop'] / 1e9:7.2f} {w['flop'] / us / 1e6:8.2f} {tb:14.1f} {tf:13.1f} {max(tb, tf) / us:6.1%} "
                  f"{'operations' if tf > tb else 'bytes'}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed run of the fused route (the torch route takes a quarter)")
    ap.add_argument("--out", default=None, help="end-to-end mode: also write the JSON line here")
    ap.add_argument("--profile", default=None, metavar="DIR", help="run the fused calls only (under rocprofv3) and write DIR/metrics_meta.json")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.profile:
        profile(a.profile, a.reps)
    else:
        end_to_end(a.reps, a.iters, a.out)
