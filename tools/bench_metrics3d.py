#!/usr/bin/env python3
"""`metrics.ssim` with the 3-D window on one MI355X: uint8 volume pairs [1, 1, 50, 2048, 2048] and [1, 1, 50, 4096, 4096] (one
stain of an 8 x 8- and of a 16 x 16-tile ROI, 50 slices), 11 taps at sigma 1.5.

End to end (default mode, profiler off): milliseconds per call, alternated run by run in one process, of
  volume   `metrics.ssim` on the 5-D pair (tm_ssim_volumes: one pass over the uint8 voxels),
  planes   `metrics.ssim` on the same voxels as 50 planes [1, 50, H, W] (tm_ssim_planes): the yardstick; the 3-D pass does
           three filter passes where the plane kernel does two, and re-reads the in-plane halo of its smaller tile,
  torch    the reference's formula composed from torch ops on the same GPU: float32 copies and the grouped `F.conv3d`
           composition of `_ssim` (utils/metrics.py:236-305, restated below).  With --torch_max_side S it runs only on
           volumes whose side is at most S (its intermediates are several GB per 2048^2 x 50 volume).
A run is --iters calls between two synchronisations; median of --reps runs after a warm-up of every route, spread = max - min.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_metrics3d.py --profile OUT
    python tools/bench_metrics3d.py --summarize OUT
--summarize joins the trace with the work computed from the shapes: bytes = the voxels of X and Y read once, operations = five
quantities x 11 taps x three passes per output voxel plus the row pass over the 26 / 16 halo rows of a tile (one FMA =
2 FLOP), the ns per voxel of both kernels, and the share of the larger of the two bounds (8.0 TB/s, 157.3 TFLOP/s fp32
vector: the specification figures) and which one binds.
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

SIDES = (2048, 4096)
DEPTH = 50
WIN, SIGMA = 11, 1.5
PEAK_BYTES, PEAK_FLOPS = 8.0e12, 157.3e12
TILE = 16                                                # SSIM3_TH = SSIM3_TW


def synthetic_pair(n, device):
    """Two uint8 volumes [1, 1, DEPTH, n, n]: a smooth field that drifts with z plus noise, and the same field with other
    noise (seeded); built plane by plane on the device."""
    import torch
    g = torch.Generator(device=device).manual_seed(n)
    y, x = torch.meshgrid(torch.arange(n, dtype=torch.float32, device=device), torch.arange(n, dtype=torch.float32, device=device),
                          indexing="ij")
    a = torch.empty((1, 1, DEPTH, n, n), dtype=torch.uint8, device=device)
    b = torch.empty_like(a)
    for z in range(DEPTH):
        base = 127.5 + 90 * torch.sin(x / 61.0 + 0.2 * z) * torch.cos(y / 47.0 - 0.1 * z)
        a[0, 0, z] = (base + 6 * torch.randn(n, n, generator=g, device=device)).clamp_(0, 255).to(torch.uint8)
        b[0, 0, z] = (base + 12 * torch.randn(n, n, generator=g, device=device)).clamp_(0, 255).to(torch.uint8)
    return a, b


def torch_ssim3(X, Y, win, data_range=255.0, K=(0.01, 0.03)):
    """The reference's 5-D `ssim(..., size_average=False)` composed from torch ops: float copies, fifteen grouped conv3d calls."""
    import torch.nn.functional as F
    X, Y = X.float(), Y.float()
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2

    def filt(t):
        for i in range(3):
            t = F.conv3d(t, weight=win.transpose(2 + i, -1), stride=1, padding=0, groups=t.shape[1])
        return t
    mu1, mu2 = filt(X), filt(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = filt(X * X) - mu1_sq, filt(Y * Y) - mu2_sq, filt(X * Y) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1).mean(1)


def work(n):
    """Bytes and FLOP of one volume call and of the plane call over the same voxels."""
    o2 = (n - WIN + 1) ** 2
    halo = (TILE + WIN - 1) / TILE                        # input rows the row pass filters per output row of a tile
    vol = 2 * 5 * WIN * (DEPTH * o2 * (halo + 1) + (DEPTH - WIN + 1) * o2)
    return {"voxels": DEPTH * n * n, "bytes": 2 * DEPTH * n * n, "flop_volume": vol, "flop_planes": 2 * 5 * WIN * 2 * o2 * DEPTH}


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, r


def end_to_end(reps, iters, out, torch_max_side):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import metrics
    assert torch.cuda.is_available(), "bench_metrics3d needs a GPU"
    res = {"what": "metrics.ssim, 3-D window, against the plane route on the same voxels and the torch composition of the "
                   "reference's 5-D _ssim; ms per call, profiler off", "taps": WIN, "depth": DEPTH, "reps": reps,
           "iters_per_run": iters, "volumes": []}
    for n in SIDES:
        X, Y = synthetic_pair(n, "cuda:0")
        Xp, Yp = X[0], Y[0]                                                      # [1, 50, n, n]: the same memory as planes
        win = metrics._fspecial_gauss_1d(WIN, SIGMA).repeat(1, 1, 1, 1, 1).to("cuda:0")
        routes = {"volume": lambda: metrics.ssim(X, Y, size_average=False),
                  "planes": lambda: metrics.ssim(Xp, Yp, size_average=False)}
        if n <= torch_max_side:
            routes["torch"] = lambda: torch_ssim3(X, Y, win)
        vals = {k: timed(f, 1)[1].item() for k, f in routes.items()}                # warm-up of every route
        times = {k: [] for k in routes}
        for _ in range(reps):                                                       # alternated
            for k, f in routes.items():
                times[k].append(timed(f, 1 if k == "torch" else iters)[0])
        vox = work(n)["voxels"]
        r = {"volume": f"{DEPTH} x {n} x {n}"}
        for k in routes:
            med = statistics.median(times[k])
            r[k + "_value"] = vals[k]
            r[k + "_ms_median"], r[k + "_ms_spread"] = round(med, 4), round(max(times[k]) - min(times[k]), 4)
            r[k + "_ns_per_voxel"] = round(med * 1e6 / vox, 4)
        r["volume_over_planes"] = round(r["volume_ms_median"] / r["planes_ms_median"], 2)
        if "torch" in routes:
            r["abs_diff_to_torch"] = abs(vals["volume"] - vals["torch"])
            r["torch_over_volume"] = round(r["torch_ms_median"] / r["volume_ms_median"], 2)
            torch.cuda.reset_peak_memory_stats()
            base0 = torch.cuda.memory_allocated()
            timed(routes["torch"], 1)
            r["torch_peak_alloc_MB"] = round((torch.cuda.max_memory_allocated() - base0) / 2 ** 20, 1)
        torch.cuda.reset_peak_memory_stats()
        base0 = torch.cuda.memory_allocated()
        timed(routes["volume"], 1)
        r["volume_peak_alloc_MB"] = round((torch.cuda.max_memory_allocated() - base0) / 2 ** 20, 3)
        res["volumes"].append(r)
        print(json.dumps(r), flush=True)
        del X, Y, Xp, Yp, routes
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
    assert torch.cuda.is_available(), "bench_metrics3d needs a GPU"
    for n in SIDES:
        X, Y = synthetic_pair(n, "cuda:0")
        Xp, Yp = X[0], Y[0]
        for _ in range(1 + reps):
            metrics.ssim(X, Y, size_average=False)
            metrics.ssim(Xp, Yp, size_average=False)
        torch.cuda.synchronize()
        del X, Y, Xp, Yp
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "metrics3d_meta.json"), "w") as f:
        json.dump({"calls": 1 + reps, "sides": list(SIDES)}, f)


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    meta = json.load(open(os.path.join(d, "metrics3d_meta.json")))
    per = {}
    for row in csv.DictReader(open(files[0])):
        for key in ("ssim_volumes_kernel", "ssim_planes_kernel"):
            if key in row["Kernel_Name"]:
                per.setdefault(key, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    print("kernel times per metrics.ssim call (rocprofv3 --kernel-trace; median over the calls after the warm-up)")
    print(f"{'side':>6s} {'kernel':20s} {'us':>10s} {'spread us':>10s} {'ns/voxel':>9s} {'GB/s':>8s} {'GFLOP':>8s} {'TFLOP/s':>8s} "
          f"{'bytes bound us':>14s} {'flop bound us':>13s} {'share':>6s} binds")
    k = meta["calls"]
    for name in per:
        per[name].sort()
    for i, n in enumerate(meta["sides"]):
        w = work(n)
        us_of = {}
        for name, calls in per.items():
            runs = [c[1] for c in calls[i * k + 1:(i + 1) * k]]
            if not runs:
                print(f"{n:6d} {name:20s} not in the trace")
                continue
            us = us_of[name] = statistics.median(runs)
            flop = w["flop_volume"] if name == "ssim_volumes_kernel" else w["flop_planes"]
            tb, tf = w["bytes"] / PEAK_BYTES * 1e6, flop / PEAK_FLOPS * 1e6
            print(f"{n:6d} {name:20s} {us:10.1f} {max(runs) - min(runs):10.1f} {us * 1e3 / w['voxels']:9.4f} {w['bytes'] / us / 1e3:8.1f} "
                  f"{flop / 1e9:8.2f} {flop / us / 1e6:8.2f} {tb:14.1f} {tf:13.1f} {max(tb, tf) / us:6.1%} "
                  f"{'operations' if tf > tb else 'bytes'}")
        if len(us_of) == 2:
            print(f"{n:6d} volume kernel / plane kernel on the same voxels: {us_of['ssim_volumes_kernel'] / us_of['ssim_planes_kernel']:.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed run of the kernel routes (the torch route takes one)")
    ap.add_argument("--torch_max_side", type=int, default=4096, help="largest volume side the torch composition is run on")
    ap.add_argument("--out", default=None, help="end-to-end mode: also write the JSON line here")
    ap.add_argument("--profile", default=None, metavar="DIR", help="run the kernel routes only (under rocprofv3) and write DIR/metrics3d_meta.json")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.profile:
        profile(a.profile, a.reps)
    else:
        end_to_end(a.reps, a.iters, a.out, a.torch_max_side)
