#!/usr/bin/env python3
"""State snapshots on one MI355X: TileSweep.save_step of a 4 x 8-tile sweep state (32 tiles of float16 [100, 256, 256]) with
compressor None (raw chunks), "zlib" (host) and "blosc" (Blosc-lz4 frames encoded on the GPU).

The canvas is synthetic: every tile is half constant background (-1) and half smooth signal with noisy low mantissa bits --
the sampler's output on hashed weights is noise and says nothing about ratios.

End to end (default mode, profiler off): the three routes alternated in one process, median of --reps calls after one
warm-up each, spread = max - min of identical calls, bytes written per route, every blosc file read back.  The None and
"zlib" routes are the code of the commit before the encoder, so one process serves as the comparison.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_snapshot.py --profile OUT
    python tools/bench_snapshot.py --summarize OUT
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HNM, WNM, SLC = 4, 8, 50
TILE_BYTES = 2 * SLC * 256 * 256 * 2
WHOLE_BRAIN_RANK_TILES = 14904


def synthetic_sweep(state="fp16"):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd.brain import PAD, TileSweep
    from teramind_amd.config import PathConfig
    from teramind_amd.diffusion import SpacedDiffusionBeatGans
    assert torch.cuda.is_available(), "bench_snapshot needs a GPU"
    dev = "cuda:0"
    sw = TileSweep(PathConfig(), SpacedDiffusionBeatGans(15, "ddim"), None, None, hst=0, wst=0, hnm=HNM, wnm=WNM, total_epochs=15,
                   total_slc=SLC, device=dev, init="device", state=state)
    g = torch.Generator(device=dev).manual_seed(7)
    C, H, W = sw.chn, HNM * 256, WNM * 256
    y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    c = torch.arange(C, device=dev, dtype=torch.float32)[:, None, None]
    sig = 0.6 * torch.sin(x / 61.0 + c * 0.3) * torch.cos(y / 47.0) + 0.004 * torch.randn((C, H, W), generator=g, device=dev)
    sig = torch.where((x % 256) < 128, torch.full_like(sig, -1.0), sig)          # the left half of every tile is background
    sw.cur[:, PAD:-PAD, PAD:-PAD].copy_(sig.half().to(sw.cur.dtype))
    sw.epoch = 1
    torch.cuda.synchronize()
    return sw


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def end_to_end(reps, out):
    import numpy as np
    import torch
    from teramind_amd import formats
    sw = synthetic_sweep()
    routes = [("none", None), ("zlib", "zlib"), ("blosc", "blosc")]
    ntiles = HNM * WNM
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        times, sizes = {k: [] for k, _ in routes}, {}
        for rep in range(reps + 1):                                  # rep 0 warms every route up
            for key, comp in routes:                                 # alternated
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = sw.save_step(os.path.join(tmp, key), compressor=comp)
                torch.cuda.synchronize()
                if rep:
                    times[key].append(time.perf_counter() - t0)
                sizes[key] = dir_bytes(d)
        d = sw.step_dir(os.path.join(tmp, "blosc"))
        same = all(np.array_equal(formats.read_state_tile(os.path.join(d, f)), formats.read_state_tile(os.path.join(sw.step_dir(os.path.join(tmp, "none")), f)))
                   for f in sorted(os.listdir(d)))
    lines.append(f"save_step of a {HNM} x {WNM}-tile state ({ntiles} tiles, {TILE_BYTES / 1e6:.1f} MB each as float16), profiler off, "
                 f"routes alternated in one process, median of {reps} after a warm-up; spread = max - min of identical calls")
    lines.append(f"{'route':6s} {'s/snapshot':>11s} {'spread s':>9s} {'ms/tile':>8s} {'MB written':>11s} {'of plain':>9s}")
    med = {}
    for key, _ in routes:
        med[key] = statistics.median(times[key])
        lines.append(f"{key:6s} {med[key]:11.3f} {max(times[key]) - min(times[key]):9.3f} {1e3 * med[key] / ntiles:8.2f} "
                     f"{sizes[key] / 1e6:11.1f} {sizes[key] / (ntiles * TILE_BYTES):9.3f}")
    spread = max(max(times[k]) - min(times[k]) for k in ("zlib", "blosc"))
    gain = med["zlib"] - med["blosc"]
    lines.append(f"blosc files decode to the raw route's tiles: {same}")
    lines.append(f"zlib - blosc = {gain:.3f} s per snapshot ({1e3 * gain / ntiles:.2f} ms per tile), spread {spread:.3f} s: "
                 + ("blosc is faster by more than the spread" if gain > spread else "NO gain beyond the spread"))
    lines.append(f"none - blosc = {med['none'] - med['blosc']:.3f} s per snapshot")
    lines.append(f"EXTRAPOLATED to one rank's share of the brain ({WHOLE_BRAIN_RANK_TILES} tiles), by tile count from the figures above, not "
                 f"measured: none {med['none'] / ntiles * WHOLE_BRAIN_RANK_TILES / 60:.1f} min, zlib "
                 f"{med['zlib'] / ntiles * WHOLE_BRAIN_RANK_TILES / 60:.1f} min, blosc {med['blosc'] / ntiles * WHOLE_BRAIN_RANK_TILES / 60:.1f} min per snapshot")
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def profile(out_dir, reps):
    import torch
    sw = synthetic_sweep()
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(1 + reps):
            sw.save_step(os.path.join(tmp, "blosc"), compressor="blosc")
            torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "snapshot_meta.json"), "w") as f:
        json.dump({"snapshots": 1 + reps, "rows": HNM, "tiles": HNM * WNM, "tile_bytes": TILE_BYTES}, f)


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    meta = json.load(open(os.path.join(d, "snapshot_meta.json")))
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].split("(")[0].replace("tmk::", "").replace("void ", "")
        if "blosc" in name:
            per.setdefault(name.split("<")[0], []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    inp = meta["tiles"] * meta["tile_bytes"]
    print(f"encoder kernels per snapshot of {meta['tiles']} tiles ({inp / 1e6:.0f} MB of float16 in), rocprofv3 --kernel-trace, median over "
          f"{meta['snapshots'] - 1} snapshots after the warm-up; {meta['rows']} dispatches each (one per tile row)")
    print(f"{'kernel':22s} {'us/snapshot':>12s} {'spread us':>10s} {'input GB/s':>11s}")
    total = 0.0
    for name, calls in per.items():
        calls.sort()
        k = meta["rows"]
        runs = [sum(c[1] for c in calls[e * k:(e + 1) * k]) for e in range(meta["snapshots"])][1:]
        us = statistics.median(runs)
        total += us
        print(f"{name:22s} {us:12.1f} {max(runs) - min(runs):10.1f} {inp / us / 1e3:11.1f}")
    print(f"{'all three':22s} {total:12.1f} {'':10s} {inp / total / 1e3:11.1f}   ({total / meta['tiles']:.1f} us per tile)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="end-to-end mode: also write the report here")
    ap.add_argument("--profile", default=None, metavar="DIR", help="run the blosc snapshots only (under rocprofv3) and write DIR/snapshot_meta.json")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.profile:
        profile(a.profile, a.reps)
    else:
        end_to_end(a.reps, a.out)
