#!/usr/bin/env python3
"""Attention heat-map export on one MI355X: one whole-brain slice of read-out mosaic, float16 [8, 4576, 6624] (286 x 414 tiles
of 16 x 16 cells, K = 2), mode att_all, sigma 2, scale 2, inferno, quality 90 -> one pyramidal colour OME-TIFF of
9152 x 13248 px.

End to end (default mode, profiler off): seconds per slice for field + render + pyramid file
(`stitch.save_attn_heatmaps_pyramid` on the resident slice), alternated in the same process with the route a host would
take: the same expression with scipy.ndimage.gaussian_filter in float32 (or, where scipy is absent, a numpy separable filter:
the JSON line says which), bilinear x 2 and the table look-up in numpy, 2 x 2 numpy reductions and every 256 x 256 tile encoded
with Pillow at 4:4:4 into the same container.  The two routes are not held to equal bytes here (the host field is scipy's
float32, not the kernel's); tests/test_gpu_export_heatmap.py does that against the restatement.  Median of --reps runs after
one warm-up of each route, spread = max - min.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_heatmap.py --profile OUT
    python tools/bench_heatmap.py --summarize OUT
--profile runs field + render (planar and interleaved) 1 + --reps times; --summarize sets heat_field_kernel against its traffic
floor, (nsum + nmask) * 2 + 4 bytes per cell at the measured 2:1 read:write stream rate of profiles/r03_micro_hbm_rw.txt
(4841.9 GB/s).  The floor does not count the halo that neighbouring workgroups stage again: a floor, not a target.
"""
import argparse
import csv
import glob
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, H, W = 2, 4576, 6624
SIGMA, SCALE, VMAX, QUALITY, WEI = 2.0, 2, 2.0, 90, 229
STREAM_GBS = 4841.9                     # profiles/r03_micro_hbm_rw.txt, r:w 2:1, grid 2048


def synthetic_slice(device, h=H, w=W):
    """float16 [4K, h, w]: smooth attention channels in [0, 0.05] times noise, integer expression with ~40 % zeros (seeded)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(h * 7 + w)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    out = torch.empty((4 * K, h, w), dtype=torch.float16)
    for c in range(3 * K):
        out[c] = (0.025 * (1 + torch.sin(x / (61.0 + 5 * c)) * torch.cos(y / (47.0 - 3 * c))) * (0.5 + 0.5 * torch.rand(h, w, generator=g))).half()
    for c in range(K):
        out[3 * K + c] = (torch.randint(1, 6, (h, w), generator=g) * (torch.rand(h, w, generator=g) >= 0.4)).half()
    return out.to(device)


def host_filter():
    try:
        from scipy.ndimage import gaussian_filter
        return "scipy.ndimage.gaussian_filter (float32)", lambda p: gaussian_filter(p, sigma=SIGMA)
    except ImportError:
        import numpy as np
        from teramind_amd import heatmap

        def sep(p):
            r, t = heatmap.gaussian_taps(SIGMA)
            for ax in (0, 1):
                q = np.pad(p, [(r, r) if a == ax else (0, 0) for a in (0, 1)], mode="symmetric")
                p = sum(t[j] * (q[j:j + p.shape[0]] if ax == 0 else q[:, j:j + p.shape[1]]) for j in range(2 * r + 1))
            return p
        return "numpy separable filter (scipy absent)", sep


def host_export(mosaic_host, path, filt):
    """The host route: field, x 2 bilinear, table, reductions, Pillow tiles, same container."""
    import numpy as np
    from PIL import Image
    from teramind_amd import heatmap, ometiff
    a = mosaic_host
    v = np.maximum(a[2 * K].astype(np.float32), 0) + np.maximum(a[2 * K + 1].astype(np.float32), 0)
    msk = (a[3 * K] != 0) & (a[3 * K + 1] != 0)
    fld = filt((np.log2(v * np.float32(WEI) + 1) * msk).astype(np.float32))

    def axis(n):
        s = np.clip((np.arange(n * SCALE, dtype=np.float32) + 0.5) / SCALE - 0.5, 0, n - 1)
        i0 = s.astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), (s - i0).astype(np.float32)
    y0, y1, wy = axis(fld.shape[0])
    x0, x1, wx = axis(fld.shape[1])
    rows = fld[:, x0] + (fld[:, x1] - fld[:, x0]) * wx[None, :]
    g = rows[y0] + (rows[y1] - rows[y0]) * wy[:, None]
    idx = np.clip((g * np.float32(256.0 / VMAX)).astype(np.int32), 0, 255)
    lut = heatmap.INFERNO.copy()
    lut[0] = 0
    levels = [lut[idx]]
    for _ in ometiff.pyramid_sizes(*idx.shape)[1:]:
        s = levels[-1]
        h, w = s.shape[:2]
        ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
        b = s[ys][:, xs].astype(np.uint16)
        levels.append(((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8))

    def tiles(lv, h, w):
        s = levels[lv]
        for ty in range(0, h, 256):
            for tx in range(0, w, 256):
                ys, xs = np.minimum(np.arange(ty, ty + 256), h - 1), np.minimum(np.arange(tx, tx + 256), w - 1)
                buf = io.BytesIO()
                Image.fromarray(s[ys][:, xs], mode="RGB").save(buf, format="JPEG", quality=QUALITY, subsampling=0)
                d = buf.getvalue()
                i = d.index(b"\xff\xda")
                yield ometiff.jpeg_tile_stream_rgb(d[i + 2 + int.from_bytes(d[i + 2:i + 4], "big"):-2])
    ometiff.write_tiles(path, idx.shape[0], idx.shape[1], tiles, "jpeg", ometiff.jpeg_tables_rgb(QUALITY), samples=3)


def gpu_export(mosaic, odir):
    import torch
    from teramind_amd import stitch
    stitch.save_attn_heatmaps_pyramid(mosaic, odir, K, vmax=VMAX, wei=WEI, sigma=SIGMA, scale=SCALE, quality=QUALITY)
    torch.cuda.synchronize()


def end_to_end(reps, out, h, w):
    import torch
    import teramind_amd  # noqa: F401
    assert torch.cuda.is_available(), "bench_heatmap needs a GPU"
    sl = synthetic_slice("cuda:0", h, w)
    mosaic, host = sl[None], sl.cpu().numpy()
    which, filt = host_filter()
    with tempfile.TemporaryDirectory() as tmp:
        gpu_export(mosaic, os.path.join(tmp, "g"))                         # warm-up of both routes
        host_export(host, os.path.join(tmp, "h.tif"), filt)
        tg, th = [], []
        for _ in range(reps):                                               # alternated
            t0 = time.perf_counter()
            gpu_export(mosaic, os.path.join(tmp, "g"))
            t1 = time.perf_counter()
            host_export(host, os.path.join(tmp, "h.tif"), filt)
            t2 = time.perf_counter()
            tg.append(t1 - t0)
            th.append(t2 - t1)
        res = {"what": "attention heat-map export, seconds per slice (field + render + pyramid file), profiler off",
               "mosaic_slice": [4 * K, h, w], "mode": "att_all", "sigma": SIGMA, "scale": SCALE, "quality": QUALITY, "reps": reps,
               "image_px": [h * SCALE, w * SCALE], "host_filter": which,
               "gpu_file_bytes": os.path.getsize(os.path.join(tmp, "g", "heat_att_all_0.tif")),
               "host_file_bytes": os.path.getsize(os.path.join(tmp, "h.tif")),
               "gpu_s_median": round(statistics.median(tg), 4), "gpu_s_spread": round(max(tg) - min(tg), 4),
               "host_s_median": round(statistics.median(th), 4), "host_s_spread": round(max(th) - min(th), 4)}
    res["host_over_gpu"] = round(res["host_s_median"] / res["gpu_s_median"], 2)
    res["whole_brain_50_slices_s_EXTRAPOLATED"] = round(50 * res["gpu_s_median"], 1)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def profile(out_dir, reps, h, w):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import heatmap
    assert torch.cuda.is_available(), "bench_heatmap needs a GPU"
    sl = synthetic_slice("cuda:0", h, w)
    for _ in range(1 + reps):
        fld = heatmap.field(sl, K, "att_all", WEI, SIGMA)
        heatmap.render(fld, heatmap.INFERNO, 0.0, VMAX, SCALE, 1)
        heatmap.render(fld, heatmap.INFERNO, 0.0, VMAX, SCALE, 1, interleaved=True)
        torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "heatmap_meta.json"), "w") as f:
        json.dump({"runs": 1 + reps, "cells": h * w, "pixels": h * w * SCALE * SCALE, "nsum": K, "nmask": K}, f)


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    meta = json.load(open(os.path.join(d, "heatmap_meta.json")))
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].split("(")[0].replace("tmk::", "").replace("void ", "")
        if name.startswith("heat_"):
            per.setdefault(name, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    cells, px = meta["cells"], meta["pixels"]
    floor_us = cells * ((meta["nsum"] + meta["nmask"]) * 2 + 4) / (STREAM_GBS * 1e3)
    print(f"kernel times, {cells} cells -> {px} px (rocprofv3 --kernel-trace; warm-up run dropped; median, spread = max - min)")
    for name, calls in sorted(per.items()):
        calls.sort()
        per_run = len(calls) // meta["runs"]
        for k in range(per_run):                                            # render: planar first, then interleaved
            us = [c[1] for c in calls[per_run + k::per_run]]
            med = statistics.median(us)
            if name.startswith("heat_field"):
                note = (f"traffic floor {floor_us:.1f} us ({(meta['nsum'] + meta['nmask']) * 2 + 4} B/cell at {STREAM_GBS} GB/s): "
                        f"{med / floor_us:.2f} x the floor, {cells / med / 1e3:.2f} Gcell/s")
            else:
                moved = 3 * px + 4 * cells
                note = f"{'planar' if k == 0 else 'interleaved'}: {moved / 1e6:.1f} MB moved, {moved / med / 1e3:.1f} GB/s, {px / med / 1e3:.2f} Gpx/s"
            print(f"  {name:40s} {med:10.1f} us  spread {max(us) - min(us):8.1f}  n = {len(us)}  {note}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="end-to-end mode: also write the JSON line here")
    ap.add_argument("--profile", default=None, metavar="DIR", help="run field + render only (under rocprofv3), write DIR/heatmap_meta.json")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    ap.add_argument("--cells", type=int, nargs=2, default=(H, W), metavar=("H", "W"), help="mosaic cells (default: the whole brain)")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.profile:
        profile(a.profile, a.reps, *a.cells)
    else:
        end_to_end(a.reps, a.out, *a.cells)
