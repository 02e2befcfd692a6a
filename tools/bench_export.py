#!/usr/bin/env python3
"""Pyramidal OME-TIFF export on one MI355X: a 16 x 16-tile plane (4096^2, 341 tiles with its pyramid) and a 32 x 32-tile
plane (8192^2, 1365 tiles), smooth plus noise, quality 75.

End to end (default mode, profiler off): seconds per plane for uint8 conversion + pyramid + encode + copy + file write
(`stitch.save_slices_pyramid` on a resident float plane), alternated in the same process with the baseline an exporter
without these kernels would run: the plane downloaded, the levels reduced with numpy and every 256 x 256 tile encoded with
Pillow on the host into the same container.  Median of --reps runs after one warm-up, spread = max - min.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_export.py --profile OUT
    python tools/bench_export.py --summarize OUT
--profile exports each plane 1 + --reps times and writes OUT/export_meta.json (dispatches per export, pixels, scan bytes);
--summarize joins it with the kernel trace: per kernel the time per plane, the bytes its algorithm moves and pixels per second.

--rgb: the same for the colour composite export of a plane pair (`stitch.save_composites_pyramid`: PolyT green, DAPI blue,
YCbCr 4:4:4 tiles) against Pillow encoding the same composite tiles with `subsampling=0` on the host; the files of the two
routes must be identical.  With --profile / --summarize it records and reports the colour tile kernel against three grey
encodes (`tm_jpeg_encode_tiles`) of planes of that size, which is the number of 8 x 8 blocks the colour kernel processes.
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

SIZES = (4096, 8192)
QUALITY = 75


def synthetic_state(n, device):
    """One float plane in [-1, 1]: smooth field plus noise (seeded)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(n)
    y, x = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    a = 0.6 * torch.sin(x / 61.0) * torch.cos(y / 47.0) + 0.08 * torch.randn(n, n, generator=g)
    return a.clamp_(-1, 1)[None].to(device)


def host_export(state, path):
    """The baseline: download, numpy reductions, Pillow per tile, same container."""
    import numpy as np
    from PIL import Image
    from teramind_amd import ometiff, stitch
    a = stitch.to_uint8(state[0]).cpu().numpy()
    levels = [a]
    for _ in ometiff.pyramid_sizes(*a.shape)[1:]:
        s = levels[-1]
        h, w = s.shape
        ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
        b = s[np.ix_(ys, xs)].astype(np.uint16)
        levels.append(((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8))

    def tiles(lv, h, w):
        s = levels[lv]
        for y0 in range(0, h, 256):
            for x0 in range(0, w, 256):
                ys, xs = np.minimum(np.arange(y0, y0 + 256), h - 1), np.minimum(np.arange(x0, x0 + 256), w - 1)
                buf = io.BytesIO()
                Image.fromarray(s[np.ix_(ys, xs)], mode="L").save(buf, format="JPEG", quality=QUALITY)
                d = buf.getvalue()
                i = d.index(b"\xff\xda")
                yield ometiff.jpeg_tile_stream(d[i + 2 + int.from_bytes(d[i + 2:i + 4], "big"):-2])
    ometiff.write_tiles(path, a.shape[0], a.shape[1], tiles, "jpeg", ometiff.jpeg_tables(QUALITY))


def gpu_export(state, odir):
    import torch
    from teramind_amd import stitch
    stitch.save_slices_pyramid(state, odir, slc=1, quality=QUALITY)
    torch.cuda.synchronize()


def synthetic_pair(n, device):
    """A two-stain state [(c s) = 2, n, n] of one slice: two different planes of synthetic_state's kind."""
    import torch
    return torch.cat([synthetic_state(n, device), synthetic_state(n + 1, device)[:, :n, :n]])


def host_export_rgb(state, path):
    """The colour baseline: both planes downloaded, each reduced with numpy, every level's tiles stacked [0, PolyT, DAPI] and
    encoded with Pillow at 4:4:4 on the host into the same container."""
    import numpy as np
    from PIL import Image
    from teramind_amd import ometiff, stitch

    def pyramid(a):
        levels = [a]
        for _ in ometiff.pyramid_sizes(*a.shape)[1:]:
            s = levels[-1]
            h, w = s.shape
            ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
            b = s[np.ix_(ys, xs)].astype(np.uint16)
            levels.append(((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8))
        return levels
    dapi, polyt = pyramid(stitch.to_uint8(state[0]).cpu().numpy()), pyramid(stitch.to_uint8(state[1]).cpu().numpy())

    def tiles(lv, h, w):
        for y0 in range(0, h, 256):
            for x0 in range(0, w, 256):
                ys, xs = np.minimum(np.arange(y0, y0 + 256), h - 1), np.minimum(np.arange(x0, x0 + 256), w - 1)
                g, b = polyt[lv][np.ix_(ys, xs)], dapi[lv][np.ix_(ys, xs)]
                buf = io.BytesIO()
                Image.fromarray(np.stack([np.zeros_like(g), g, b], -1), mode="RGB").save(buf, format="JPEG", quality=QUALITY, subsampling=0)
                d = buf.getvalue()
                i = d.index(b"\xff\xda")
                yield ometiff.jpeg_tile_stream_rgb(d[i + 2 + int.from_bytes(d[i + 2:i + 4], "big"):-2])
    ometiff.write_tiles(path, state.shape[1], state.shape[2], tiles, "jpeg", ometiff.jpeg_tables_rgb(QUALITY), samples=3)


def gpu_export_rgb(state, odir):
    import torch
    from teramind_amd import stitch
    stitch.save_composites_pyramid(state, odir, slc=1, quality=QUALITY)
    torch.cuda.synchronize()


def end_to_end(reps, out, rgb=False):
    import torch
    import teramind_amd  # noqa: F401
    assert torch.cuda.is_available(), "bench_export needs a GPU"
    what = "colour composite (plane pair)" if rgb else "pyramidal OME-TIFF"
    unit = "plane pair" if rgb else "plane"
    res = {"what": f"{what} export, seconds per {unit}, profiler off", "quality": QUALITY, "reps": reps, "planes": []}
    gpu_route, host_route, name = (gpu_export_rgb, host_export_rgb, "rgb_0.tif") if rgb else (gpu_export, host_export, "all_0.tif")
    with tempfile.TemporaryDirectory() as tmp:
        for n in SIZES:
            state = synthetic_pair(n, "cuda:0") if rgb else synthetic_state(n, "cuda:0")
            gpu_route(state, os.path.join(tmp, "g"))                       # warm-up of both routes
            host_route(state, os.path.join(tmp, "h.tif"))
            same = open(os.path.join(tmp, "g", name), "rb").read() == open(os.path.join(tmp, "h.tif"), "rb").read()
            if rgb and not same:
                sys.exit(f"{n} x {n}: the GPU route and the host route wrote different files")
            tg, th = [], []
            for _ in range(reps):                                           # alternated
                t0 = time.perf_counter()
                gpu_route(state, os.path.join(tmp, "g"))
                t1 = time.perf_counter()
                host_route(state, os.path.join(tmp, "h.tif"))
                t2 = time.perf_counter()
                tg.append(t1 - t0)
                th.append(t2 - t1)
            r = {"plane": f"{n} x {n}", "file_bytes": os.path.getsize(os.path.join(tmp, "h.tif")),
                 "gpu_file_equals_host_file": same,
                 "gpu_s_median": round(statistics.median(tg), 4), "gpu_s_spread": round(max(tg) - min(tg), 4),
                 "host_s_median": round(statistics.median(th), 4), "host_s_spread": round(max(th) - min(th), 4)}
            r["host_over_gpu"] = round(r["host_s_median"] / r["gpu_s_median"], 2)
            res["planes"].append(r)
            del state
    # whole-brain plane: 286 x 414 tiles = 73216 x 105984 px, by pixel count from the larger measured plane
    big = res["planes"][-1]
    res["whole_brain_plane_s_EXTRAPOLATED"] = round(big["gpu_s_median"] * (73216 * 105984) / (SIZES[-1] ** 2), 1)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def profile(out_dir, reps):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import ometiff
    assert torch.cuda.is_available(), "bench_export needs a GPU"
    meta = {"exports": 1 + reps, "planes": []}
    with tempfile.TemporaryDirectory() as tmp:
        for n in SIZES:
            state = synthetic_state(n, "cuda:0")
            for _ in range(1 + reps):
                gpu_export(state, os.path.join(tmp, "g"))
            sizes = ometiff.pyramid_sizes(n, n)
            tiles = [((h + 255) // 256) * ((w + 255) // 256) for h, w in sizes]
            batches = sum((t + ometiff.BATCH_TILES - 1) // ometiff.BATCH_TILES for t in tiles)
            with open(os.path.join(tmp, "g", "all_0.tif"), "rb") as f:
                file_bytes = len(f.read())
            scan = file_bytes - sum(tiles) * 27 - 4096               # file minus tile markers and (about) the IFDs
            meta["planes"].append({"n": n, "levels": len(sizes), "tiles": sum(tiles), "pyramid_px": sum(h * w for h, w in sizes),
                                   "shrink_read": sum(h * w for h, w in sizes[:-1]), "shrink_write": sum(h * w for h, w in sizes[1:]),
                                   "scan_bytes": scan, "dispatches": {"u8_shrink2_kernel": len(sizes) - 1, "jpeg_tile_kernel": batches,
                                                                      "jpeg_offsets_kernel": batches, "jpeg_compact_kernel": batches}})
            del state
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "export_meta.json"), "w") as f:
        json.dump(meta, f)


def profile_rgb(out_dir, reps):
    """Under rocprofv3: per size the colour export of a plane pair 1 + reps times, then the grey export of one plane 1 + 3
    times.  Three grey planes are the 8 x 8 blocks one colour export transforms and codes."""
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import ometiff
    assert torch.cuda.is_available(), "bench_export needs a GPU"
    meta = {"exports": 1 + reps, "grey_exports": 1 + 3, "planes": []}
    with tempfile.TemporaryDirectory() as tmp:
        for n in SIZES:
            state = synthetic_pair(n, "cuda:0")
            for _ in range(1 + reps):
                gpu_export_rgb(state, os.path.join(tmp, "g"))
            for _ in range(1 + 3):
                gpu_export(state[:1], os.path.join(tmp, "g"))
            tiles = [((h + 255) // 256) * ((w + 255) // 256) for h, w in ometiff.pyramid_sizes(n, n)]
            meta["planes"].append({"n": n, "tiles": sum(tiles),
                                   "batches": sum((t + ometiff.BATCH_TILES - 1) // ometiff.BATCH_TILES for t in tiles)})
            del state
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "export_rgb_meta.json"), "w") as f:
        json.dump(meta, f)


def summarize_rgb(d):
    """Colour kernel time per export against three grey encodes of the same size, from the trace of profile_rgb."""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    meta = json.load(open(os.path.join(d, "export_rgb_meta.json")))
    per = {"jpeg_tile_rgb_kernel": [], "jpeg_tile_kernel": []}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].split("(")[0].replace("tmk::", "").replace("void ", "")
        if name in per:
            per[name].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    for name in per:
        per[name].sort()
    print("tile encoder kernel time per export (rocprofv3 --kernel-trace; warm-up export dropped)")
    print(f"{'plane':>6s} {'tiles':>6s} {'colour us (median)':>19s} {'spread':>8s} {'3 x grey us':>12s} {'colour / 3 grey':>16s} {'Mblocks/s colour':>17s}")
    used_c = used_g = 0
    for pl in meta["planes"]:
        k = pl["batches"]
        col = [sum(c[1] for c in per["jpeg_tile_rgb_kernel"][used_c + e * k: used_c + (e + 1) * k]) for e in range(meta["exports"])][1:]
        gre = [sum(c[1] for c in per["jpeg_tile_kernel"][used_g + e * k: used_g + (e + 1) * k]) for e in range(meta["grey_exports"])][1:]
        used_c += meta["exports"] * k
        used_g += meta["grey_exports"] * k
        cm, g3 = statistics.median(col), sum(gre)
        print(f"{pl['n']:6d} {pl['tiles']:6d} {cm:19.1f} {max(col) - min(col):8.1f} {g3:12.1f} {cm / g3:16.2f} {3072 * pl['tiles'] / cm:17.1f}")


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    meta = json.load(open(os.path.join(d, "export_meta.json")))
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].split("(")[0].replace("tmk::", "").replace("void ", "")
        per.setdefault(name, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    print("kernel times per exported plane (rocprofv3 --kernel-trace; median over the exports after the warm-up)")
    print(f"{'plane':>6s} {'kernel':22s} {'disp':>4s} {'us/plane':>10s} {'spread us':>10s} {'MB moved':>9s} {'GB/s':>8s} {'Gpx/s':>7s}")
    for name in per:
        per[name].sort()
    used = {k: 0 for k in per}
    for pl in meta["planes"]:
        for name, k in pl["dispatches"].items():
            calls = per.get(name, [])
            runs = []
            for e in range(meta["exports"]):
                chunk = calls[used[name] + e * k: used[name] + (e + 1) * k]
                if len(chunk) == k:
                    runs.append(sum(c[1] for c in chunk))
            used[name] = used.get(name, 0) + meta["exports"] * k
            if len(runs) < 2:
                print(f"{pl['n']:6d} {name:22s} not in the trace")
                continue
            runs = runs[1:]
            us = statistics.median(runs)
            moved = {"u8_shrink2_kernel": pl["shrink_read"] + pl["shrink_write"],
                     "jpeg_tile_kernel": 65536 * pl["tiles"] + pl["scan_bytes"],        # pixels in once, scan out
                     "jpeg_offsets_kernel": 12 * pl["tiles"],
                     "jpeg_compact_kernel": 2 * pl["scan_bytes"]}[name]
            px = pl["shrink_write"] if name == "u8_shrink2_kernel" else 65536 * pl["tiles"]
            print(f"{pl['n']:6d} {name:22s} {k:4d} {us:10.1f} {max(runs) - min(runs):10.1f} {moved / 1e6:9.2f} {moved / us / 1e3:8.1f} {px / us / 1e3:7.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="end-to-end mode: also write the JSON line here")
    ap.add_argument("--profile", default=None, metavar="DIR", help="run the exports only (under rocprofv3) and write DIR/export_meta.json")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    ap.add_argument("--rgb", action="store_true", help="the colour composite export of a plane pair (stitch.save_composites_pyramid) "
                    "against Pillow at 4:4:4 on the host; with --profile / --summarize: the colour tile kernel against three grey encodes")
    a = ap.parse_args()
    if a.summarize:
        (summarize_rgb if a.rgb else summarize)(a.summarize)
    elif a.profile:
        (profile_rgb if a.rgb else profile)(a.profile, a.reps)
    else:
        end_to_end(a.reps, a.out, a.rgb)
