#!/usr/bin/env python3
"""Reading a step directory on one MI355X: TileSweep.load_step of a 4 x 8-tile state (32 tiles of float16 [100, 256, 256])
with decoder "host" (tm_blosc_decompress per chunk, then a copy of the plain tile) and "gpu" (the chunk members copied as
they are, tm_blosc_decompress_tiles into the canvas).  The read-side twin of tools/bench_snapshot.py, on its canvas: every
tile half constant background, half smooth signal with noisy low mantissa bits.

Two directories:
  ours       written once by save_step(compressor="blosc"): one chunk per tile, block size 65536, 400 streams of 32 KiB
  reference  the chunking zarr gives the reference's tiles, [25, 64, 128] chunks (32 per tile) framed at block size 262144 as
             c-blosc frames chunks of that size: ONE tile is minted with the Python frame encoder of tests/blosc_cases.py
             (streams by the run encoder of tests/blosc_decode_cases.py: too slow for 32 different tiles) and the file is
             replicated under the 32 tile names.  The chunking is derived from zarr's rule, not read from a real file.

The two routes are alternated in one process, median of --reps calls after one warm-up each, spread = max - min of identical
calls.  The files are warm in the page cache (written moments before, read once by the warm-up): the figures are decode and
copy time, not disk time.  The decoder call alone (memset of the status, the two tables, the decode and the unshuffle
kernels) is timed by hipEvents around tm_blosc_decompress_tiles in the same calls."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HNM, WNM, SLC = 4, 8, 50
TILE_BYTES = 2 * SLC * 256 * 256 * 2
REF_CHUNKS, REF_BLOCK = (25, 64, 128), 262144
WHOLE_BRAIN_RANK_TILES = 14904


def mint_reference_dir(sw, d):
    """One tile of the canvas in the reference's chunking, replicated under every tile name of the sweep."""
    import json
    import zipfile
    import blosc_cases as bc
    import blosc_decode_cases as dc
    from teramind_amd import tiles
    a = sw.tile(0, 0).half().cpu().numpy()
    meta = {"chunks": list(REF_CHUNKS), "compressor": {"blocksize": 0, "clevel": 5, "cname": "lz4", "id": "blosc", "shuffle": 1}, "dtype": "<f2",
            "fill_value": 0.0, "filters": None, "order": "C", "shape": list(a.shape), "zarr_format": 2}
    os.makedirs(d, exist_ok=True)
    first = None
    for lr in range(sw.nrows):
        for c in range(sw.wnm):
            path = os.path.join(d, tiles.state_tile_name(sw.row0 + sw.r0 + lr, sw.col0 + c) + ".zip")
            if first is not None:
                shutil.copyfile(first, path)
                continue
            with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as z:
                z.writestr(".zarray", json.dumps(meta, indent=4, sort_keys=True))
                for i in range(a.shape[0] // REF_CHUNKS[0]):
                    for j in range(a.shape[1] // REF_CHUNKS[1]):
                        for k in range(a.shape[2] // REF_CHUNKS[2]):
                            blk = a[i * 25:(i + 1) * 25, j * 64:(j + 1) * 64, k * 128:(k + 1) * 128]
                            z.writestr(f"{i}.{j}.{k}", bc.encode_frame(blk.tobytes(), 2, REF_BLOCK, lz4=dc.lz4_runs))
            first = path
    return a


def measure(sw, base, epoch, reps, label, lines):
    import torch
    from teramind_amd import formats
    times, kern = {"host": [], "gpu": []}, []
    state = {}
    for rep in range(reps + 1):                                      # rep 0 warms both routes (and the page cache) up
        for route in ("host", "gpu"):                                # alternated
            formats.decode_timings = [] if route == "gpu" else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sw.load_step(base, epoch, decoder=route)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[route].append(dt)
                if route == "gpu":
                    kern.append(sum(t[0] for t in formats.decode_timings))
            if route == "gpu":
                calls, frames, fbytes = len(formats.decode_timings), sum(t[1] for t in formats.decode_timings), sum(t[2] for t in formats.decode_timings)
            state[route] = sw.cur.clone()
            formats.decode_timings = None
    ntiles = HNM * WNM
    same = bool(torch.equal(state["host"], state["gpu"]))
    med = {k: statistics.median(v) for k, v in times.items()}
    spr = {k: max(v) - min(v) for k, v in times.items()}
    lines.append(f"-- {label}: {ntiles} tiles, {frames} frames, {fbytes / 1e6:.1f} MB of frames for {ntiles * TILE_BYTES / 1e6:.1f} MB plain; "
                 f"decode_fallbacks {sw.decode_fallbacks}; canvases of the two routes equal: {same}")
    lines.append(f"{'route':6s} {'s/load':>9s} {'spread s':>9s} {'ms/tile':>8s}")
    for k in ("host", "gpu"):
        lines.append(f"{k:6s} {med[k]:9.3f} {spr[k]:9.3f} {1e3 * med[k] / ntiles:8.2f}")
    kmed = statistics.median(kern)
    lines.append(f"decoder call alone (hipEvents around tm_blosc_decompress_tiles, {calls} call(s) per load): {kmed:.2f} ms per load "
                 f"(spread {max(kern) - min(kern):.2f}), {kmed / ntiles:.3f} ms per tile, {ntiles * TILE_BYTES / kmed / 1e6:.1f} GB/s of plain bytes")
    gain, need = med["host"] - med["gpu"], spr["host"] + spr["gpu"]
    lines.append(f"host - gpu = {gain:.3f} s per load ({1e3 * gain / ntiles:.2f} ms per tile), sum of the two spreads {need:.3f} s: "
                 + ("the GPU route is faster by more than the spreads" if gain > need else "NOT faster beyond the spreads"))
    lines.append(f"EXTRAPOLATED to one rank's share of the brain ({WHOLE_BRAIN_RANK_TILES} tiles) by tile count, not measured: host "
                 f"{med['host'] / ntiles * WHOLE_BRAIN_RANK_TILES / 60:.1f} min, gpu {med['gpu'] / ntiles * WHOLE_BRAIN_RANK_TILES / 60:.1f} min per load")
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--skip_reference", action="store_true", help="only the directory save_step writes")
    a = ap.parse_args()
    from bench_snapshot import synthetic_sweep
    sw = synthetic_sweep()
    lines = [f"load_step of a {HNM} x {WNM}-tile state ({HNM * WNM} tiles, {TILE_BYTES / 1e6:.1f} MB each as float16), profiler off, routes alternated in "
             f"one process, median of {a.reps} after a warm-up; spread = max - min of identical calls; files warm in the page cache"]
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        want = sw.cur.clone()
        sw.save_step(os.path.join(tmp, "ours"), compressor="blosc")
        ok &= measure(sw, os.path.join(tmp, "ours"), 1, a.reps, "ours (one chunk per tile, block size 65536)", lines)
        ok &= bool((sw.cur == want).all())
        if not a.skip_reference:
            t0 = time.perf_counter()
            tile = mint_reference_dir(sw, sw.step_dir(os.path.join(tmp, "ref"), 1))
            lines.append(f"(minted one tile in [25, 64, 128] chunks at block size {REF_BLOCK} and replicated it 32 times in {time.perf_counter() - t0:.1f} s)")
            ok &= measure(sw, os.path.join(tmp, "ref"), 1, a.reps, "reference chunking ([25, 64, 128] chunks, block size 262144; one tile replicated)", lines)
            import torch
            ok &= bool(torch.equal(sw.tile(3, 7).half().cpu(), torch.from_numpy(tile)))
    lines.append(f"every load gave the expected canvas: {ok}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
