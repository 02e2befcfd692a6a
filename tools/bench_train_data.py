#!/usr/bin/env python3
"""Measures the training batch draw (tm_train_batch_images + tm_train_batch_genes) at the checkpoint geometry: B = 32 crops of
256 px, snum 4, gblk 16, pdim 2, from synthetic resident tiles.  hipEvent times over `--reps` repeats after warm-up (median,
min, max); the image kernel's achieved bytes per second (1 B read + 4 B written per element) for rot 0 (row-wise loads) and
rot 1 (column-wise loads) beside the project's measured 1:4 read:write stream (profiles/r03_micro_hbm_rw.txt); the share of
one Trainer.step() that the draw takes.  Writes text to stdout (recorded in profiles/train_data.txt).
Run:  python tools/bench_train_data.py"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import teramind_amd  # noqa: E402,F401
from teramind_amd import synth  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.dataset import TrainGeometry, TrainTileSet  # noqa: E402
from teramind_amd.trainer import Trainer  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402

STREAM_1_4_GBS = 5306.9          # profiles/r03_micro_hbm_rw.txt, r:w 1:4, grid 65536


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--nnz", type=int, default=1_500_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step_batch", type=int, default=2)
    a = ap.parse_args()
    cfg = PathConfig()
    geo = TrainGeometry.from_config(cfg)
    imgs = [synth.image_tile(f"bench/img{i}", (2 * a.slices, a.size, a.size), 0) for i in range(a.tiles)]
    genes = [synth.train_gene_tile(f"bench/gene{i}", a.size, a.size, a.slices, a.nnz, 0) for i in range(a.tiles)]
    ts = TrainTileSet.from_arrays(imgs, genes, geo, "cuda:0", seed=0, repeat=max(1, 4 * a.batch // a.tiles))
    B = a.batch
    print(f"tiles: {a.tiles} x [{2 * a.slices}, {a.size}, {a.size}] uint8, {a.nnz} COO entries each (uniform, counts 1..3); "
          f"B = {B}, sdim {geo.sdim}, snum {geo.snum}, gblk {geo.gblk}, pdim {geo.pdim}; {a.reps} repeats after 5 warm-up calls")
    params = ts.sampler.params(B, 0)
    gp = geo.gs + 2 * geo.pdim
    img = torch.empty((B, geo.img_channels, geo.sdim, geo.sdim), device="cuda:0")
    rna = torch.empty((B, gp, gp, geo.snum * 500), device="cuda:0")
    med, lo, hi = timed(lambda: ts.gather(params, img=img, rna=rna), a.reps)
    print(f"draw (descriptor upload + both kernels, outputs preallocated): median {med:.3f} ms  min {lo:.3f}  max {hi:.3f}")
    med, lo, hi = timed(lambda: ts.draw(B, 0), a.reps)
    print(f"draw (as the trainer calls it, outputs from the caching allocator): median {med:.3f} ms  min {lo:.3f}  max {hi:.3f}")
    band = int(a.nnz * geo.sdim / a.size)
    print(f"  genes: {rna.numel() * 4 / 1e6:.1f} MB zero-filled, ~{band} entries read per sample (rows of the crop only)")
    # image kernel alone, through an entry-free set so that the gene call is the memset only; rot 0 vs rot 1
    from teramind_amd import _lib
    L, st = _lib.lib(), _lib.current_stream_ptr()
    nbytes = img.numel() * 5
    for rot in (0, 1):
        p = params.copy()
        p[:, 4], p[:, 5] = rot, 0
        host = torch.from_numpy(p).pin_memory()
        dev = host.to("cuda:0")
        fn = lambda: _lib.check(L.tm_train_batch_images(_lib.ptr(ts.img), 0, ts.n_tiles, ts.zt, ts.H, ts.W, _lib.ptr(dev), _lib.ptr(host), B,   # noqa: E731
                                                        geo.sdim, geo.snum, 0, _lib.ptr(img), st))
        med, lo, hi = timed(fn, a.reps)
        print(f"image kernel rot {rot}: median {med * 1e3:.1f} us  min {lo * 1e3:.1f}  max {hi * 1e3:.1f};  {nbytes / 1e6:.1f} MB moved -> "
              f"{nbytes / med / 1e6:.0f} GB/s = {100 * nbytes / med / 1e6 / STREAM_1_4_GBS:.1f} % of the 1:4 stream ({STREAM_1_4_GBS} GB/s)")
    # share of one optimizer step
    tr = Trainer(cfg, hashed_state_dict(cfg, 0), ts, a.step_batch, accum_batches=1, seed=0)
    tr.step()
    torch.cuda.synchronize()
    t0 = time.time()
    tr.step()
    torch.cuda.synchronize()
    step_s = time.time() - t0
    med, _, _ = timed(lambda: ts.draw(a.step_batch, 1), a.reps)
    print(f"Trainer.step() (default config, batch {a.step_batch}, 1 micro-batch): {step_s:.3f} s wall; its draw: {med:.3f} ms = "
          f"{100 * med / 1e3 / step_s:.3f} % of the step")


if __name__ == "__main__":
    main()
