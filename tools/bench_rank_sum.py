#!/usr/bin/env python3
"""Times rank_sum_kernel, the only arithmetic of the data-parallel gradient exchange (teramind_amd.train_dist), through the
library's own hook tm_op_rank_sum_time: random device data, one warm-up launch, `--reps` repetitions of `--iters` launches between
two events.  Per W: the shard a rank reduces at the checkpoint arena (--arena floats / W, rounded as train_dist.shard_layout
does), the median of the repetitions, their spread (max - min) and the rate over the (W + 1) * 4 bytes per element the kernel
must move.  One JSON line per W.

    python tools/bench_rank_sum.py --worlds 2 4 8"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import teramind_amd  # noqa: E402,F401
from teramind_amd import _lib  # noqa: E402
from teramind_amd.train_dist import shard_layout  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena", type=int, default=213_800_000, help="floats of the gradient arena (checkpoint configuration: 213.8 M)")
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    for W in a.worlds:
        n, _ = shard_layout(a.arena, W)
        ms = (C.c_float * a.reps)()
        _lib.check(_lib.lib().tm_op_rank_sum_time(W, n, a.iters, a.reps, C.cast(ms, C.c_void_p), None), "tm_op_rank_sum_time")
        t = sorted(float(v) for v in ms)
        med = statistics.median(t)
        nbytes = (W + 1) * 4 * n
        print(json.dumps({"W": W, "n": n, "bytes": nbytes, "ms_median": round(med, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                          "spread_ms": round(t[-1] - t[0], 4), "GBps_median": round(nbytes / med / 1e6, 1), "iters": a.iters, "reps": a.reps}),
              flush=True)


if __name__ == "__main__":
    main()
