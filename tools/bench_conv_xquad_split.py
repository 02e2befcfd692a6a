#!/usr/bin/env python3
"""Op-level timing of split K in the x-quad form (conv3d_xquad + xquad_split_reduce) against the unsplit x-quad launch and the
pair form, at the launches of the fp32 step that have fewer than 256 large x-quad workgroups and at the N = 400 shapes of the
deepest decoder level.  Per geometry ROUNDS rounds of CHUNK launches of every combination, interleaved, every launch (conv and,
when split, its reduction) between two events of its own (tm_op_conv_pad1_time_split_f32); the first launch of a chunk is
dropped.  Combinations: the pair form; the x-quad form at ksplit 1 / 2 / 4 in both schedules (s0 = four barriers per cin block,
s1 = pipelined), in the small tile where the launch has fewer than 256 large workgroups and in the launcher's tile otherwise (there
ksplit 1 and 2 only).  Prints one JSON line per geometry: median, 10th and 90th percentile in microseconds of each combination, the
fastest one and whether it beats `--incumbent` (default: the pair form) by the project's rule: its median lies below the
incumbent's by more than the larger of the two p90 - p10 widths.

    python3 tools/bench_conv_xquad_split.py [--rounds 5] [--chunk 21] [--geometry I] [--incumbent pair|k1_s0|...]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import teramind_amd  # noqa: E402,F401
from teramind_amd import _lib  # noqa: E402

# (N, Cin, Cout, S): the deepest decoder level at 32 collage patches (64 large workgroups, 128 small); the level-2 decoder blocks
# at S = 16 and the encoder's 256 -> 256 at S = 8 on 128 patches (128 large, 256 small); the deep shapes at the 400 patches of
# bench.py --tile (unsplit: pair against x-quad)
GEOMETRIES = [(32, 1253, 512, 8), (32, 512, 512, 8), (32, 997, 512, 8), (32, 896, 256, 16), (32, 640, 256, 16), (32, 512, 256, 16),
              (32, 256, 256, 16), (128, 256, 256, 8), (400, 1253, 512, 8), (400, 512, 512, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=21)
    ap.add_argument("--geometry", type=int, default=-1, help="index into GEOMETRIES (default: all)")
    ap.add_argument("--shape", type=int, nargs=4, default=None, metavar=("N", "CIN", "COUT", "S"), help="one geometry of your own")
    ap.add_argument("--incumbent", default="pair")
    a = ap.parse_args()
    L = _lib.lib()
    geos = [tuple(a.shape)] if a.shape else (GEOMETRIES if a.geometry < 0 else [GEOMETRIES[a.geometry]])
    for (N, Cin, Cout, S) in geos:
        g = torch.Generator(device="cuda").manual_seed(N + Cin + Cout + S)
        x = torch.randn((N, (Cin + 7) // 8, 2, S, S, 8), device="cuda", generator=g)
        y = torch.empty((N, (Cout + 7) // 8, 2, S, S, 8), device="cuda")
        w = (torch.randn((Cout, Cin, 27)) / (27 * Cin) ** 0.5).contiguous()
        b = torch.randn((Cout,))
        ms = (C.c_float * a.chunk)()
        large_wgs = (N * 2 * S * S // 1024) * 2 * ((Cout + 63) // 64)
        small = large_wgs < 256

        def run(form, tile, sched, ksplit):
            rc = L.tm_op_conv_pad1_time_split_f32(_lib.ptr(x), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), _lib.ptr(y), N, Cin,
                                                  Cout, S, form, tile, sched, ksplit, a.chunk, ms, _lib.current_stream_ptr())
            _lib.check(rc, "tm_op_conv_pad1_time_split_f32")
            return [1e3 * v for v in list(ms)[1:]]

        combos = {"pair": (0, 0, -1, 1)}
        for k in ((1, 2, 4) if small else (1, 2)):
            for s in (0, 1):
                combos["k%d_s%d" % (k, s)] = (2, 1 if small else 0, s, k)
        t = {k: [] for k in combos}
        for _ in range(a.rounds):
            for k, c in combos.items():
                t[k] += run(*c)
        q = {k: [float(np.percentile(t[k], p)) for p in (50, 10, 90)] for k in t}
        inc = a.incumbent
        best = min(combos, key=lambda k: q[k][0])
        width = max(q[best][2] - q[best][1], q[inc][2] - q[inc][1])
        out = {"N": N, "Cin": Cin, "Cout": Cout, "S": S, "launches": len(t["pair"]), "large_wgs": large_wgs,
               "rule_ksplit": L.tm_conv_xquad_ksplit(N, Cin, Cout, S, 0)}
        for k in combos:
            out[k + "_us"] = [round(v, 1) for v in q[k]]
        out["incumbent"] = inc
        out["best"] = best
        out["gap_us"] = round(q[inc][0] - q[best][0], 1)
        out["width_us"] = round(width, 1)
        out["best_wins"] = bool(best != inc and q[inc][0] - q[best][0] > width)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
