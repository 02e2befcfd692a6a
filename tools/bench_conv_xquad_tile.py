#!/usr/bin/env python3
"""Op-level timing of the two tiles of the x-quad form (conv3d_xquad: 1 = 64 four-column groups on four waves, two workgroups per
CU; 2 = 128 groups on eight waves, one per CU) in both schedules (s0 = four barriers per cin block, s1 = pipelined), at the
geometries of tools/bench_conv_xquad.py and at (128, 64, 64, 64).  Per geometry ROUNDS rounds of CHUNK launches of each of the
four (tile, schedule) combinations, interleaved, every launch between two events of its own (tm_op_conv_pad1_time_sched_f32); the
first launch of a chunk is dropped.  Prints one JSON line per geometry: median, 10th and 90th percentile in microseconds of each
combination, the combination the launcher takes on its own (`incumbent`), the fastest one (`best`) and whether it wins by the
project's rule: its median lies below the incumbent's by more than the larger of the two p90 - p10 widths.

    python3 tools/bench_conv_xquad_tile.py [--rounds 5] [--chunk 21] [--geometry I]
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

GEOMETRIES = [(128, 64, 64, 64), (128, 96, 64, 64), (128, 128, 128, 32), (128, 256, 256, 16), (128, 512, 512, 8), (32, 1253, 512, 8),
              (32, 512, 256, 16), (32, 160, 64, 64), (32, 512, 512, 8)]
COMBOS = [(1, 0), (1, 1), (2, 0), (2, 1)]            # (tile, schedule)


def name(k):
    return "t%d_s%d" % k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=21)
    ap.add_argument("--geometry", type=int, default=-1, help="index into GEOMETRIES (default: all)")
    a = ap.parse_args()
    L = _lib.lib()
    geos = GEOMETRIES if a.geometry < 0 else [GEOMETRIES[a.geometry]]
    for (N, Cin, Cout, S) in geos:
        g = torch.Generator(device="cuda").manual_seed(N + Cin + Cout + S)
        x = torch.randn((N, (Cin + 7) // 8, 2, S, S, 8), device="cuda", generator=g)
        y = torch.empty((N, (Cout + 7) // 8, 2, S, S, 8), device="cuda")
        w = (torch.randn((Cout, Cin, 27)) / (27 * Cin) ** 0.5).contiguous()
        b = torch.randn((Cout,))
        ms = (C.c_float * a.chunk)()

        def run(tile, sched):
            rc = L.tm_op_conv_pad1_time_sched_f32(_lib.ptr(x), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), _lib.ptr(y), N, Cin,
                                                  Cout, S, 2, tile, sched, a.chunk, ms, _lib.current_stream_ptr())
            _lib.check(rc, "tm_op_conv_pad1_time_sched_f32")
            return [1e3 * v for v in list(ms)[1:]]

        t = {k: [] for k in COMBOS}
        auto = []                                    # the launcher's own choice of tile and schedule
        for _ in range(a.rounds):
            for k in COMBOS:
                t[k] += run(*k)
            auto += run(0, -1)
        q = {k: [float(np.percentile(t[k], p)) for p in (50, 10, 90)] for k in t}
        qa = [float(np.percentile(auto, p)) for p in (50, 10, 90)]
        tile_auto = L.tm_op_conv_xquad_f32(_lib.ptr(x), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), _lib.ptr(y), C.c_void_p(0), 0,
                                           N, Cin, Cout, 2, S, 0, _lib.current_stream_ptr())
        if tile_auto < 0:
            _lib.check(tile_auto, "tm_op_conv_xquad_f32")
        # the launcher's tile as the hook reports it; of its two schedules the one whose median the launcher's own run matches
        inc = min([k for k in COMBOS if k[0] == tile_auto], key=lambda k: abs(q[k][0] - qa[0]))
        best = min(COMBOS, key=lambda k: q[k][0])
        width = max(q[best][2] - q[best][1], q[inc][2] - q[inc][1])
        out = {"N": N, "Cin": Cin, "Cout": Cout, "S": S, "launches": len(auto), "large_wgs": (N * S * S // 512) * ((Cout + 31) // 32)}
        for k in COMBOS:
            out[name(k) + "_us"] = [round(v, 1) for v in q[k]]
        out["auto_us"] = [round(v, 1) for v in qa]
        out["incumbent"] = name(inc)
        out["best"] = name(best)
        out["gap_us"] = round(q[inc][0] - q[best][0], 1)
        out["width_us"] = round(width, 1)
        out["best_wins"] = bool(best != inc and q[inc][0] - q[best][0] > width)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
