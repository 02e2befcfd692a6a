#!/usr/bin/env python3
"""Op-level timing of the fp32 3x3x3 pad-1 conv at Z = 2 in its two forms, the pair form (conv3d_zpair) and the x-quad form
(conv3d_xquad, F(4,3) along x), at the governing geometries of the fp32 step.  Per geometry ROUNDS rounds of CHUNK launches of
each form, interleaved (pair, x-quad s0, x-quad s1, pair, ..), every launch between two events of its own
(tm_op_conv_pad1_time_sched_f32); the first launch of a chunk is dropped.  Prints one JSON line per geometry: median, 10th and
90th percentile in microseconds of each form -- the x-quad form once per schedule of conv3d_xquad (s0 = four barriers per cin
block, s1 = pipelined) -- xquad_ratio, the better x-quad median over the pair form's, and xquad_wins, whether it is below the pair
form's by more than the largest of the p90 - p10 spreads; pipe_wins: schedule 1 against schedule 0 by the same rule on their two
widths.

    python3 tools/bench_conv_xquad.py [--rounds 5] [--chunk 21] [--tile 0]
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

# (N, Cin, Cout, S): the four encoder / decoder levels of configs[1] at b = 32, P = 1, the widest decoder concat, the deepest
# decoder's second conv and the shallowest decoder's
GEOMETRIES = [(128, 96, 64, 64), (128, 128, 128, 32), (128, 256, 256, 16), (128, 512, 512, 8), (32, 1253, 512, 8),
              (32, 512, 256, 16), (32, 160, 64, 64), (32, 512, 512, 8)]
NAMES = {0: "pair", 3: "xquad_s0", 4: "xquad_s1"}   # 3 | 4: the timing hook's form 2 with schedule 0 | 1 forced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=21)
    ap.add_argument("--tile", type=int, default=0)
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
        t = {f: [] for f in NAMES}
        for _ in range(a.rounds):
            for form in NAMES:
                rc = L.tm_op_conv_pad1_time_sched_f32(_lib.ptr(x), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), _lib.ptr(y), N,
                                                      Cin, Cout, S, min(form, 2), a.tile, form - 3 if form > 2 else -1, a.chunk, ms,
                                                      _lib.current_stream_ptr())
                _lib.check(rc, "tm_op_conv_pad1_time_sched_f32")
                t[form] += [1e3 * v for v in list(ms)[1:]]
        q = {f: [float(np.percentile(t[f], p)) for p in (50, 10, 90)] for f in t}
        spread = max(q[f][2] - q[f][1] for f in q)
        out = {"N": N, "Cin": Cin, "Cout": Cout, "S": S, "tile": a.tile, "launches": len(t[0])}
        for f, name in NAMES.items():
            out[name + "_us"] = [round(v, 1) for v in q[f]]
        xq = min(q[3][0], q[4][0])
        out["xquad_ratio"] = round(xq / q[0][0], 4)
        out["pipe_ratio"] = round(q[4][0] / q[3][0], 4)
        out["spread_us"] = round(spread, 1)
        out["xquad_wins"] = bool(q[0][0] - xq > spread)
        out["pipe_wins"] = bool(q[3][0] - q[4][0] > max(q[3][2] - q[3][1], q[4][2] - q[4][1]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
