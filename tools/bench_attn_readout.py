#!/usr/bin/env python3
"""One-tile timing of the attention read-out (checkpoint config, b = 1 -> B = 625 patches, GLUT): attn_maps.run_attn_batch
through the four maps (tm_gene_attn + torch gather, `unfused`) against the fused kernel (tm_gene_attn_readout, `fused`).
hipEvent-timed after warm-up, the two paths alternating in rounds inside one process; the spread is that of the rounds of
identical calls.  `--mode fused|unfused` runs one path only (for a kernel trace of its own).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["both", "fused", "unfused"], default="both")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls per round and path")
    ap.add_argument("--path", default="GLUT")
    args = ap.parse_args()
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import synth
    from teramind_amd.attn_maps import PATHWAYS, run_attn_batch
    from teramind_amd.config import PathConfig
    from teramind_amd.unet import GeneAttnModel
    from teramind_amd.weights import hashed_state_dict

    dev = torch.device("cuda", 0)
    cfg = PathConfig()
    m = GeneAttnModel(cfg, dev).load_state_dict(hashed_state_dict(cfg, 0, vis_only=True), strict=False)
    tile = synth.gene_counts("attn/tile", (1, 20, 20, 26000), 0, density=0.05).to(dev)
    glst = PATHWAYS[args.path]
    modes = ["unfused", "fused"] if args.mode == "both" else [args.mode]
    outs = {}
    for md in modes:                                              # warm-up: code objects, allocator, workspaces
        for _ in range(3):
            outs[md] = run_attn_batch(m, tile, glst, fused=(md == "fused"))
    torch.cuda.synchronize()
    ms = {md: [] for md in modes}
    for _ in range(args.rounds):
        for md in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                run_attn_batch(m, tile, glst, fused=(md == "fused"))
            e1.record()
            e1.synchronize()
            ms[md].append(e0.elapsed_time(e1) / args.reps)
    res = {"what": "run_attn_batch, one 256-px tile (B = 625 patches), ms per call, hipEvent", "glst": list(glst),
           "rounds": args.rounds, "reps": args.reps}
    for md in modes:
        v = sorted(ms[md])
        res[md] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                   "rounds_ms": [round(x, 4) for x in ms[md]]}
    if len(modes) == 2:
        res["speedup_median"] = round(res["unfused"]["median_ms"] / res["fused"]["median_ms"], 2)
        res["max_abs_diff_fp16_tiles"] = float((outs["fused"].float() - outs["unfused"].float()).abs().max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
