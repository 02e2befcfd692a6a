#!/usr/bin/env python3
"""Bit-level digest of the forward executor, for comparing two builds of the library (TM_LIB_PATH selects the one under test):
an executor change that only moves host code must leave every line of the table as it was.

Per case -- the ten configuration points of tests/config_cases.CONFIGS plus the default (64, 4, "all", 229), in fp32, bf16 and
f16 wherever the model accepts the combination -- a synthetic model (tests/util.state_dict) runs b = 1 on a 2 x 2 patch grid
(four encoder patches, one decoder patch: the smallest grid with a collage decoder and an encoder-grid pred2) and one JSON line
records the SHA-256 of pred and pred2 from tm_unet_forward, from tm_unet_forward_rna on a tm_rna_pyramid buffer and from
tm_unet_forward_level0 on a tm_rna_level0 buffer, the SHA-256 of the weight arena, the workspace / pyramid / level-0 byte
counts, and the tm_profile_collect fields of one profiled forward (all but total_ms, a time).

    python tools/forward_digest.py [out.jsonl]        # default: standard output
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case, dtype):
    import torch
    import config_cases as cc
    import util
    from teramind_amd.unet import BeatGANsUNetModel
    rec = {"case": cc.tag_of(case), "dtype": dtype}
    cfg = cc.path_config(case, compute_dtype=dtype)
    try:
        m = BeatGANsUNetModel(cfg, "cuda:0")
    except RuntimeError as e:                     # the model refuses the combination (16-bit modes at patch size 32)
        rec["refused"] = str(e)
        return rec
    m.load_state_dict(util.state_dict(cc.path_config(case)))
    x, rna, t = (v.to("cuda:0") for v in cc.inputs(cfg))
    imgs = torch.empty((1, cfg.in_channels, cfg.patch_size, cfg.patch_size), device="meta")
    kw = dict(x=x, t=t, imgs=imgs, patch_size=cfg.patch_size, want_pred2=True)
    sources = {"forward": rna, "forward_rna": m.precompute_rna(rna, 1, imgs=imgs, patch_size=cfg.patch_size),
               "forward_level0": m.precompute_rna_level0(rna, 1, imgs=imgs, patch_size=cfg.patch_size)}
    for name, src in sources.items():
        out = m(rna=src, **kw)
        torch.cuda.synchronize()
        rec[name] = {"pred": sha(out.pred), "pred2": sha(out.pred2)}
    rec["arena"] = sha(m.arena())
    L, h = m._L, m._h
    rec["bytes"] = {"workspace": L.tm_workspace_bytes(h, 1, 2, 2, 0), "workspace_pred2": L.tm_workspace_bytes(h, 1, 2, 2, 1),
                    "pyramid": L.tm_rna_pyramid_bytes(h, 1, 2, 2), "level0": L.tm_rna_level0_bytes(h, 1, 2, 2)}
    m.profile(True)
    m(rna=rna, **kw)
    prof = m.profile_collect()
    m.profile(False)
    prof.pop("total_ms")
    rec["profile"] = prof
    return rec


def main():
    import config_cases as cc
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    for case in cc.CONFIGS + [(64, 4, "all", 229)]:
        for dtype in ("f32", "bf16", "f16"):
            print(json.dumps(run_case(case, dtype), sort_keys=True), file=out, flush=True)


if __name__ == "__main__":
    main()
