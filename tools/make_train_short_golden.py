#!/usr/bin/env python3
"""Mints the two short-window training fixtures FROM THE REFERENCE (test infrastructure; runs on the CPU where the reference is,
like the oracle/make_*.py scripts; no GPU test imports it):

  tests/golden/train_grad_short_ref.npz   the reference's own training_losses(...).backward() in float32, model in .eval() (no
      dropout), for the tiny model (net_ch 16, 37 genes) at the three configurations of train_short_cases.GRAD_SHORT_CASES:
      rna_slc 1 / patch 64 (middle-block windows of 16 tokens, every conv at Z = 1, down_z at kz = 1), rna_slc 4 / patch 32
      (windows of 8 tokens, S = 4 planes, 2 x 2 gene grid) and rna_slc 4 / patch 128 (S = 128 planes, 8 x 8 gene grid).  Content of
      train_grad_ref.npz: per parameter the L2 norm, GRAD_PROBES seeded projections and the whole gradient where it has at most
      GRAD_FULL_MAX elements; the norms and projections of a case are packed into one array each, in the order of "<case>/keys"
      (three cases of one zip member per number would pass the size limit of a committed file).
  tests/golden/train_attn_short_ref.npz   the reference AttnBlock in float64 at windows of 4 tokens (Z = 1, S = 4) and of 16
      tokens from four planes (Z = 4, S = 4), C = 32, G = 20, as oracle/make_train_block_golden.py mints train_attn_ref.npz: out,
      dx, dcond and all 18 parameter gradients, stored as float32.

Run:  python tools/make_train_short_golden.py"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import teramind_amd  # noqa: E402,F401
from oracle import ref_harness as rh  # noqa: E402
from train_cases import GRAD_FULL_MAX, GRAD_PROBES, grad_probe  # noqa: E402
from train_short_cases import ATTN_SHORT_CASES, GRAD_SHORT_CASES, make_attn_short_inputs, make_short_inputs  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402


def mint_grad():
    out = {}
    for name in GRAD_SHORT_CASES:
        over, loss_type, (ix, iy), (x_pad, rna, imgs, t, pos, mask, idx, noise) = make_short_inputs(name)
        cfg = PathConfig(**over)
        conf = rh.make_conf(size=cfg.patch_size, nrna=cfg.rna_num, net_ch=cfg.net_ch, srna=cfg.rna_slc)
        model = rh.make_model(conf)
        model.load_state_dict(hashed_state_dict(cfg, 0), strict=True)
        model.eval()
        sampler = rh.make_sampler(conf, 1000, "ddpm")
        from utils.choices import LossType
        sampler.loss_type = LossType.mse if loss_type == "mse" else LossType.l1
        draws = [ix, iy]
        real_tensor, real_rr = torch.tensor, random.randrange
        torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
        random.randrange = lambda *a, **k: draws.pop(0)
        model.zero_grad()
        try:
            terms = sampler.training_losses(model=model, x_start=x_pad, r_start=(rna[0].clone(), rna[1].clone(), rna[2]),
                                            imgs=imgs, t=t, pos=pos, loss_mask=mask, idx=idx, patch_size=cfg.patch_size, noise=noise)
        finally:
            torch.tensor, random.randrange = real_tensor, real_rr
        assert not draws
        loss = terms["loss"].mean()
        loss.backward()
        out[f"{name}/loss"] = np.array(float(loss), dtype=np.float64)
        keys, norms, projs = [], [], []
        for k, p in model.named_parameters():
            g = p.grad.detach().double().reshape(-1).numpy()
            keys.append(k)
            norms.append(float(np.linalg.norm(g)))
            projs.append([float(g @ grad_probe(k, g.size, j)) for j in range(GRAD_PROBES)])
            if g.size <= GRAD_FULL_MAX:
                out[f"{name}/full/{k}"] = g.astype(np.float32).reshape(p.shape)
        out[f"{name}/keys"] = np.array(keys)
        out[f"{name}/norm"] = np.array(norms, dtype=np.float64)
        out[f"{name}/proj"] = np.array(projs, dtype=np.float64)
        print(name, "loss", float(loss), "params", len(norms), "min/median/max grad norm", min(norms), sorted(norms)[len(norms) // 2],
              max(norms), flush=True)
    p = os.path.join(ROOT, "tests", "golden", "train_grad_short_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


def mint_attn():
    rh.load()
    from model.MBAblocks import AttnBlock
    out = {}
    for name, c in ATTN_SHORT_CASES.items():
        x, cond, dout, params = make_attn_short_inputs(name)
        blk = AttnBlock(c["C"], num_heads=1, enable_flash_attn=True, gene_trans=True, gene_size=c["G"], z_size=c["Z"], n_h=2).double()
        blk.load_state_dict({k: v.double() for k, v in params.items()}, strict=True)
        blk.train()
        xx, cc = x.double().requires_grad_(True), cond.double().requires_grad_(True)
        y = blk(xx, None, cc)
        (y * dout.double()).sum().backward()
        out[f"{name}/out"] = y.detach().float().numpy()
        out[f"{name}/dx"] = xx.grad.float().numpy()
        out[f"{name}/dcond"] = cc.grad.float().numpy()
        for k, p in blk.named_parameters():
            out[f"{name}/grad/{k}"] = p.grad.float().numpy()
        print(name, "out", float(y.abs().mean()), "dx", float(xx.grad.abs().mean()), "dcond", float(cc.grad.abs().mean()), flush=True)
    p = os.path.join(ROOT, "tests", "golden", "train_attn_short_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    mint_attn()
    mint_grad()
