#!/usr/bin/env python3
"""Mints the rna_slc 16 training fixture FROM THE REFERENCE (test infrastructure; runs on the CPU where the reference is, like
tools/make_train_slc8_golden.py; no GPU test imports it):

  tests/golden/train_grad_slc16_ref.npz   the reference's own training_losses(...).backward() in float32, model in .eval() (no
      dropout), configuration train_slc16_cases.SLC16_CFG (net_ch 16, 37 genes, rna_slc 16: every conv at Z = 8, attention windows
      of 512 tokens at C = 64 and of 128 tokens at C = 128, down_z at kz = 9).  Format of train_grad_slc8_ref.npz: per parameter the
      L2 norm, GRAD_PROBES seeded projections and the whole gradient where it has at most GRAD_FULL_MAX elements.

Run:  python tools/make_train_slc16_golden.py"""
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
from train_cases import GRAD_FULL_MAX, GRAD_PROBES, grad_probe, make_inputs  # noqa: E402
from train_slc16_cases import SLC16_CASES, SLC16_CFG  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402


def mint_grad():
    cfg = PathConfig(**SLC16_CFG)
    conf = rh.make_conf(nrna=cfg.rna_num, net_ch=cfg.net_ch, srna=cfg.rna_slc)
    model = rh.make_model(conf)
    model.load_state_dict(hashed_state_dict(cfg, 0), strict=True)
    model.eval()
    out = {}
    for name, (seed, loss_type, (ix, iy)) in SLC16_CASES.items():
        sampler = rh.make_sampler(conf, 1000, "ddpm")
        from utils.choices import LossType
        sampler.loss_type = LossType.mse if loss_type == "mse" else LossType.l1
        x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed, C=cfg.n_stain * cfg.z_size, srna=cfg.rna_slc)
        draws = [ix, iy]
        real_tensor, real_rr = torch.tensor, random.randrange
        torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
        random.randrange = lambda *a, **k: draws.pop(0)
        model.zero_grad()
        try:
            terms = sampler.training_losses(model=model, x_start=x_pad, r_start=(rna[0].clone(), rna[1].clone(), rna[2]),
                                            imgs=imgs, t=t, pos=pos, loss_mask=mask, idx=idx, patch_size=64, noise=noise)
        finally:
            torch.tensor, random.randrange = real_tensor, real_rr
        assert not draws
        loss = terms["loss"].mean()
        loss.backward()
        out[f"{name}/loss"] = np.array(float(loss), dtype=np.float64)
        norms = []
        for k, p in model.named_parameters():
            g = p.grad.detach().double().reshape(-1).numpy()
            out[f"{name}/norm/{k}"] = np.array(np.linalg.norm(g))
            out[f"{name}/proj/{k}"] = np.array([float(g @ grad_probe(k, g.size, j)) for j in range(GRAD_PROBES)])
            if g.size <= GRAD_FULL_MAX:
                out[f"{name}/full/{k}"] = g.astype(np.float32).reshape(p.shape)
            norms.append(float(np.linalg.norm(g)))
        print(name, "loss", float(loss), "params", len(norms), "min/median/max grad norm", min(norms), sorted(norms)[len(norms) // 2],
              max(norms), flush=True)
    p = os.path.join(ROOT, "tests", "golden", "train_grad_slc16_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    mint_grad()
