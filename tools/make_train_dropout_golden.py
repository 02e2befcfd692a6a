#!/usr/bin/env python3
"""Mints tests/golden/train_grad_dropout_ref.npz FROM THE REFERENCE (test infrastructure; runs where the reference is, like the
oracle/make_*.py scripts; no GPU test runs it): the whole-model training objective and the gradient of every parameter, as
oracle/make_train_grad_golden.py mints them, but with the reference model in `.train()` and ResBlock dropout LIVE at p = 0.1.

The reference's nn.Dropout in every ResBlock's out_layers (model/MBAblocks.py:196-203; p = conf.dropout = 0.1,
config_parm.py:46) draws from torch's generator.  Here each of those modules is replaced by one that applies the keep mask of
DESIGN.md §8 (tests/dropout_rng.py, the rule the HIP kernels draw by) as `x * keep.div_(1 - p)` -- torch's own dropout
arithmetic with a pinned mask.  Its site is 2 j + k: j = the block's index in the sorted list of `*.out_layers.0.weight`
prefixes, k = the module's call count in the forward (0, then 1 for the plain pass of a decoder block; the reference runs the
collage pass first, model/unet_ours.py:396-425).  The other dropouts of the model are p = 0.

Same inputs, crop draws and output format as train_grad_ref.npz (tests/train_cases.py GRAD_*), plus `p`, `key` and `sites`.
Run:  python tools/make_train_dropout_golden.py"""
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import teramind_amd  # noqa: E402,F401
from oracle import ref_harness as rh  # noqa: E402
from dropout_rng import keep_mask  # noqa: E402
from train_cases import GRAD_CASES, GRAD_CFG, GRAD_FULL_MAX, GRAD_PROBES, grad_probe, make_inputs  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.train_model import dropout_sites  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402

P = 0.1
KEY = 0x5EED_D20F_0123_4567          # the fixture's dropout key (tests/test_gpu_train_dropout.py reads it back from the file)


class SiteDropout(nn.Module):
    """nn.Dropout(p) with the keep mask of DESIGN.md §8 at sites 2 j, 2 j + 1 (call 0, call 1 of one forward)."""

    def __init__(self, j, p, key):
        super().__init__()
        self.j, self.p, self.key, self.calls = j, p, key, 0

    def forward(self, x):
        assert self.training and x.dim() == 5 and x.shape[-1] == x.shape[-2], x.shape
        assert self.calls < 2, "a ResBlock ran more than twice in one forward"
        keep = torch.from_numpy(keep_mask(self.key, 2 * self.j + self.calls, self.p, tuple(x.shape))).to(x.dtype)
        self.calls += 1
        return x * keep.div_(1 - self.p)


def main():
    torch.set_num_threads(8)
    cfg = PathConfig(**GRAD_CFG)
    conf = rh.make_conf(nrna=cfg.rna_num, net_ch=cfg.net_ch)
    assert conf.dropout == P, conf.dropout
    assert conf.net_beatgans_gradient_checkpoint is False       # recomputation in backward would call the masks again
    model = rh.make_model(conf)
    sd = hashed_state_dict(cfg, 0)
    model.load_state_dict(sd, strict=True)
    model.train()                                               # make_model returns the model in .eval()
    sites = dropout_sites(sd.keys())
    repl = []
    for name, m in model.named_modules():
        if name in sites:
            assert m.conf.use_checkpoint is False, name
            d = m.out_layers[2]
            assert isinstance(d, nn.Dropout) and d.p == P, (name, d)
            m.out_layers[2] = SiteDropout(sites[name], P, KEY)
            repl.append(m.out_layers[2])
    assert len(repl) == len(sites), (len(repl), len(sites))
    for name, m in model.named_modules():
        if isinstance(m, nn.Dropout):
            assert m.p == 0.0, (name, m.p)                      # the attention / MLP dropouts
    out = {"p": np.array(P, dtype=np.float64), "key": np.array(KEY, dtype=np.uint64), "sites": np.array(len(sites), dtype=np.int64)}
    for name, (seed, loss_type, (ix, iy)) in GRAD_CASES.items():
        sampler = rh.make_sampler(conf, 1000, "ddpm")
        from utils.choices import LossType
        sampler.loss_type = LossType.mse if loss_type == "mse" else LossType.l1
        x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed)
        draws = [ix, iy]
        real_tensor, real_rr = torch.tensor, random.randrange
        torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
        random.randrange = lambda *a, **k: draws.pop(0)
        model.zero_grad()
        for r in repl:
            r.calls = 0
        try:
            terms = sampler.training_losses(model=model, x_start=x_pad, r_start=(rna[0].clone(), rna[1].clone(), rna[2]),
                                            imgs=imgs, t=t, pos=pos, loss_mask=mask, idx=idx, patch_size=64, noise=noise)
        finally:
            torch.tensor, random.randrange = real_tensor, real_rr
        assert not draws
        calls = sorted(r.calls for r in repl)
        assert set(calls) <= {1, 2} and 2 in calls, calls         # encoder / middle blocks once, decoder blocks twice
        before = [r.calls for r in repl]
        loss = terms["loss"].mean()
        loss.backward()
        assert [r.calls for r in repl] == before                  # nothing recomputed in the backward pass
        out[f"{name}/loss"] = np.array(float(loss), dtype=np.float64)
        for k, p in model.named_parameters():
            g = p.grad.detach().double().reshape(-1).numpy()
            out[f"{name}/norm/{k}"] = np.array(np.linalg.norm(g))
            out[f"{name}/proj/{k}"] = np.array([float(g @ grad_probe(k, g.size, j)) for j in range(GRAD_PROBES)])
            if g.size <= GRAD_FULL_MAX:
                out[f"{name}/full/{k}"] = g.astype(np.float32).reshape(p.shape)
        gn = {k: float(out[f"{name}/norm/{k}"]) for k, _ in model.named_parameters()}
        print(name, "loss", float(loss), "params", len(gn), "dropout calls", sum(calls), "min/median/max grad norm", min(gn.values()),
              sorted(gn.values())[len(gn) // 2], max(gn.values()), flush=True)
    p = os.path.join(ROOT, "tests", "golden", "train_grad_dropout_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
