#!/usr/bin/env python3
"""One whole-model training step (loss + all gradients) of the tiny configuration of tests/train_cases.py (GRAD_CFG), for a
kernel trace of ResBlock dropout three ways:
    --mode p0        dropout_p = 0 (the eval-mode step)
    --mode drawn     dropout_p = 0.1, keep masks drawn in the prep kernels (tm_op_prep_train_rng / tm_op_prep_bwd_rng)
    --mode supplied  dropout_p = 0.1, the same masks materialised (tm_op_dropout_mask) and passed to the supplied-mask ops
                     (tm_op_prep_train / tm_op_prep_bwd): 4 more bytes read per element in each pass
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -o <mode> -- python3 tools/train_step_profile.py --mode <mode>
The drawn and the supplied step compute the same bits (printed loss)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import teramind_amd  # noqa: E402,F401
from teramind_amd import _lib  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.diffusion import SpacedDiffusionBeatGans  # noqa: E402
from teramind_amd.train_model import UNetTrain, _V, training_loss_and_grads  # noqa: E402
from teramind_amd.training import _hp  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402
from train_cases import GRAD_CASES, GRAD_CFG, make_inputs  # noqa: E402


class SuppliedMaskUNetTrain(UNetTrain):
    """UNetTrain whose dropout preps take a materialised fp32 CB8 mask (kept alive until the backward) instead of drawing it."""

    def prep(self, x, key, ss=None, per_image=1, drop=None):
        if drop is None:
            return super().prep(x, key, ss, per_image)
        dkey, site, p = drop
        N, Z, S = self._geo(x.t)
        L, st = _lib.lib(), self._st()
        mask = torch.empty_like(x.t)
        _lib.check(L.tm_op_dropout_mask(dkey, site, p, _lib.ptr(mask), N, x.C, Z, S, st), "tm_op_dropout_mask")
        ds = 1.0 / (1.0 - p)
        nw = self.W[key].reshape(-1)
        sc = sh = None
        if ss is not None:
            h = ss.t.to("cpu")
            sc, sh = h[:, :x.C].contiguous(), h[:, x.C:].contiguous()
        y = torch.empty_like(x.t)
        _lib.check(L.tm_op_prep_train(_lib.ptr(x.t), _hp(nw), _hp(sc), _hp(sh), _lib.ptr(mask), ds, per_image, _lib.ptr(y), N, x.C, Z, S, st),
                   "tm_op_prep_train")
        out = _V(y, x.C)

        def bwd():
            dx = torch.empty_like(x.t)
            nimg = (N + per_image - 1) // per_image
            dw = torch.empty((x.C,), dtype=torch.float32)
            dsc = torch.empty((nimg, x.C), dtype=torch.float32) if ss is not None else None
            dsh = torch.empty((nimg, x.C), dtype=torch.float32) if ss is not None else None
            _lib.check(L.tm_op_prep_bwd(_lib.ptr(x.t), _lib.ptr(out.g), _hp(nw), _hp(sc), _hp(sh), _lib.ptr(mask), ds, per_image, _lib.ptr(dx),
                                        _hp(dw), _hp(dsc), _hp(dsh), N, x.C, Z, S, self._st()), "tm_op_prep_bwd")
            self._gacc(key, dw)
            self._acc(x, dx)
            if ss is not None:
                self._acc(ss, torch.cat([dsc, dsh], dim=1).to(self.dev))
        self.tape.append(bwd)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("p0", "drawn", "supplied"), required=True)
    ap.add_argument("--key", type=lambda s: int(s, 0), default=0x5EEDD20F01234567)
    a = ap.parse_args()
    seed, loss_type, crop = GRAD_CASES["mse_seed3"]
    cfg = PathConfig(**GRAD_CFG)
    p = 0.0 if a.mode == "p0" else 0.1
    net = (SuppliedMaskUNetTrain if a.mode == "supplied" else UNetTrain)(cfg, hashed_state_dict(cfg, 0), "cuda:0", dropout_p=p)
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    loss, grads = training_loss_and_grads(net, sampler, x_pad, rna, t, mask, noise, crop, cfg.patch_size, loss_type, dropout_key=a.key)
    torch.cuda.synchronize()
    gsum = sum(float(g.double().abs().sum()) for g in grads.values())
    print(f"mode {a.mode}: loss {loss!r}  sum|grad| {gsum!r}")


if __name__ == "__main__":
    main()
