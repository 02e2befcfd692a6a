"""-m gpu: training at the configurations whose middle-block AttnBlock has short windows, and at patch size 128.

  * training.AttnBlockTrain at windows of 4 tokens (Z 1, S 4) and of 16 tokens from four planes (Z 4, S 4) against the reference
    module in float64 (tests/golden/train_attn_short_ref.npz), relative L2 < 1e-4 per tensor as tests/test_gpu_train.py asks;
  * the whole step for rna_slc 1 / patch 64, rna_slc 4 / patch 32 and rna_slc 4 / patch 128 against the reference's own
    training_losses(...).backward() (tests/golden/train_grad_short_ref.npz) with the bounds of tests/test_gpu_train_model.py, host
    and resident engine, every bit reproduced by a second run;
  * the Trainer on a synthetic rna_slc 4 / patch 32 tile directory, with dropout, on both engines: 2 steps equal
    1 + save + resume + 1;
  * rna_slc 1 at patch size 32 is refused in the constructor, with the reason.
Both fixtures are minted by tools/make_train_short_golden.py."""
import os

import numpy as np
import pytest
import torch

from train_cases import GRAD_FULL_MAX, GRAD_PROBES, grad_probe
from train_short_cases import ATTN_SHORT_CASES, GRAD_SHORT_CASES, make_attn_short_inputs, make_short_inputs
from teramind_amd import synth
from teramind_amd.config import PathConfig
from teramind_amd.dataset import TrainTileSet
from teramind_amd.diffusion import SpacedDiffusionBeatGans
from teramind_amd.train_model import UNetTrain, training_loss_and_grads
from teramind_amd.trainer import Trainer
from teramind_amd.training import AttnBlockTrain
from teramind_amd.weights import hashed_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(ATTN_SHORT_CASES))
def test_attn_block_short_window_vs_reference(name):
    gold = np.load(os.path.join(GOLD, "train_attn_short_ref.npz"))
    x, cond, dout, params = make_attn_short_inputs(name)
    blk = AttnBlockTrain(params, DEV)
    out = blk.forward(x, cond)
    dx, dcond, grads = blk.backward(dout)
    rel = lambda a, r: float((a.double().cpu() - r.double()).norm() / r.double().norm())
    errs = {"out": rel(out, torch.from_numpy(gold[f"{name}/out"])), "dx": rel(dx, torch.from_numpy(gold[f"{name}/dx"])),
            "dcond": rel(dcond, torch.from_numpy(gold[f"{name}/dcond"]))}
    assert sorted(grads) == sorted(params)
    for k in params:
        errs[k] = rel(grads[k].reshape(params[k].shape), torch.from_numpy(gold[f"{name}/grad/{k}"]))
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("name", sorted(GRAD_SHORT_CASES))
def test_whole_model_gradients_vs_reference_backward(name, resident):
    gold = np.load(os.path.join(GOLD, "train_grad_short_ref.npz"))
    over, loss_type, crop, (x_pad, rna, imgs, t, pos, mask, idx, noise) = make_short_inputs(name)
    cfg = PathConfig(**over)
    sd = hashed_state_dict(cfg, 0)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    step = lambda: training_loss_and_grads(UNetTrain(cfg, sd, DEV, resident=resident), sampler, x_pad, rna, t, mask, noise, crop,
                                           cfg.patch_size, loss_type)
    loss, grads = step()
    ref_loss = float(gold[f"{name}/loss"])
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    keys = [str(k) for k in gold[f"{name}/keys"]]
    assert sorted(keys) == sorted(sd) and sorted(grads) == sorted(keys), (set(keys) ^ set(grads))
    bad = []
    for i, k in enumerate(keys):
        g = grads[k].double().cpu().reshape(-1).numpy()
        nref = float(gold[f"{name}/norm"][i])
        e_norm = abs(np.linalg.norm(g) - nref) / nref
        pr = np.array([float(g @ grad_probe(k, g.size, j)) for j in range(GRAD_PROBES)])
        e_proj = float(np.abs(pr - gold[f"{name}/proj"][i]).max()) / nref
        e_full = 0.0
        if g.size <= GRAD_FULL_MAX:
            rf = gold[f"{name}/full/{k}"].astype(np.float64).reshape(-1)
            e_full = float(np.linalg.norm(g - rf) / np.linalg.norm(rf))
        if not (e_norm < 2e-3 and e_proj < 3e-3 and e_full < 2e-3):
            bad.append((k, nref, e_norm, e_proj, e_full))
    assert not bad, f"{len(bad)} of {len(keys)} gradients off: " + "; ".join(f"{k} |g|={n:.3g} norm {a:.2e} proj {b:.2e} full {c:.2e}"
                                                                              for k, n, a, b, c in bad[:12])
    loss2, grads2 = step()
    assert loss2 == loss and all(torch.equal(grads2[k], grads[k]) for k in keys)


@pytest.mark.parametrize("resident", [False, True])
def test_trainer_resumes_bit_for_bit(tmp_path, resident):
    cfg = PathConfig(net_ch=16, rna_num=37, rna_slc=4, patch_size=32)
    synth.write_train_tile_dir(tmp_path, n_tiles=2, H=192, W=192, zt=6, nnz=100000, seed=1)
    tiles = TrainTileSet(os.path.join(str(tmp_path), "gene"), cfg, DEV, seed=7, repeat=4)
    new = lambda: Trainer(cfg, hashed_state_dict(cfg, 0), tiles, 2, accum_batches=1, seed=7, dropout_p=0.1, resident=resident)
    straight = new()
    losses = [straight.step()["loss"] for _ in range(2)]
    assert all(np.isfinite(v) for v in losses)
    first = new()
    l0 = first.step()["loss"]
    path = os.path.join(tmp_path, "last.ckpt")
    first.save(path)
    del first
    resumed = Trainer.resume(path, tiles)
    assert resumed.global_step == 1 and resumed.cfg.patch_size == 32 and resumed.cfg.rna_slc == 4
    assert [l0, resumed.step()["loss"]] == losses
    assert torch.equal(resumed.opt.p, straight.opt.p) and torch.equal(resumed.opt.m, straight.opt.m) and torch.equal(resumed.opt.v, straight.opt.v)


def test_rna_slc_1_at_patch_32_is_refused_in_the_constructor():
    cfg = PathConfig(rna_slc=1, patch_size=32)
    with pytest.raises(NotImplementedError, match="32 voxels"):
        UNetTrain(cfg, {"out.0.weight": torch.zeros(1)}, DEV)
