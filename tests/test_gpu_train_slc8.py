"""-m gpu: training the rna_slc 8 model (windows of 256 tokens in the resolution-16 AttnBlocks, down_z at kz = 5).

  * training.DownZTrain on small integers: forward, dx, dw, db equal F.conv3d and its autograd bit for bit, on both engines;
  * training.AttnBlockTrain at 512-token windows against the reference module in float64
    (tests/golden/train_attn_long_ref.npz), relative L2 < 1e-4 per tensor as tests/test_gpu_train.py asks of the short windows;
  * the whole step against the reference's own training_losses(...).backward() (tests/golden/train_grad_slc8_ref.npz) with
    the bounds of tests/test_gpu_train_model.py, host and resident engine, every bit reproduced by a second run;
  * the Trainer on a synthetic rna_slc 8 tile directory, with dropout, on both engines: 2 steps equal 1 + save + resume + 1;
  * rna_slc 16 is still refused, and the message says what is missing.
Both fixtures are minted by tools/make_train_slc8_golden.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
from train_cases import GRAD_FULL_MAX, GRAD_PROBES, grad_probe, make_inputs
from train_long_cases import ATTN_LONG_CASES, SLC8_CASES, SLC8_CFG, make_attn_long_inputs
from teramind_amd import synth
from teramind_amd.config import PathConfig
from teramind_amd.dataset import TrainTileSet
from teramind_amd.diffusion import SpacedDiffusionBeatGans
from teramind_amd.train_model import UNetTrain, training_loss_and_grads
from teramind_amd.trainer import Trainer
from teramind_amd.training import AttnBlockTrain, DownZTrain
from teramind_amd.weights import hashed_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")


# (kz, planes in): rna_slc 8 (8 in, 4 out) and the depth rna_slc 16 will need (16 in, 8 out is beyond the four staged planes of
# the weight-gradient kernels, so kz = 9 runs here at 12 in, 4 out)
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("kz,Zi", [(5, 8), (9, 12)])
def test_down_z_exact_on_integers(kz, Zi, resident):
    N, Ci, Co, S = 2, 13, 40, 4
    x = util.rand_int((N, Ci, Zi, S, S), -3, 3, 61)
    w = util.rand_int((Co, Ci, kz, 3, 3), -3, 3, 62)
    b = util.rand_int((Co,), -3, 3, 63)
    dy = util.rand_int((N, Co, Zi - kz + 1, S, S), -3, 3, 64)
    leaves = [t.double().clone().requires_grad_(True) for t in (x, w, b)]
    ref = F.conv3d(leaves[0], leaves[1], leaves[2], padding=(0, 1, 1))
    ref.backward(dy.double())
    runs = []
    for _ in range(2):
        blk = DownZTrain(w.float(), b.float(), DEV, resident=resident)
        y = blk.forward(x.float())
        dx, dw, db = blk.backward(dy.float())
        runs.append([t.cpu() for t in (y, dx, dw, db)])
    for name, got, want in zip(("y", "dx", "dw", "db"), runs[0], (ref.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad)):
        assert torch.equal(got.double(), want), util.report(name, got.double(), want)
    assert all(torch.equal(a, c) for a, c in zip(*runs))


@pytest.mark.parametrize("name", sorted(ATTN_LONG_CASES))
def test_attn_block_long_window_vs_reference(name):
    gold = np.load(os.path.join(GOLD, "train_attn_long_ref.npz"))
    x, cond, dout, params = make_attn_long_inputs(name)
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
@pytest.mark.parametrize("name", sorted(SLC8_CASES))
def test_whole_model_gradients_vs_reference_backward(name, resident):
    gold = np.load(os.path.join(GOLD, "train_grad_slc8_ref.npz"))
    seed, loss_type, crop = SLC8_CASES[name]
    cfg = PathConfig(**SLC8_CFG)
    sd = hashed_state_dict(cfg, 0)
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed, C=cfg.n_stain * cfg.z_size, srna=cfg.rna_slc)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    step = lambda: training_loss_and_grads(UNetTrain(cfg, sd, DEV, resident=resident), sampler, x_pad, rna, t, mask, noise, crop,
                                           cfg.patch_size, loss_type)
    loss, grads = step()
    ref_loss = float(gold[f"{name}/loss"])
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    keys = sorted(k[len(name) + 6:] for k in gold.files if k.startswith(f"{name}/norm/"))
    assert keys == sorted(sd) and sorted(grads) == keys, (set(keys) ^ set(grads))
    bad = []
    for k in keys:
        g = grads[k].double().cpu().reshape(-1).numpy()
        nref = float(gold[f"{name}/norm/{k}"])
        e_norm = abs(np.linalg.norm(g) - nref) / nref
        pr = np.array([float(g @ grad_probe(k, g.size, j)) for j in range(GRAD_PROBES)])
        e_proj = float(np.abs(pr - gold[f"{name}/proj/{k}"]).max()) / nref
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


# dropout on both engines: the host-weight one rebuilds its down_z block after every optimizer step, the resident one repacks
@pytest.mark.parametrize("resident", [False, True])
def test_trainer_resumes_bit_for_bit(tmp_path, resident):
    cfg = PathConfig(**SLC8_CFG)
    synth.write_train_tile_dir(tmp_path, n_tiles=2, H=320, W=320, zt=12, nnz=300000, seed=1)
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
    assert resumed.global_step == 1 and resumed.cfg.rna_slc == 8
    assert [l0, resumed.step()["loss"]] == losses
    assert torch.equal(resumed.opt.p, straight.opt.p) and torch.equal(resumed.opt.m, straight.opt.m) and torch.equal(resumed.opt.v, straight.opt.v)


def test_rna_slc_16_is_still_refused():
    cfg = PathConfig(rna_slc=16)
    with pytest.raises(NotImplementedError, match="Z <= 4"):
        UNetTrain(cfg, {"out.0.weight": torch.zeros(1)}, DEV)
