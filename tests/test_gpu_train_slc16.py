"""-m gpu: training the rna_slc 16 model on the resident engine (every conv at Z = 8, windows of 512 tokens in the resolution-16
AttnBlocks and of 128 in the middle block, down_z at kz = 9: 16 gene planes in, 8 out).

  * training.DownZTrain at (kz 9, 16 planes) on small integers: forward, dx, dw, db equal F.conv3d and its autograd bit for bit on the
    resident engine; the host-weight engine refuses the call;
  * the whole step against the reference's own training_losses(...).backward() (tests/golden/train_grad_slc16_ref.npz, minted by
    tools/make_train_slc16_golden.py) with the bounds of tests/test_gpu_train_model.py, every bit reproduced by a second run;
  * the Trainer on a synthetic rna_slc 16 tile directory, with dropout: 2 steps equal 1 + save + resume + 1;
  * the host-weight engine refuses rna_slc 16 and says where it trains; patch sizes other than 64 are refused."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
from train_cases import GRAD_FULL_MAX, GRAD_PROBES, grad_probe, make_inputs
from train_slc16_cases import SLC16_CASES, SLC16_CFG
from teramind_amd import synth
from teramind_amd.config import PathConfig
from teramind_amd.dataset import TrainTileSet
from teramind_amd.diffusion import SpacedDiffusionBeatGans
from teramind_amd.train_model import UNetTrain, training_loss_and_grads
from teramind_amd.trainer import Trainer
from teramind_amd.training import DownZTrain
from teramind_amd.weights import hashed_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _down_z_case():
    N, Ci, Co, S, kz, Zi = 2, 13, 40, 4, 9, 16
    x = util.rand_int((N, Ci, Zi, S, S), -3, 3, 61)
    w = util.rand_int((Co, Ci, kz, 3, 3), -3, 3, 62)
    b = util.rand_int((Co,), -3, 3, 63)
    dy = util.rand_int((N, Co, Zi - kz + 1, S, S), -3, 3, 64)
    return x, w, b, dy


def test_down_z_16_planes_exact_on_integers():
    """Sums of at most 13 * 81 products of integers in [-3, 3] (y, dw: 2 * 8 * 16 * 9 per tap plane), far below 2^24: exact."""
    x, w, b, dy = _down_z_case()
    leaves = [t.double().clone().requires_grad_(True) for t in (x, w, b)]
    ref = F.conv3d(leaves[0], leaves[1], leaves[2], padding=(0, 1, 1))
    ref.backward(dy.double())
    runs = []
    for _ in range(2):
        blk = DownZTrain(w.float(), b.float(), DEV, resident=True)
        y = blk.forward(x.float())
        dx, dw, db = blk.backward(dy.float())
        runs.append([t.cpu() for t in (y, dx, dw, db)])
    assert tuple(runs[0][0].shape) == (2, 40, 8, 4, 4)
    for name, got, want in zip(("y", "dx", "dw", "db"), runs[0], (ref.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad)):
        assert torch.equal(got.double(), want), util.report(name, got.double(), want)
    assert all(torch.equal(a, c) for a, c in zip(*runs))


def test_down_z_16_planes_refused_on_host_engine():
    x, w, b, _ = _down_z_case()
    blk = DownZTrain(w.float(), b.float(), DEV, resident=False)
    with pytest.raises(ValueError, match="resident"):
        blk.forward(x.float())


@pytest.mark.parametrize("name", sorted(SLC16_CASES))
def test_whole_model_gradients_vs_reference_backward(name, capsys):
    """Bounds of test_gpu_train_model.py: loss 2e-5 relative; per tensor norm 2e-3, projections 3e-3 (of the norm), whole gradient
    2e-3.  The worst of each is printed before the assertion (pytest -s); measured: profiles/train_slc16.txt."""
    gold = np.load(os.path.join(GOLD, "train_grad_slc16_ref.npz"))
    seed, loss_type, crop = SLC16_CASES[name]
    cfg = PathConfig(**SLC16_CFG)
    sd = hashed_state_dict(cfg, 0)
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed, C=cfg.n_stain * cfg.z_size, srna=cfg.rna_slc)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    step = lambda: training_loss_and_grads(UNetTrain(cfg, sd, DEV, resident=True), sampler, x_pad, rna, t, mask, noise, crop,
                                           cfg.patch_size, loss_type)
    loss, grads = step()
    ref_loss = float(gold[f"{name}/loss"])
    keys = sorted(k[len(name) + 6:] for k in gold.files if k.startswith(f"{name}/norm/"))
    assert keys == sorted(sd) and sorted(grads) == keys, (set(keys) ^ set(grads))
    bad, worst = [], [0.0, 0.0, 0.0]
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
        worst = [max(a, c) for a, c in zip(worst, (e_norm, e_proj, e_full))]
        if not (e_norm < 2e-3 and e_proj < 3e-3 and e_full < 2e-3):
            bad.append((k, nref, e_norm, e_proj, e_full))
    with capsys.disabled():
        print(f"\nslc16 step {name}: loss {loss:.7f} (ref {ref_loss:.7f}, rel {abs(loss - ref_loss) / abs(ref_loss):.2e} of 2e-5)  worst/bound: "
              f"norm {worst[0] / 2e-3:.3f}  proj {worst[1] / 3e-3:.3f}  full {worst[2] / 2e-3:.3f}")
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    assert not bad, f"{len(bad)} of {len(keys)} gradients off: " + "; ".join(f"{k} |g|={n:.3g} norm {a:.2e} proj {b:.2e} full {c:.2e}"
                                                                              for k, n, a, b, c in bad[:12])
    loss2, grads2 = step()
    assert loss2 == loss and all(torch.equal(grads2[k], grads[k]) for k in keys)


def test_trainer_resumes_bit_for_bit(tmp_path):
    cfg = PathConfig(**SLC16_CFG)
    synth.write_train_tile_dir(tmp_path, n_tiles=2, H=320, W=320, zt=16, nnz=300000, seed=1)
    tiles = TrainTileSet(os.path.join(str(tmp_path), "gene"), cfg, DEV, seed=7, repeat=4)
    new = lambda: Trainer(cfg, hashed_state_dict(cfg, 0), tiles, 2, accum_batches=1, seed=7, dropout_p=0.1, resident=True)
    straight = new()
    losses = [straight.step()["loss"] for _ in range(2)]
    assert all(np.isfinite(v) for v in losses)
    first = new()
    l0 = first.step()["loss"]
    path = os.path.join(tmp_path, "last.ckpt")
    first.save(path)
    del first
    resumed = Trainer.resume(path, tiles)
    assert resumed.global_step == 1 and resumed.cfg.rna_slc == 16 and resumed.net.resident
    assert [l0, resumed.step()["loss"]] == losses
    assert torch.equal(resumed.opt.p, straight.opt.p) and torch.equal(resumed.opt.m, straight.opt.m) and torch.equal(resumed.opt.v, straight.opt.v)


def test_host_engine_refuses_rna_slc_16():
    cfg = PathConfig(rna_slc=16)
    with pytest.raises(NotImplementedError) as e:
        UNetTrain(cfg, {"out.0.weight": torch.zeros(1)}, DEV, resident=False)
    assert "Z <= 4" in str(e.value) and "resident=True" in str(e.value)


@pytest.mark.parametrize("ps", [32, 128])
def test_other_patch_sizes_refused_at_rna_slc_16(ps):
    with pytest.raises(NotImplementedError, match="patch size 64 only"):
        UNetTrain(PathConfig(rna_slc=16, patch_size=ps), {"out.0.weight": torch.zeros(1)}, DEV, resident=True)
