"""-m gpu: the device-resident conv engine of the training tape (UNetTrain / Trainer with resident=True): conv weights packed on
the GPU once per role per optimizer step, conv gradients written by the MFMA weight-gradient kernel into device tensors.  The
forward equals the host-weight engine bit for bit (same packs, same kernels); the gradients are held to the reference's own
autograd through the goldens of test_gpu_train_model.py / test_gpu_train_dropout.py with the same checks and bounds."""
import os

import numpy as np
import pytest
import torch

from teramind_amd import synth
from teramind_amd.config import PathConfig
from teramind_amd.dataset import TrainTileSet
from teramind_amd.diffusion import SpacedDiffusionBeatGans
from teramind_amd.train_model import AdamTrainer, UNetTrain, training_loss_and_grads
from teramind_amd.trainer import Trainer, load_checkpoint
from teramind_amd.weights import hashed_state_dict, strip_lightning_state_dict
from train_cases import GRAD_CASES, GRAD_CFG, GRAD_FULL_MAX, GRAD_PROBES, grad_probe, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, BATCH = 7, 2
NAME = "mse_seed3"


@pytest.fixture(scope="module")
def cfg():
    return PathConfig(**GRAD_CFG)


@pytest.fixture(scope="module")
def tiles(cfg, tmp_path_factory):
    root = tmp_path_factory.mktemp("tiles")
    synth.write_train_tile_dir(root, n_tiles=2, H=320, W=320, zt=6, nnz=300000, seed=1)
    return TrainTileSet(os.path.join(str(root), "gene"), cfg, DEV, seed=SEED, repeat=4)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_resident_forward_equals_host_weight_forward(cfg):
    sd = hashed_state_dict(cfg, 0)
    b, ps = 2, cfg.patch_size
    g = torch.Generator().manual_seed(4)
    x = torch.randn((b * 4, cfg.in_channels, ps, ps), generator=g)
    rna = (torch.rand((b * 4, cfg.gn_sz, cfg.gn_sz, cfg.rna_slc * 500), generator=g) < 0.02).float() * 3.0
    t = torch.tensor([17, 803])
    ref, ref2 = UNetTrain(cfg, sd, DEV).forward(x, t, rna, b)
    got, got2 = UNetTrain(cfg, sd, DEV, resident=True).forward(x, t, rna, b)
    assert float(ref.abs().max()) > 0 and _same_bits(got, ref) and _same_bits(got2, ref2)


def _step(cfg, p=None, key=0, resident=True):
    seed, loss_type, crop = GRAD_CASES[NAME]
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed)
    net = UNetTrain(cfg, hashed_state_dict(cfg, 0), DEV, resident=resident)
    return training_loss_and_grads(net, SpacedDiffusionBeatGans(1000, "ddpm"), x_pad, rna, t, mask, noise, crop, cfg.patch_size, loss_type,
                                   dropout_p=p, dropout_key=key)


def _check_against_golden(gold, sd, loss, grads):
    """The checks of test_whole_model_gradients_vs_reference_backward, with its bounds."""
    ref_loss = float(gold[f"{NAME}/loss"])
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    keys = sorted(k[len(NAME) + 6:] for k in gold.files if k.startswith(f"{NAME}/norm/"))
    assert keys == sorted(sd) and sorted(grads) == keys, (set(keys) ^ set(grads))
    assert len(keys) == 403
    bad = []
    for k in keys:
        assert grads[k].is_cuda and tuple(grads[k].shape) == tuple(sd[k].shape), k
        g = grads[k].double().reshape(-1).cpu().numpy()
        nref = float(gold[f"{NAME}/norm/{k}"])
        e_norm = abs(np.linalg.norm(g) - nref) / nref
        pr = np.array([float(g @ grad_probe(k, g.size, j)) for j in range(GRAD_PROBES)])
        e_proj = float(np.abs(pr - gold[f"{NAME}/proj/{k}"]).max()) / nref
        e_full = 0.0
        if g.size <= GRAD_FULL_MAX:
            rf = gold[f"{NAME}/full/{k}"].astype(np.float64).reshape(-1)
            e_full = float(np.linalg.norm(g - rf) / np.linalg.norm(rf))
        if not (e_norm < 2e-3 and e_proj < 3e-3 and e_full < 2e-3):
            bad.append((k, nref, e_norm, e_proj, e_full))
    assert not bad, f"{len(bad)} of {len(keys)} gradients off: " + "; ".join(f"{k} |g|={n:.3g} norm {a:.2e} proj {b:.2e} full {c:.2e}"
                                                                              for k, n, a, b, c in bad[:12])
    return keys


def test_resident_whole_model_gradients_vs_reference_backward(cfg):
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_grad_ref.npz"))
    loss, grads = _step(cfg)
    keys = _check_against_golden(gold, hashed_state_dict(cfg, 0), loss, grads)
    loss2, grads2 = _step(cfg)
    assert loss2 == loss and all(_same_bits(grads2[k], grads[k]) for k in keys)


def test_resident_whole_model_dropout_gradients_vs_reference(cfg):
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_grad_dropout_ref.npz"))
    p, key = float(gold["p"]), int(gold["key"])
    loss, grads = _step(cfg, p, key)
    keys = _check_against_golden(gold, hashed_state_dict(cfg, 0), loss, grads)
    loss2, grads2 = _step(cfg, p, key)
    assert loss2 == loss and all(_same_bits(grads2[k], grads[k]) for k in keys)


def _trainer(cfg, tiles, accum=1):
    return Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=accum, seed=SEED, dropout_p=0.1, resident=True)


def test_resident_resume_continues_bit_for_bit_and_checkpoint_loads(cfg, tiles, tmp_path):
    straight = _trainer(cfg, tiles)
    losses = [straight.step()["loss"] for _ in range(3)]
    assert all(np.isfinite(v) for v in losses)
    first = _trainer(cfg, tiles)
    l0 = first.step()["loss"]
    path = os.path.join(tmp_path, "last.ckpt")
    first.save(path)
    del first
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd0 = hashed_state_dict(cfg, 0)
    assert sorted(ck["state_dict"]) == sorted("model." + k for k in sd0)
    assert any(not torch.equal(ck["state_dict"]["model." + k], torch.as_tensor(sd0[k]).float()) for k in sd0)     # the stepped weights
    assert load_checkpoint(path)["hparams"]["resident"] is True
    resumed = Trainer.resume(path, tiles)
    assert resumed.net.resident and resumed.global_step == 1 and resumed.opt.t == 1 and resumed.seed == SEED
    assert resumed.opt.p is resumed.net.P                                                  # one master copy
    l12 = [resumed.step()["loss"] for _ in range(2)]
    assert [l0] + l12 == losses
    assert torch.equal(resumed.opt.p, straight.opt.p) and torch.equal(resumed.opt.m, straight.opt.m) and torch.equal(resumed.opt.v, straight.opt.v)
    assert all(torch.equal(resumed.net.W[k], straight.net.W[k]) for k in straight.net.W)


def test_each_conv_weight_packed_once_per_role_per_optimizer_step(cfg, tiles):
    tr = _trainer(cfg, tiles, accum=2)
    sd = hashed_state_dict(cfg, 0)
    convs = [k[:-len(".weight")] for k, v in sd.items()                     # Conv3d parameters: 5-d weight with a bias (norms have none)
             if k.endswith(".weight") and torch.as_tensor(v).dim() == 5 and k[:-len("weight")] + "bias" in sd]
    assert len(convs) > 50
    seen = {}
    for step in range(2):
        tr.step()                                            # two micro-batches, decoder blocks run twice in each
        now = dict(tr.net.pack_count)
        assert sorted(now) == sorted((c, r) for c in convs for r in (0, 1)), set(now) ^ {(c, r) for c in convs for r in (0, 1)}
        assert all(now[k] - seen.get(k, 0) == 1 for k in now), {k: now[k] - seen.get(k, 0) for k in now if now[k] - seen.get(k, 0) != 1}
        seen = now
        assert not tr.net.convs._packs                           # stale after AdamTrainer.step()


def test_next_forward_uses_the_updated_weights(cfg):
    sd = hashed_state_dict(cfg, 0)
    seed, loss_type, crop = GRAD_CASES[NAME]
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    net = UNetTrain(cfg, sd, DEV, resident=True)
    opt = AdamTrainer(net)
    assert opt.p is net.P
    run = lambda n: training_loss_and_grads(n, sampler, x_pad, rna, t, mask, noise, crop, cfg.patch_size, loss_type)     # noqa: E731
    loss0, grads = run(net)
    opt.accumulate(grads)
    opt.step()
    loss1, grads1 = run(net)
    assert loss1 != loss0 and loss1 < loss0
    new_sd = {k: v.clone() for k, v in net.W.items()}                     # what checkpoint() saves
    assert any(not torch.equal(new_sd[k], torch.as_tensor(sd[k]).float()) for k in sd)
    fresh_loss, fresh = run(UNetTrain(cfg, new_sd, DEV, resident=True))
    assert fresh_loss == loss1 and all(_same_bits(fresh[k], grads1[k]) for k in grads1)
