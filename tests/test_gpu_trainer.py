"""GPU: the training loop of teramind_amd.trainer over a synthetic two-tile set (tools/make_train_tiles.py's writer), on the
tiny model of tests/train_cases.py (GRAD_CFG), batch 2.  About ten training steps in all (~4 s each)."""
import os

import numpy as np
import pytest
import torch

from train_cases import GRAD_CFG
from teramind_amd import synth
from teramind_amd.config import PathConfig
from teramind_amd.dataset import TrainTileSet
from teramind_amd.diffusion import SpacedDiffusionBeatGans
from teramind_amd.train_model import AdamTrainer, UNetTrain, derive_dropout_key, training_loss_and_grads
from teramind_amd.trainer import Trainer, load_checkpoint, pad_and_mask, step_noise, step_randoms
from teramind_amd.unet import BeatGANsUNetModel
from teramind_amd.weights import hashed_state_dict, strip_lightning_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, BATCH = 7, 2


@pytest.fixture(scope="module")
def cfg():
    return PathConfig(**GRAD_CFG)


@pytest.fixture(scope="module")
def tiles(cfg, tmp_path_factory):
    root = tmp_path_factory.mktemp("tiles")
    paths = synth.write_train_tile_dir(root, n_tiles=2, H=320, W=320, zt=6, nnz=300000, seed=1)
    assert os.path.isfile(paths[0].replace("gene", "img").replace(".npz", ".zip"))
    return TrainTileSet(os.path.join(str(root), "gene"), cfg, DEV, seed=SEED, repeat=4)


def new_trainer(cfg, tiles, seed=SEED):
    return Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=1, seed=seed, dropout_p=0.1)


def test_dense_route_equals_tuple_route(cfg, tiles):
    bt = tiles.draw(BATCH, 0)
    x_pad, mask = pad_and_mask(bt.img, cfg.patch_size)
    assert x_pad.shape == (BATCH, 4, 320, 320) and bt.rna.shape == (BATCH, 20, 20, 2000) and float(bt.rna.sum()) > 0
    t = torch.tensor([17, 803])
    noise = step_noise(SEED, 0, 0, 0, x_pad.shape, DEV)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    sd = hashed_state_dict(cfg, 0)
    key = derive_dropout_key(SEED, 0, 0)
    _, dat, crd, ssz, _ = bt.as_coo()
    for crop in ((3, 0),):                                         # the window at the far edge of the padded image
        l_d, g_d = training_loss_and_grads(UNetTrain(cfg, sd, DEV, dropout_p=0.1), sampler, x_pad, bt.rna, t, mask, noise, crop, cfg.patch_size,
                                           "mse", dropout_key=key)
        l_t, g_t = training_loss_and_grads(UNetTrain(cfg, sd, DEV, dropout_p=0.1), sampler, x_pad, (dat, crd, ssz), t, mask, noise, crop,
                                           cfg.patch_size, "mse", dropout_key=key)
        assert np.isfinite(l_d) and l_d == l_t
        assert len(g_d) == 403 and sorted(g_d) == sorted(g_t)
        assert all(torch.equal(g_d[k], g_t[k]) for k in g_d)


def test_trainer_step_equals_hand_assembly(cfg, tiles):
    tr = new_trainer(cfg, tiles)
    info = tr.step()
    assert np.isfinite(info["loss"]) and info["step"] == 1 and info["grad_norm"] > 0 and 0 < info["clip_coef"] <= 1
    # the same step by hand
    net = UNetTrain(cfg, hashed_state_dict(cfg, 0), DEV, dropout_p=0.1)
    opt = AdamTrainer(net, lr=2e-5, grad_clip=1.0)
    bt = tiles.gather(tr.sampler.params(BATCH, 0, 0))
    x_pad, mask = pad_and_mask(bt.img, cfg.patch_size)
    t, ix, iy = step_randoms(SEED, 0, 0, 0, BATCH, tiles.geo.sdim // cfg.patch_size)
    assert t.min() >= 0 and t.max() < 1000 and 0 <= ix < 4 and 0 <= iy < 4
    noise = step_noise(SEED, 0, 0, 0, x_pad.shape, DEV)
    loss, grads = training_loss_and_grads(net, SpacedDiffusionBeatGans(1000, "ddpm"), x_pad, bt.rna, torch.from_numpy(t), mask, noise,
                                          (ix, iy), cfg.patch_size, "mse", dropout_key=derive_dropout_key(SEED, 0, 0))
    opt.accumulate(grads)
    info2 = opt.step()
    assert loss == info["loss"] and info2["grad_norm"] == info["grad_norm"]
    assert torch.equal(opt.p, tr.opt.p) and torch.equal(opt.m, tr.opt.m) and torch.equal(opt.v, tr.opt.v)
    assert all(torch.equal(net.W[k], tr.net.W[k]) for k in net.W)
    # a different seed gives a different first batch
    other = new_trainer(cfg, tiles, seed=SEED + 1)
    assert not np.array_equal(other.sampler.params(BATCH, 0), tr.sampler.params(BATCH, 0))
    a, b = other.micro_batch(0, 0), tr.micro_batch(0, 0)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[4], b[4])


def test_resume_continues_bit_for_bit_and_checkpoint_loads(cfg, tiles, tmp_path):
    straight = new_trainer(cfg, tiles)
    losses = [straight.step()["loss"] for _ in range(3)]
    assert all(np.isfinite(v) for v in losses)
    first = new_trainer(cfg, tiles)
    l0 = first.step()["loss"]
    path = os.path.join(tmp_path, "last.ckpt")
    first.save(path)
    del first
    resumed = Trainer.resume(path, tiles)
    assert resumed.global_step == 1 and resumed.opt.t == 1 and resumed.seed == SEED
    l12 = [resumed.step()["loss"] for _ in range(2)]
    assert [l0] + l12 == losses
    assert torch.equal(resumed.opt.p, straight.opt.p) and torch.equal(resumed.opt.m, straight.opt.m) and torch.equal(resumed.opt.v, straight.opt.v)
    assert all(torch.equal(resumed.net.W[k], straight.net.W[k]) for k in straight.net.W)


def test_checkpoint_loads_into_the_inference_model(tiles, tmp_path):
    """experiment.py:50-58 / test_brn.py:140-147: the saved state_dict, stripped of its 'model.' prefix, feeds
    BeatGANsUNetModel.load_state_dict(strict=True) unchanged, and a forward runs.  On the default config: the inference
    model needs net_ch to be a multiple of 64, which GRAD_CFG (net_ch = 16) is not."""
    cfg = PathConfig()
    tr = Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=1, seed=SEED, dropout_p=0.1)
    assert np.isfinite(tr.step()["loss"])
    path = os.path.join(tmp_path, "last.ckpt")
    tr.save(path)
    ck = load_checkpoint(path)
    assert ck["global_step"] == 1 and ck["config_name"] == cfg.name
    sd = strip_lightning_state_dict(ck)
    model = BeatGANsUNetModel(cfg, DEV)
    model.load_state_dict(sd, strict=True)
    assert all(torch.equal(sd[k], tr.net.W[k]) for k in sd)
    ps = cfg.patch_size
    x = synth.normal("trainer/x", (4, cfg.in_channels, ps, ps), 0).to(DEV)
    rna = synth.gene_counts("trainer/rna", (4, cfg.gn_sz, cfg.gn_sz, cfg.rna_slc * 500), 0).to(DEV)
    out = model(x=x, t=torch.tensor([500], device=DEV), rna=rna, imgs=torch.zeros(1, cfg.in_channels, ps, ps), patch_size=ps)
    assert torch.isfinite(out.pred).all()
