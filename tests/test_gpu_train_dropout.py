"""-m gpu: ResBlock dropout with the keep mask drawn on the GPU.  tm_op_dropout_mask equals the numpy statement of
the rule (tests/dropout_rng.py); the drawing prep forward / backward equal the supplied-mask ops given that mask, bit for bit;
the whole-model training step with dropout_p = 0.1 equals the reference's own train-mode `training_losses(...).backward()`
with the same masks (tests/golden/train_grad_dropout_ref.npz, minted by tools/make_train_dropout_golden.py)."""
import os

import numpy as np
import pytest
import torch

from dropout_rng import drop_scale, keep_mask
from teramind_amd import _lib
from teramind_amd.config import PathConfig
from teramind_amd.diffusion import SpacedDiffusionBeatGans
from teramind_amd.train_model import UNetTrain, derive_dropout_key, dropout_sites, training_loss_and_grads
from teramind_amd.training import _cb8, _hp
from teramind_amd.weights import hashed_state_dict
from train_cases import GRAD_CASES, GRAD_CFG, GRAD_FULL_MAX, GRAD_PROBES, grad_probe, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mask_cb8(key, site, p, N, Cc, Z, S):
    m = torch.full((N, (Cc + 7) // 8, Z, S, S, 8), -1.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().tm_op_dropout_mask(key, site, p, _lib.ptr(m), N, Cc, Z, S, _lib.current_stream_ptr()), "tm_op_dropout_mask")
    return m


@pytest.mark.parametrize("N,Cc,Z,S", [(1, 8, 1, 8), (25, 20, 2, 8), (3, 37, 2, 64), (2, 64, 1, 64), (4, 13, 1, 8)])
def test_dropout_mask_kernel_equals_rule(N, Cc, Z, S):
    for key, site, p in ((0, 0, 0.1), (0xFEDC_BA98_7654_3210, 41, 0.5), (12345, 7, 0.1), ((1 << 64) - 1, 0xFFFFFFFF, 0.5)):
        m = _mask_cb8(key, site, p, N, Cc, Z, S)
        got = m.permute(0, 1, 5, 2, 3, 4).reshape(N, -1, Z, S, S).cpu()
        want = torch.from_numpy(keep_mask(key, site, p, (N, Cc, Z, S, S)).astype(np.float32))
        assert torch.equal(got[:, :Cc], want), (N, Cc, Z, S, key, site, p)
        assert torch.equal(got[:, Cc:], torch.zeros_like(got[:, Cc:]))           # pad channels
    with pytest.raises(RuntimeError):
        _mask_cb8(1, 0, 1.0, 1, 8, 1, 8)


def _prep_case(Cc, N, Z, S, per_image, mod, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, Cc, Z, S, S), generator=g)
    dy = torch.randn((N, Cc, Z, S, S), generator=g)
    w = 1.0 + 0.2 * torch.randn((Cc,), generator=g)
    nimg = (N + per_image - 1) // per_image
    sc = 0.3 * torch.randn((nimg, Cc), generator=g) if mod else None
    sh = 0.3 * torch.randn((nimg, Cc), generator=g) if mod else None
    return _cb8(x.to(DEV)), _cb8(dy.to(DEV)), w, sc, sh


@pytest.mark.parametrize("Cc", [20, 300, 600])            # Cb = 3 (cached forward), 38 (uncached), 75 (> 16 blocks per wave: redraw)
@pytest.mark.parametrize("mod", [False, True])
def test_drawn_prep_equals_supplied_mask(Cc, mod):
    N, Z, S, per_image = 4, 2, 8, 2
    xc, gc, w, sc, sh = _prep_case(Cc, N, Z, S, per_image, mod, Cc + mod)
    L, st = _lib.lib(), _lib.current_stream_ptr()
    nimg = N // per_image
    for key, site, p in ((0xA5A5_0000_1234_5678, 9, 0.1), (3, 0, 0.5)):
        mask = _mask_cb8(key, site, p, N, Cc, Z, S)
        s = float(drop_scale(p))
        y_ref, y = torch.empty_like(xc), torch.empty_like(xc)
        _lib.check(L.tm_op_prep_train(_lib.ptr(xc), _hp(w), _hp(sc), _hp(sh), _lib.ptr(mask), s, per_image, _lib.ptr(y_ref), N, Cc, Z, S, st))
        _lib.check(L.tm_op_prep_train_rng(_lib.ptr(xc), _hp(w), _hp(sc), _hp(sh), key, site, p, per_image, _lib.ptr(y), N, Cc, Z, S, st))
        assert torch.equal(y, y_ref), (Cc, mod, key, site, p)
        assert float((y == 0).float().mean()) > p / 2                                # something is dropped
        outs = []
        for rng in (False, True):
            dx = torch.empty_like(xc)
            dw = torch.empty((Cc,), dtype=torch.float32)
            dsc = torch.empty((nimg, Cc), dtype=torch.float32) if mod else None
            dsh = torch.empty((nimg, Cc), dtype=torch.float32) if mod else None
            if rng:
                _lib.check(L.tm_op_prep_bwd_rng(_lib.ptr(xc), _lib.ptr(gc), _hp(w), _hp(sc), _hp(sh), key, site, p, per_image, _lib.ptr(dx),
                                                _hp(dw), _hp(dsc), _hp(dsh), N, Cc, Z, S, st))
            else:
                _lib.check(L.tm_op_prep_bwd(_lib.ptr(xc), _lib.ptr(gc), _hp(w), _hp(sc), _hp(sh), _lib.ptr(mask), s, per_image, _lib.ptr(dx),
                                            _hp(dw), _hp(dsc), _hp(dsh), N, Cc, Z, S, st))
            outs.append((dx, dw, dsc, dsh))
        for a, b, nm in zip(outs[0], outs[1], ("dx", "dw", "dscale", "dshift")):
            if a is not None:
                assert torch.equal(a, b), (nm, Cc, mod, key, site, p)
    # p = 0: the no-dropout path
    y0, y_rng = torch.empty_like(xc), torch.empty_like(xc)
    _lib.check(L.tm_op_prep_train(_lib.ptr(xc), _hp(w), _hp(sc), _hp(sh), None, 1.0, per_image, _lib.ptr(y0), N, Cc, Z, S, st))
    _lib.check(L.tm_op_prep_train_rng(_lib.ptr(xc), _hp(w), _hp(sc), _hp(sh), 77, 1, 0.0, per_image, _lib.ptr(y_rng), N, Cc, Z, S, st))
    assert torch.equal(y0, y_rng)


def _step(p, key, seed_case="mse_seed3", net_p=0.0):
    seed, loss_type, crop = GRAD_CASES[seed_case]
    cfg = PathConfig(**GRAD_CFG)
    sd = hashed_state_dict(cfg, 0)
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(seed)
    net = UNetTrain(cfg, sd, DEV, dropout_p=net_p)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    return training_loss_and_grads(net, sampler, x_pad, rna, t, mask, noise, crop, cfg.patch_size, loss_type, dropout_p=p, dropout_key=key)


def test_whole_model_dropout_gradients_vs_reference():
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_grad_dropout_ref.npz"))
    p, key = float(gold["p"]), int(gold["key"])
    cfg = PathConfig(**GRAD_CFG)
    sd = hashed_state_dict(cfg, 0)
    assert int(gold["sites"]) == len(dropout_sites(sd))
    name = "mse_seed3"
    loss, grads = _step(p, key)
    ref_loss = float(gold[f"{name}/loss"])
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    keys = sorted(k[len(name) + 6:] for k in gold.files if k.startswith(f"{name}/norm/"))
    assert keys == sorted(sd) and sorted(grads) == keys
    bad = []
    for k in keys:
        g = grads[k].double().reshape(-1).numpy()
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
    # the same key again: every bit; the net's own dropout_p gives the same step
    loss2, grads2 = _step(None, key, net_p=p)
    assert loss2 == loss and all(torch.equal(grads2[k], grads[k]) for k in keys)
    # another key: other masks, another loss
    loss3, _ = _step(p, derive_dropout_key(0, 1, 0))
    assert loss3 != loss


def test_dropout_p0_equals_eval_mode_bit_for_bit():
    loss0, g0 = _step(None, 0)
    loss1, g1 = _step(0.0, 0xFFFF)
    assert loss0 == loss1 and sorted(g0) == sorted(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert derive_dropout_key(0, 1, 0) != derive_dropout_key(0, 1, 1) != derive_dropout_key(0, 2, 1)


def test_forward_needs_a_key():
    cfg = PathConfig(**GRAD_CFG)
    net = UNetTrain(cfg, hashed_state_dict(cfg, 0), DEV, dropout_p=0.1)
    with pytest.raises(ValueError):
        net.forward(torch.zeros((8, cfg.in_channels, 64, 64)), torch.tensor([1, 2]), None, 2)
    with pytest.raises(ValueError):
        UNetTrain(cfg, hashed_state_dict(cfg, 0), DEV, dropout_p=1.0)
