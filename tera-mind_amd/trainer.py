"""The training loop of the reference (experiment.py:121-219: `training_step`, gradient accumulation, clip + Adam) over
resident tiles, with checkpoints the reference's own loaders accept (experiment.py:50-58, test_brn.py:140-147).

One optimizer step = `accum_batches` micro-batches of
    dataset draw -> F.pad by half a patch + loss mask (experiment.py:160-168) -> t ~ U[0, 1000) per image, the 2 x 2-patch
    window (ix, iy) ~ U (diffusion/base.py:221-222) -> noise -> train_model.training_loss_and_grads -> AdamTrainer.accumulate
followed by AdamTrainer.step().  Every random quantity is a pure function of (seed, step, micro, rank): the data draw and
(t, ix, iy) come from dataset.keyed_rng, the noise from a device generator seeded from the same key, the dropout masks from
train_model.derive_dropout_key.  A run resumed from a checkpoint therefore continues bit for bit.

Data-parallel (`world` > 1, one process per rank in a process group: launch.spawn_ranks / launch.init_distributed): `rank` /
`world` select the data share, and every optimizer step sums the ranks' accumulated gradients in rank order before clip + Adam
(train_dist.GradExchange), so all ranks hold bit-identical parameters after every step with nothing broadcast.  `world` = 1 runs
no exchange.
"""
import dataclasses
import hashlib
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .config import PathConfig
from .dataset import STREAM_STEP, TileSampler, TrainTileSet, keyed_rng
from .diffusion import SpacedDiffusionBeatGans
from .train_dist import GradExchange, require_group
from .train_model import AdamTrainer, UNetTrain, derive_dropout_key, training_loss_and_grads

CKPT_FORMAT = 1
_CFG_FIELDS = ("patch_size", "rna_slc", "stain", "rna_num", "mouse", "method", "net_ch", "ch_mult", "embed_ch", "attn_res",
               "num_res_blocks", "T", "beta_scheduler", "gen_type")


def step_randoms(seed: int, step: int, micro: int, rank: int, batch: int, n_patch: int) -> Tuple[np.ndarray, int, int]:
    """(t int64 [batch] in [0, 1000), ix, iy in [0, n_patch)) of one micro-batch: `torch.randint(0, 1000, ...)` of
    experiment.py:128 and the two `random.randrange(pos.shape[k] - 1)` of diffusion/base.py:221-222, from the keyed generator."""
    rng = keyed_rng(seed, STREAM_STEP, 0, step, micro, rank)
    t = rng.integers(0, 1000, batch).astype(np.int64)
    ix, iy = int(rng.integers(0, n_patch)), int(rng.integers(0, n_patch))
    return t, ix, iy


def step_noise(seed: int, step: int, micro: int, rank: int, shape, device) -> torch.Tensor:
    """Standard normal noise of one micro-batch from a device generator seeded from (seed, step, micro, rank)."""
    h = hashlib.blake2b(f"teramind-noise/{int(seed)}/{int(step)}/{int(micro)}/{int(rank)}".encode(), digest_size=8).digest()
    g = torch.Generator(device=device)
    g.manual_seed(int.from_bytes(h, "little") >> 1)
    return torch.randn(tuple(shape), generator=g, device=device, dtype=torch.float32)


def rank_mean(values) -> float:
    """Mean of one float per rank, added in rank order in float64 (the logged loss of a data-parallel step)."""
    s = 0.0
    for v in values:
        s += float(v)
    return s / len(values)


def pad_and_mask(img: torch.Tensor, patch_size: int):
    """experiment.py:156-168: the image padded by half a patch and the loss mask that is 1 on the unpadded part."""
    halfp = patch_size // 2
    H, W = img.shape[2:]
    assert H % patch_size == 0 and W % patch_size == 0
    x_pad = F.pad(img, (halfp, halfp, halfp, halfp))
    mask = torch.zeros_like(x_pad)
    mask[:, :, halfp:-halfp, halfp:-halfp] = 1.0
    return x_pad, mask


def config_to_dict(cfg: PathConfig) -> Dict[str, object]:
    d = dataclasses.asdict(cfg)
    return {k: (list(d[k]) if isinstance(d[k], tuple) else d[k]) for k in _CFG_FIELDS}


def config_from_dict(d: Dict[str, object]) -> PathConfig:
    return PathConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in d.items() if k in _CFG_FIELDS})


def make_checkpoint(cfg: PathConfig, state: Dict[str, torch.Tensor], global_step: int = 0, adam_m=None, adam_v=None, adam_t: int = 0,
                    seed: int = 0, epoch: int = 0, epoch_batch: int = 0, hparams: Optional[Dict[str, object]] = None) -> Dict[str, object]:
    """The checkpoint dictionary: tensors, numbers, strings, lists and dicts only (loads under `weights_only=True`).
    `state_dict` carries the reference's LitModel keys ('model.' + parameter name), `global_step` as Lightning names it."""
    host = lambda t: torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous().clone()    # noqa: E731
    ck = {"format": CKPT_FORMAT, "state_dict": {"model." + k: host(v) for k, v in state.items()}, "global_step": int(global_step),
          "config_name": cfg.name, "config": config_to_dict(cfg), "seed": int(seed), "epoch": int(epoch), "epoch_batch": int(epoch_batch),
          "adam_step": int(adam_t), "hparams": dict(hparams or {})}
    if adam_m is not None:
        ck["adam_m"] = {k: host(v) for k, v in adam_m.items()}
        ck["adam_v"] = {k: host(v) for k, v in adam_v.items()}
    return ck


def load_checkpoint(path) -> Dict[str, object]:
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or "state_dict" not in ck:
        raise ValueError(f"{path}: not a training checkpoint (no state_dict)")
    return ck


class Trainer:
    def __init__(self, cfg: PathConfig, state: Dict[str, "object"], tiles: TrainTileSet, batch_size: int, accum_batches: int = 1,
                 seed: int = 0, dropout_p: float = 0.1, lr: float = 2e-5, grad_clip: float = 1.0, loss_type: str = "mse",
                 rank: int = 0, world: int = 1, resident: bool = False, exchange=None):
        """`exchange`: with world > 1, the gradient exchange to use in place of a train_dist.GradExchange over the process group
        (an object with `world`, `reduce_(g)` and `all_gather_scalars(x)`; tests emulate the ranks in one process with it)."""
        if loss_type not in ("mse", "l1"):
            raise ValueError(f"loss_type {loss_type!r}")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank {rank} of world {world}")
        if world > 1 and exchange is None:
            require_group(world)                                           # raises before anything is built
        g = tiles.geo
        if g.sdim % cfg.patch_size or g.snum != cfg.rna_slc:
            raise ValueError("tile set geometry does not match the model config")
        self.cfg, self.tiles, self.batch, self.accum, self.seed = cfg, tiles, int(batch_size), int(accum_batches), int(seed)
        self.loss_type, self.rank, self.world = loss_type, int(rank), int(world)
        self.net = UNetTrain(cfg, state, tiles.dev, dropout_p=dropout_p, resident=resident)
        self.opt = AdamTrainer(self.net, lr=lr, grad_clip=grad_clip)
        if self.world > 1:
            self.opt.exchange = exchange or GradExchange(self.opt.n, self.rank, self.world, self.net.dev)
        self.diffusion = SpacedDiffusionBeatGans(cfg.T, "ddpm", cfg.T, cfg.beta_scheduler)
        s = tiles.sampler
        self.sampler = TileSampler(s.entries, s.H, s.W, g, self.seed, gmax=s.gmax, accum_batches=self.accum)
        self.sampler.batches_per_epoch(self.batch, self.world)             # raises if the list cannot fill one batch
        self.global_step = 0

    # -- one micro-batch -------------------------------------------------------------------------
    def micro_batch(self, step: int, micro: int):
        """Everything training_loss_and_grads needs for micro-batch `micro` of step `step` (all queued, nothing awaited):
        (x_pad, rna_dense, t, mask, noise, (ix, iy), dropout_key)."""
        bt = self.tiles.gather(self.sampler.params(self.batch, step, micro, self.rank, self.world))
        x_pad, mask = pad_and_mask(bt.img, self.cfg.patch_size)
        t, ix, iy = step_randoms(self.seed, step, micro, self.rank, self.batch, self.tiles.geo.sdim // self.cfg.patch_size)
        noise = step_noise(self.seed, step, micro, self.rank, x_pad.shape, self.tiles.dev)
        return x_pad, bt.rna, torch.from_numpy(t), mask, noise, (ix, iy), derive_dropout_key(self.seed, step, micro, self.rank)

    def step(self) -> Dict[str, float]:
        losses = []
        for micro in range(self.accum):
            x_pad, rna, t, mask, noise, crop, key = self.micro_batch(self.global_step, micro)
            loss, grads = training_loss_and_grads(self.net, self.diffusion, x_pad, rna, t, mask, noise, crop, self.cfg.patch_size,
                                                  self.loss_type, dropout_key=key)
            self.opt.accumulate(grads)
            losses.append(loss)
        info = self.opt.step()
        self.global_step += 1
        loss = float(np.mean(losses))
        if self.opt.exchange is not None:                                  # the mean over ranks, added in rank order on the host
            loss = rank_mean(self.opt.exchange.all_gather_scalars(loss))
        return {"step": self.global_step, "loss": loss, "grad_norm": info["grad_norm"], "clip_coef": info["clip_coef"]}

    # -- checkpoints -----------------------------------------------------------------------------
    def _split(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return self.opt.layout.split(flat.cpu())

    def checkpoint(self) -> Dict[str, object]:
        epoch, k = self.sampler.position(self.batch, self.global_step, 0, self.world)
        hp = {"batch_size": self.batch, "accum_batches": self.accum, "dropout_p": self.net.dropout_p, "lr": self.opt.lr,
              "grad_clip": self.opt.clip, "loss_type": self.loss_type}
        if self.net.resident:
            hp["resident"] = True
        if self.world > 1:
            hp["world"] = self.world
        return make_checkpoint(self.cfg, self.net.W, self.global_step, self._split(self.opt.m), self._split(self.opt.v), self.opt.t,
                               self.seed, epoch, k, hp)

    def save(self, path):
        """Every rank holds the same state; in a data-parallel run rank 0 saves."""
        torch.save(self.checkpoint(), path)

    @classmethod
    def resume(cls, path, tiles: TrainTileSet, cfg: Optional[PathConfig] = None, rank: int = 0, world: int = 1,
               resident: Optional[bool] = None, exchange=None) -> "Trainer":
        """A trainer that continues the run saved at `path`; cfg defaults to the one stored in the checkpoint, `resident` to the
        engine the run was saved with.  A data-parallel run (hparams['world']) is resumed by every rank from rank 0's file."""
        from .weights import strip_lightning_state_dict
        ck = load_checkpoint(path)
        cfg = cfg or config_from_dict(ck["config"])
        if cfg.name != ck["config_name"]:
            raise ValueError(f"checkpoint of {ck['config_name']!r} resumed with config {cfg.name!r}")
        hp = ck["hparams"]
        if int(hp.get("world", 1)) != int(world):
            raise ValueError(f"checkpoint of a world = {hp.get('world', 1)} run resumed with world = {world}: the data shares differ")
        tr = cls(cfg, strip_lightning_state_dict(ck), tiles, hp["batch_size"], hp["accum_batches"], ck["seed"], hp["dropout_p"], hp["lr"],
                 hp["grad_clip"], hp["loss_type"], rank, world, bool(hp.get("resident", False)) if resident is None else bool(resident), exchange)
        tr.global_step = int(ck["global_step"])
        if "adam_m" in ck:
            o = tr.opt
            o.m = o.layout.flatten(ck["adam_m"]).to(tr.net.dev)
            o.v = o.layout.flatten(ck["adam_v"]).to(tr.net.dev)
            o.t = int(ck["adam_step"])
        return tr
