#!/usr/bin/env python3
"""Trains the patch UNet from a directory of tiles (reference train.py:9-39 -> experiment.py:121-219, 458-461) on one GPU or,
with --gpus N, data-parallel on N (experiment.py:449-490): resident tiles, batches drawn on the device, gradient accumulation to
64 samples per rank and optimizer step (config_parm.py:45), clip + Adam, a checkpoint every --save_every steps and at the end.
One JSON line per optimizer step.

    python tools/make_train_tiles.py --out /tmp/tiles
    python tools/train.py --data /tmp/tiles/gene --out /tmp/run --steps 2 --batch_size 2
    python tools/train.py --data /tmp/tiles/gene --out /tmp/run --steps 2 --batch_size 2 --gpus 2 [--rehearse]

--gpus N: this process starts N fresh rank processes (teramind_amd.launch.spawn_ranks) before it touches a GPU, rank r on
cuda:r over RCCL; every optimizer step sums the ranks' gradients in rank order (teramind_amd.train_dist), so all ranks hold the
same bits and rank 0 alone prints and saves.  --rehearse: every rank on cuda:0 over gloo (a one-GPU box checks the plumbing).

--ckpt: a checkpoint written by this tool (the run continues where it stopped, bit for bit) or any reference checkpoint
(its weights are loaded, the optimizer starts fresh)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import teramind_amd  # noqa: E402,F401
from teramind_amd import launch  # noqa: E402      (imports neither torch nor the HIP library)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch_size", "-b", type=int, default=32)
    ap.add_argument("--patch_size", "-ps", type=int, default=64)
    ap.add_argument("--rna_slc", type=int, choices=(1, 4, 8, 16), default=4, help="UNetTrain covers rna_slc 1 (patch 64, 128), 4, 8 and, "
                    "with --resident at patch size 64, 16")
    ap.add_argument("--mouse", default="638850", choices=["609882", "609889", "638850"])
    ap.add_argument("--stain", default="all", choices=["DAPI", "PolyT", "all"])
    ap.add_argument("--data", required=True, help="directory of gene .npz tiles (images: the same paths with gene -> img, .npz -> .zip)")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", required=True, help="directory for checkpoints")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--save_every", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=10, help="repetitions of the tile list per epoch (MBADataset repeat)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--resident", action="store_true", help="conv weights packed on the GPU once per optimizer step, conv gradients "
                    "kept there, weight gradient on the matrix pipe (UNetTrain(resident=True))")
    ap.add_argument("--accum_batches", type=int, default=None, help="micro-batches per optimizer step and rank (default: 64 // batch_size)")
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel ranks, one process per GPU")
    ap.add_argument("--rehearse", action="store_true", help="--gpus N on a one-GPU box: every rank on cuda:0, gloo instead of RCCL")
    a = ap.parse_args()
    if a.rna_slc == 16 and not a.resident:
        ap.error("--rna_slc 16 needs --resident: its convs run at Z = 8, and the host-weight engine's weight gradient takes Z <= 4")
    if a.gpus > 1 and not launch.launched_as_rank():
        sys.exit(launch.spawn_ranks(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))
    train(a)


def train(a):
    from teramind_amd.config import prep_config_parm
    from teramind_amd.dataset import TrainTileSet
    from teramind_amd.trainer import Trainer, load_checkpoint
    from teramind_amd.weights import hashed_state_dict, strip_lightning_state_dict
    rank, world = 0, 1
    if a.gpus > 1:
        import torch
        rank, local_rank, world = launch.dist_env()
        if world != a.gpus:
            raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE is {world}")
        a.device = "cuda:0" if a.rehearse else f"cuda:{local_rank}"
        torch.cuda.set_device(torch.device(a.device))
        launch.init_distributed("gloo" if a.rehearse else "nccl", a.device)
    nrna = 500 if a.mouse in ("609882", "609889") else 229
    cfg = prep_config_parm(a.data, a.batch_size, a.patch_size, 1, a.stain, a.mouse, nrna, a.rna_slc)
    accum = a.accum_batches or max(1, 64 // a.batch_size)
    tiles = TrainTileSet(a.data, cfg, a.device, seed=a.seed, repeat=a.repeat, accum_batches=accum)
    os.makedirs(a.out, exist_ok=True)
    if a.ckpt and "hparams" in load_checkpoint(a.ckpt):
        tr = Trainer.resume(a.ckpt, tiles, cfg, rank, world, resident=True if a.resident else None)
    else:
        state = strip_lightning_state_dict(load_checkpoint(a.ckpt)) if a.ckpt else hashed_state_dict(cfg, a.seed)
        tr = Trainer(cfg, state, tiles, a.batch_size, accum, a.seed, rank=rank, world=world, resident=a.resident)
    for _ in range(a.steps):
        t0 = time.time()
        info = tr.step()
        info["seconds"] = round(time.time() - t0, 3)
        if rank == 0:
            print(json.dumps(info), flush=True)
            if tr.global_step % a.save_every == 0:
                tr.save(os.path.join(a.out, f"step_{tr.global_step}.ckpt"))
    if rank == 0:
        tr.save(os.path.join(a.out, "last.ckpt"))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
