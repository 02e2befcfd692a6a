"""Rank process of the data-parallel training tests (tests/test_gpu_train_dist.py): started by teramind_amd.launch.spawn_ranks,
trains the tiny configuration of tests/train_cases.py (GRAD_CFG, batch 2, two micro-batches per step, dropout 0.1) for two
optimizer steps as one rank of a data-parallel run, rank 0 saving a checkpoint after the first; then every rank resumes that
checkpoint and repeats the second step.  Writes rank{r}_{p,m,v}.npy (int32 views of the parameters and both Adam moments after
step 2) and rank{r}.json (per-step loss / grad_norm / clip_coef, SHA-256 digests of the state after step 1, step 2 and the resumed
step 2).
argv: tile_root out_dir resident(0|1) backend(gloo|nccl)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import teramind_amd  # noqa: E402,F401
import torch  # noqa: E402

from teramind_amd import launch  # noqa: E402
from teramind_amd.config import PathConfig  # noqa: E402
from teramind_amd.dataset import TrainTileSet  # noqa: E402
from teramind_amd.trainer import Trainer  # noqa: E402
from teramind_amd.weights import hashed_state_dict  # noqa: E402
from train_cases import GRAD_CFG  # noqa: E402

SEED, BATCH, ACCUM, DROPOUT = 7, 2, 2, 0.1


def state_bits(opt):
    """{p, m, v} -> int32 numpy views of the optimizer arena."""
    return {k: getattr(opt, k).detach().cpu().contiguous().view(torch.int32).numpy() for k in ("p", "m", "v")}


def digest(opt):
    return {k: hashlib.sha256(a.tobytes()).hexdigest() for k, a in state_bits(opt).items()}


def main():
    root, out_dir, resident, backend = sys.argv[1], sys.argv[2], bool(int(sys.argv[3])), sys.argv[4]
    _, local_rank, _ = launch.dist_env()
    dev = "cuda:0" if backend == "gloo" else f"cuda:{local_rank}"            # gloo: every rank shares the one GPU
    torch.cuda.set_device(torch.device(dev))
    rank, _, world = launch.init_distributed(backend, dev)
    import torch.distributed as dist
    cfg = PathConfig(**GRAD_CFG)
    tiles = TrainTileSet(os.path.join(root, "gene"), cfg, dev, seed=SEED, repeat=4, accum_batches=ACCUM)
    tr = Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=ACCUM, seed=SEED, dropout_p=DROPOUT, rank=rank, world=world,
                 resident=resident)
    ckpt = os.path.join(out_dir, "step1.ckpt")
    infos = [tr.step()]
    after1 = digest(tr.opt)
    if rank == 0:
        tr.save(ckpt)
    dist.barrier()                                                 # the file is complete before any rank reads it
    infos.append(tr.step())
    for k, a in state_bits(tr.opt).items():
        np.save(os.path.join(out_dir, f"rank{rank}_{k}.npy"), a)
    after2, sent = digest(tr.opt), tr.opt.exchange.bytes_sent
    del tr
    resumed = Trainer.resume(ckpt, tiles, rank=rank, world=world)
    assert resumed.global_step == 1 and resumed.net.resident == resident
    info_resumed = resumed.step()
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump({"rank": rank, "world": world, "backend": dist.get_backend(), "device": dev, "infos": infos, "info_resumed": info_resumed,
                   "after1": after1, "after2": after2, "after_resumed": digest(resumed.opt), "bytes_sent": sent, "n": resumed.opt.n}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
