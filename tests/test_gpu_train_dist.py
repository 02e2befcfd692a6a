"""-m gpu: data-parallel training on ONE GPU.  Two fresh rank processes (teramind_amd.launch.spawn_ranks, gloo, both on cuda:0)
train the tiny configuration of tests/train_cases.py as ranks 0 and 1 of one run (tests/train_dist_worker.py); everything of the
N-GPU path runs -- the rank's data share and random streams, the gradient exchange with tm_op_rank_sum, the replicated clip +
Adam, the rank-averaged loss, rank 0's checkpoint and its resumption by every rank -- except RCCL itself (one GPU cannot host two
RCCL ranks).  Because the order of every sum is fixed (micro-batches in index order, then ranks in index order), the run must
equal, bit for bit, an emulation of its two ranks inside this process.  Both engines: host weights and resident.

The parent holds the GPU for the emulation, so at most three processes have it open at once."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from train_cases import GRAD_CFG
from teramind_amd import launch, synth
from teramind_amd.config import PathConfig
from teramind_amd.dataset import TrainTileSet
from teramind_amd.train_model import training_loss_and_grads
from teramind_amd.trainer import Trainer, load_checkpoint, rank_mean
from teramind_amd.weights import hashed_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "train_dist_worker.py")
DEV = "cuda:0"
SEED, BATCH, ACCUM, DROPOUT, WORLD = 7, 2, 2, 0.1, 2             # as tests/train_dist_worker.py
ENGINES = [False, True]                                          # resident


@pytest.fixture(scope="module")
def cfg():
    return PathConfig(**GRAD_CFG)


@pytest.fixture(scope="module")
def tile_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("tiles")
    synth.write_train_tile_dir(root, n_tiles=2, H=320, W=320, zt=6, nnz=300000, seed=1)
    return str(root)


@pytest.fixture(scope="module")
def tiles(cfg, tile_root):
    return TrainTileSet(os.path.join(tile_root, "gene"), cfg, DEV, seed=SEED, repeat=4, accum_batches=ACCUM)


def _spawn(tile_root, out_dir, resident, backend):
    """Two fresh rank processes; a failed or timed-out rank fails the test and nothing further is started.  The limit covers two
    interpreter starts that share a GPU and three optimizer steps of two micro-batches per rank."""
    rc = launch.spawn_ranks(WORLD, [WORKER, tile_root, str(out_dir), str(int(resident)), backend], timeout=600)
    assert rc == 0, f"rank processes failed or timed out (exit code {rc})"
    ranks = []
    for r in range(WORLD):
        d = json.load(open(os.path.join(out_dir, f"rank{r}.json")))
        d["bits"] = {k: torch.from_numpy(np.load(os.path.join(out_dir, f"rank{r}_{k}.npy"))) for k in ("p", "m", "v")}
        ranks.append(d)
    return ranks


_runs = {}


@pytest.fixture(scope="module")
def run(tile_root, tmp_path_factory):
    """run(resident) -> what the two ranks of the gloo rehearsal wrote; each engine is run once per module."""
    def get(resident):
        if resident not in _runs:
            _runs[resident] = None                                # a failed spawn is not repeated by the next test
            _runs[resident] = _spawn(tile_root, tmp_path_factory.mktemp(f"ranks{int(resident)}"), resident, "gloo")
        if _runs[resident] is None:
            pytest.fail("the rank processes of this engine failed in an earlier test")
        return _runs[resident]
    yield get
    _runs.clear()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _digest(opt):
    return {k: hashlib.sha256(_bits(getattr(opt, k)).numpy().tobytes()).hexdigest() for k in ("p", "m", "v")}


def _assert_ranks_agree(ranks):
    a, b = ranks
    assert (a["rank"], b["rank"]) == (0, 1) and a["world"] == b["world"] == WORLD
    for k in ("p", "m", "v"):
        assert torch.equal(a["bits"][k], b["bits"][k]), f"{k}: the ranks' bits differ after step 2"
    assert a["after1"] == b["after1"] and a["after2"] == b["after2"]
    assert a["infos"] == b["infos"]                               # loss, grad_norm, clip_coef of both steps: the same floats
    assert all(np.isfinite(i["loss"]) and i["grad_norm"] > 0 and 0 < i["clip_coef"] <= 1 for i in a["infos"])
    assert a["after1"] != a["after2"] and float(a["bits"]["v"].view(torch.float32).abs().sum()) > 0


@pytest.mark.parametrize("resident", ENGINES)
def test_two_ranks_hold_identical_bits(run, resident):
    ranks = run(resident)
    assert all(r["backend"] == "gloo" and r["device"] == "cuda:0" for r in ranks)
    _assert_ranks_agree(ranks)
    n = ranks[0]["n"]
    shard = (-(-n // WORLD) + 3) // 4 * 4
    assert all(r["bytes_sent"] == 2 * 4 * 2 * (WORLD - 1) * shard for r in ranks)          # two steps of ring all-reduce traffic


class Presummed:
    """The exchange of the in-process emulation: the test has already put g0 + g1 into every rank's gradient arena, so nothing
    moves; AdamTrainer.step() reads `world` for its average, 1 / (micro * world)."""
    world = WORLD

    def reduce_(self, g):
        return g


def emulate(cfg, tiles, resident, steps=2):
    """Ranks 0 and 1 of a world-2 run in this process, without a process group, from the public pieces: each rank's micro-batches
    (Trainer.micro_batch -> training_loss_and_grads -> AdamTrainer.accumulate), their gradient arenas added with ONE torch add,
    g0 + g1, then both optimizers step with avg = 1 / 4.  -> (trainers, infos per step)."""
    trs = [Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=ACCUM, seed=SEED, dropout_p=DROPOUT, rank=r, world=WORLD,
                   resident=resident, exchange=Presummed()) for r in range(WORLD)]
    infos = []
    for step in range(steps):
        means = []
        for tr in trs:
            losses = []
            for micro in range(ACCUM):
                x_pad, rna, t, mask, noise, crop, key = tr.micro_batch(step, micro)
                loss, grads = training_loss_and_grads(tr.net, tr.diffusion, x_pad, rna, t, mask, noise, crop, cfg.patch_size, "mse", dropout_key=key)
                tr.opt.accumulate(grads)
                losses.append(loss)
            means.append(float(np.mean(losses)))
        gsum = trs[0].opt.g + trs[1].opt.g
        step_infos = []
        for tr in trs:
            tr.opt.g = gsum.clone()
            step_infos.append(tr.opt.step())
            tr.global_step += 1
        assert step_infos[0] == step_infos[1]
        infos.append({"step": step + 1, "loss": rank_mean(means), **step_infos[0]})
    return trs, infos


@pytest.mark.parametrize("resident", ENGINES)
def test_two_rank_run_equals_in_process_emulation(run, cfg, tiles, resident):
    ranks = run(resident)
    trs, infos = emulate(cfg, tiles, resident)
    for k in ("p", "m", "v"):
        assert torch.equal(_bits(getattr(trs[0].opt, k)), _bits(getattr(trs[1].opt, k)))
        assert torch.equal(_bits(getattr(trs[0].opt, k)), ranks[0]["bits"][k]), f"{k}: the run differs from its emulation"
    assert _digest(trs[0].opt) == ranks[0]["after2"]
    assert infos == ranks[0]["infos"]
    # the ranks drew different data, noise and dropout masks: their own gradients differed
    a, b = trs[0].micro_batch(0, 0), trs[1].micro_batch(0, 0)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[4], b[4]) and a[6] != b[6]


@pytest.mark.parametrize("resident", ENGINES)
def test_resume_from_rank0_checkpoint_continues_bit_for_bit(run, resident):
    """1 + save + resume + 1 == 2, on every rank, from the one file rank 0 wrote."""
    for r in run(resident):
        assert r["after_resumed"] == r["after2"], f"rank {r['rank']}: the resumed step differs"
        assert r["info_resumed"] == r["infos"][1]


@pytest.mark.parametrize("resident", ENGINES)
def test_world_two_step_differs_from_world_one(run, cfg, tiles, resident):
    """The exchange is live: on the same seed a world-1 step ends elsewhere than the first step of the world-2 run."""
    ranks = run(resident)
    one = Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=ACCUM, seed=SEED, dropout_p=DROPOUT, resident=resident)
    assert one.opt.exchange is None
    info = one.step()
    d = _digest(one.opt)
    assert d["p"] != ranks[0]["after1"]["p"] and d["m"] != ranks[0]["after1"]["m"]
    assert info["grad_norm"] != ranks[0]["infos"][0]["grad_norm"]
    assert "world" not in one.checkpoint()["hparams"]             # a single-rank checkpoint keeps its bytes


def test_world_two_without_a_process_group_raises(cfg, tiles):
    import torch.distributed as dist
    assert not dist.is_initialized()
    with pytest.raises(RuntimeError, match="launch.init_distributed"):
        Trainer(cfg, hashed_state_dict(cfg, 0), tiles, BATCH, accum_batches=ACCUM, seed=SEED, dropout_p=DROPOUT, rank=0, world=2)


def _train_cli(tile_root, out_dir, extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--data", os.path.join(tile_root, "gene"), "--out", str(out_dir),
           "--steps", "1", "--batch_size", "2", "--accum_batches", "1", "--repeat", "4", "--seed", str(SEED)] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_train_cli_two_ranks_rehearsed(tile_root, tmp_path):
    """tools/train.py --gpus 2 --rehearse: the tool starts its own two ranks; rank 0 alone prints and saves."""
    lines = _train_cli(tile_root, tmp_path, ["--gpus", "2", "--rehearse"])
    assert len(lines) == 1 and lines[0]["step"] == 1 and np.isfinite(lines[0]["loss"]) and lines[0]["grad_norm"] > 0
    assert os.listdir(tmp_path) == ["last.ckpt"]
    ck = load_checkpoint(os.path.join(tmp_path, "last.ckpt"))
    assert ck["global_step"] == 1 and ck["hparams"]["world"] == 2 and ck["hparams"]["accum_batches"] == 1


def test_two_ranks_over_rccl_hold_identical_bits(tile_root, tmp_path):
    """The real thing, for the first box with two GPUs: one rank per GPU, backend nccl, the exchange on the device.  Skipped on the
    one-GPU boxes this repository has been developed on -- where it has therefore never run."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    ranks = _spawn(tile_root, tmp_path, False, "nccl")
    assert [r["device"] for r in ranks] == ["cuda:0", "cuda:1"] and all(r["backend"] == "nccl" for r in ranks)
    _assert_ranks_agree(ranks)
    if _runs.get(False):                                          # and the same bits as the gloo rehearsal: the route is free
        assert ranks[0]["after2"] == _runs[False][0]["after2"]
