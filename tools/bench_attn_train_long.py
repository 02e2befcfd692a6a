#!/usr/bin/env python3
"""Timing driver of the training attention core (tm_op_window_attn_train) at one shape, made to run under
`rocprofv3 --kernel-trace --stats`: one warm-up and --reps forward + backward calls on random data.  `--summarize DIR` reads the
kernel trace a profiler run left in DIR and prints, per kernel, the calls after the warm-up: count, median, min, max in
microseconds (the spread of identical calls is the noise of the figure).  `--step K` instead times K optimizer steps (loss, all
gradients, clip, Adam; dropout 0.1) of the tiny rna_slc 8 configuration of tests/train_long_cases.py on each engine with
torch.cuda events, the engines interleaved after one warm-up step each, as tools/bench_train.py does for rna_slc 4.  The kernel
times and the step times of profiles/attn_train_long.txt were made with it.

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/bench_attn_train_long.py --shape 8,256,4,16
    python tools/bench_attn_train_long.py --summarize OUT
    python tools/bench_attn_train_long.py --step 3"""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(shape, reps):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import _lib
    N, C, Z, S = shape
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    q, k, v, d = (torch.randn((N, (C + 7) // 8, Z, S, S, 8), generator=g).to(dev) for _ in range(4))
    qw, kw = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    dqw, dkw = torch.empty(C), torch.empty(C)
    L, st = _lib.lib(), _lib.current_stream_ptr()
    for _ in range(1 + reps):
        _lib.check(L.tm_op_window_attn_train(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(qw), _lib.ptr(kw), None, _lib.ptr(o), None, None,
                                             None, None, None, N, C, Z, S, st), "forward")
        _lib.check(L.tm_op_window_attn_train(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(qw), _lib.ptr(kw), _lib.ptr(d), None, _lib.ptr(dq),
                                             _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(dqw), _lib.ptr(dkw), N, C, Z, S, st), "backward")
    print(f"shape N={N} C={C} Z={Z} S={S} T={Z * (S // 2) ** 2}: 1 warm-up + {reps} forward and backward calls")


def step(steps):
    import torch
    from train_cases import make_inputs
    from train_long_cases import SLC8_CFG
    from teramind_amd.config import PathConfig
    from teramind_amd.diffusion import SpacedDiffusionBeatGans
    from teramind_amd.train_model import AdamTrainer, UNetTrain, derive_dropout_key, training_loss_and_grads
    from teramind_amd.weights import hashed_state_dict
    cfg = PathConfig(**SLC8_CFG)
    sd = hashed_state_dict(cfg, 0)
    x_pad, rna, imgs, t, pos, mask, idx, noise = make_inputs(3, C=cfg.n_stain * cfg.z_size, srna=cfg.rna_slc)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    eng = {}
    for resident in (False, True):
        net = UNetTrain(cfg, sd, "cuda:0", dropout_p=0.1, resident=resident)
        eng[resident] = (net, AdamTrainer(net))

    def one(resident, i):
        net, opt = eng[resident]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        loss, grads = training_loss_and_grads(net, sampler, x_pad, rna, t, mask, noise, (1, 0), cfg.patch_size, "mse",
                                              dropout_key=derive_dropout_key(0, i, 0))
        opt.accumulate(grads)
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), loss

    for resident in (False, True):
        one(resident, 0)                                               # warm-up: allocator, first packs, code objects
    ms = {False: [], True: []}
    for i in range(steps):
        for resident in (False, True):
            dt, loss = one(resident, 1 + i)
            ms[resident].append(dt)
            print(f"step {i} resident={int(resident)} {dt:9.1f} ms  loss {loss:.6f}", flush=True)
    for resident in (False, True):
        v = ms[resident]
        print(f"{cfg.name} batch 2 resident={int(resident)}: median {statistics.median(v):.1f} ms, min {min(v):.1f}, max {max(v):.1f} over {steps} steps")


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    per = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"].split("(")[0]
        per.setdefault(name, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    print(f"{'kernel':72s} calls  median us     min us     max us")
    for name, calls in sorted(per.items()):
        if "attn" not in name and "reduce_dw" not in name:
            continue
        calls.sort()
        skip = len(calls) // 6 if len(calls) >= 6 else 0          # the warm-up's share of the calls (1 of 1 + 5)
        t = [c[1] for c in calls[skip:]]
        print(f"{name[:72]:72s} {len(t):5d} {statistics.median(t):10.1f} {min(t):10.1f} {max(t):10.1f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="8,256,4,16", help="N,C,Z,S")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--step", type=int, default=0)
    a = ap.parse_args()
    if a.step:
        step(a.step)
    elif a.summarize:
        summarize(a.summarize)
    else:
        run(tuple(int(x) for x in a.shape.split(",")), a.reps)
