#!/usr/bin/env python3
"""Measures the training step on one GPU: whole optimizer steps with the conv engine resident off and on, and the conv weight
gradient layer by layer, VALU kernel against MFMA kernel.

    python tools/bench_train.py [--tiny] [--rna_slc 16] [--steps 3] [--batch 2]

Builds the checkpoint configuration (PathConfig(), or the net_ch 16 one of tests/train_cases.py with --tiny) on hashed synthetic
weights and one synthetic batch, and runs two measurement parts, each in a child process of its own under `timeout -k 10`, the
second only if the first succeeded:
  step    one trainer per engine in the same process; optimizer steps (loss + all gradients + clip + Adam) timed with
          torch.cuda events around whole steps, the two engines interleaved (off, on, off, on, ...) after one warm-up step each.
          The resident=False figure measured here is the baseline.
  layers  the conv layer list of one training step (every conv() of the tape: N, Cin, Cout, Z, S, ksize), deduplicated, each
          timed with tm_op_conv_wgrad_time: hipEvents, one warm-up launch, `reps` repetitions of `iters` identical launches; the
          spread (max - min over repetitions) is the noise floor a claimed gain has to exceed.
TFLOP/s are executed ones: a tap whose input plane z + kz - 1 falls outside the volume is skipped, so a 3x3x3 layer at Z planes
counts 9 * (3 Z - 2) / Z taps per voxel; the yardstick is the 157.3 TFLOP/s fp32 MFMA peak.
Writes its section of profiles/train_wgrad_mfma.txt (one per configuration, below a "# ---- measurements" marker line; the lines
above the first marker, asm_scan's and the tests', and the other configuration's section are kept) and the raw figures as
profiles/train_wgrad_mfma.json (train_wgrad_mfma_tiny.json with --tiny).
--rna_slc 16 (every conv at Z = 8) trains on the resident engine only, so only that engine is timed, in the step and in the layers
(the VALU kernel takes Z <= 4); its section has its own marker and its figures go to train_wgrad_mfma[_tiny]_slc16.json."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK = 157.3


def _cfg(a):
    from teramind_amd.config import PathConfig
    from train_cases import GRAD_CFG
    return PathConfig(**(GRAD_CFG if a.tiny else {}), rna_slc=a.rna_slc)


def _engines(cfg):
    """the engines that train cfg: (resident off, on), or only on where the convs run at Z = 8"""
    return (False, True) if cfg.z_size <= 4 else (True,)


def _batch(cfg, b):
    from train_cases import make_inputs
    return make_inputs(3, b=b, ps=cfg.patch_size, C=cfg.n_stain * cfg.z_size, srna=cfg.rna_slc)


def part_step(a):
    import torch
    from teramind_amd.diffusion import SpacedDiffusionBeatGans
    from teramind_amd.train_model import AdamTrainer, UNetTrain, derive_dropout_key, training_loss_and_grads
    from teramind_amd.weights import hashed_state_dict
    cfg = _cfg(a)
    sd = hashed_state_dict(cfg, 0)
    x_pad, rna, imgs, t, pos, mask, idx, noise = _batch(cfg, a.batch)
    sampler = SpacedDiffusionBeatGans(1000, "ddpm")
    eng = {}
    for resident in _engines(cfg):
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

    ms = {False: [], True: []}
    for resident in _engines(cfg):
        one(resident, 0)                                              # warm-up: allocator, first packs, code objects
    for i in range(a.steps):
        for resident in _engines(cfg):
            dt, loss = one(resident, 1 + i)
            ms[resident].append(dt)
            print(f"step {i} resident={int(resident)} {dt:9.1f} ms  loss {loss:.6f}", flush=True)
    out = {"config": cfg.name, "tiny": a.tiny, "batch": a.batch, "params": sum(v.numel() for v in sd.values()),
           "off_ms": ms[False], "on_ms": ms[True]}
    json.dump(out, open(a.out, "w"))


def part_layers(a):
    import torch
    from teramind_amd import _lib
    from teramind_amd.train_model import UNetTrain
    from teramind_amd.weights import hashed_state_dict
    cfg = _cfg(a)
    sd = hashed_state_dict(cfg, 0)
    x_pad, rna, imgs, t, pos, mask, idx, noise = _batch(cfg, a.batch)
    seen = {}

    class Rec(UNetTrain):
        def conv(self, x, key):
            shp = self._shape[key + ".weight"]
            N, Z, S = self._geo(x.t)
            g = (N, shp[1], shp[0], Z, S, 1 if shp[2:] == (1, 1, 1) else 3)
            seen[g] = seen.get(g, 0) + 1
            return super().conv(x, key)

    net = Rec(cfg, sd, "cuda:0", resident=cfg.z_size > 4)
    ps, b = cfg.patch_size, a.batch
    g = torch.Generator().manual_seed(4)
    x = torch.randn((b * 4, cfg.in_channels, ps, ps), generator=g)
    rd = (torch.rand((b * 4, cfg.gn_sz, cfg.gn_sz, cfg.rna_slc * 500), generator=g) < 0.02).float() * 3.0
    net.forward(x, torch.tensor([17 + 100 * i for i in range(b)]), rd, b)
    net.tape = []
    del net
    torch.cuda.empty_cache()
    L = _lib.lib()
    rows = []
    for (N, ci, co, Z, S, ks), uses in sorted(seen.items(), key=lambda kv: (-kv[0][1] * kv[0][2], kv[0])):
        taps_exec = 1.0 if ks == 1 else 9.0 * (3 * Z - 2) / Z
        flop = 2.0 * N * Z * S * S * ci * co * taps_exec
        r = {"N": N, "Cin": ci, "Cout": co, "Z": Z, "S": S, "ksize": ks, "uses": uses, "gflop": flop / 1e9}
        for engine, nm in ((0, "valu"), (1, "mfma"))[0 if Z <= 4 else 1:]:
            buf = (C.c_float * a.reps)()
            iters = a.iters if engine else max(1, a.iters // 4)
            _lib.check(L.tm_op_conv_wgrad_time(N, ci, co, Z, S, ks, engine, iters, a.reps, C.cast(buf, C.c_void_p), None), "tm_op_conv_wgrad_time")
            v = sorted(buf)
            r[nm + "_ms"], r[nm + "_spread_ms"] = v[len(v) // 2], v[-1] - v[0]
            r[nm + "_tflops"] = flop / (v[len(v) // 2] * 1e-3) / 1e12
        rows.append(r)
        valu = f"valu {r['valu_ms']:8.3f} ms (+-{r['valu_spread_ms']:.3f})  " if "valu_ms" in r else ""
        print(f"{ci:5d}->{co:4d} k{ks} Z{Z} S{S:2d} N{N:2d} x{uses}  {valu}"
              f"mfma {r['mfma_ms']:8.3f} ms (+-{r['mfma_spread_ms']:.3f})  {r['mfma_tflops']:6.1f} TFLOP/s = {r['mfma_tflops'] / PEAK:.2f} of peak",
              flush=True)
    json.dump({"layers": rows}, open(a.out, "w"))


def report(a, step, layers, path_txt, path_json):
    lines = []
    w = lines.append
    w(f"# tools/bench_train.py{' --tiny' if a.tiny else ''}{f' --rna_slc {a.rna_slc}' if a.rna_slc != 4 else ''} --batch {a.batch} --steps {a.steps}   ({time.strftime('%Y-%m-%d')}, one MI355X)")
    w(f"config {step['config']}  parameters {step['params'] / 1e6:.1f} M  batch {a.batch} (x 4 patches)")
    med = lambda v: sorted(v)[len(v) // 2]                                                   # noqa: E731
    off, on = step["off_ms"], step["on_ms"]
    w("optimizer step (loss + all gradients + clip + Adam), engines interleaved in one process, ms per step:")
    if off:
        sp = max(max(off) - min(off), max(on) - min(on))
        w("  resident=False  " + "  ".join(f"{v:9.1f}" for v in off) + f"   median {med(off):9.1f}")
    w("  resident=True   " + "  ".join(f"{v:9.1f}" for v in on) + f"   median {med(on):9.1f}")
    if off:
        w(f"  gain {med(off) - med(on):.1f} ms per step ({med(off) / med(on):.2f} x), spread of identical steps {sp:.1f} ms: "
          + ("gain exceeds the spread" if med(off) - med(on) > sp else "GAIN DOES NOT EXCEED THE SPREAD"))
    else:
        w(f"  resident engine only (the host-weight engine takes Z <= 4); spread of identical steps {max(on) - min(on):.1f} ms")
    w("conv weight gradient per layer of the step (median of repetitions, spread = max - min of identical calls; executed TFLOP/s,")
    w(f"z-aware tap count, against the {PEAK} TFLOP/s fp32 MFMA peak):")
    w(f"  {'Cin':>5s} {'Cout':>5s} k Z {'S':>2s} {'N':>2s} uses {'valu ms':>9s} {'spread':>7s} {'mfma ms':>9s} {'spread':>7s} {'speed-up':>8s} {'TFLOP/s':>8s} {'of peak':>7s}")
    worse = []
    for r in layers["layers"]:
        if "valu_ms" not in r:
            w(f"  {r['Cin']:5d} {r['Cout']:5d} {r['ksize']} {r['Z']} {r['S']:2d} {r['N']:2d} {r['uses']:4d} {'-':>9s} {'-':>7s} "
              f"{r['mfma_ms']:9.3f} {r['mfma_spread_ms']:7.3f} {'-':>8s} {r['mfma_tflops']:8.1f} {r['mfma_tflops'] / PEAK:7.2f}")
            continue
        w(f"  {r['Cin']:5d} {r['Cout']:5d} {r['ksize']} {r['Z']} {r['S']:2d} {r['N']:2d} {r['uses']:4d} {r['valu_ms']:9.3f} {r['valu_spread_ms']:7.3f} "
          f"{r['mfma_ms']:9.3f} {r['mfma_spread_ms']:7.3f} {r['valu_ms'] / r['mfma_ms']:8.1f} {r['mfma_tflops']:8.1f} {r['mfma_tflops'] / PEAK:7.2f}")
        if min(r["Cin"], r["Cout"]) >= 64 and not r["valu_ms"] - r["mfma_ms"] > r["valu_spread_ms"] + r["mfma_spread_ms"]:
            worse.append(r)
    tv = sum(r.get("valu_ms", 0.0) * r["uses"] for r in layers["layers"])
    tm = sum(r["mfma_ms"] * r["uses"] for r in layers["layers"])
    if off:
        w(f"  sum over the step's conv calls: valu {tv:.1f} ms, mfma {tm:.1f} ms")
        w(f"  layers with Cin, Cout >= 64 where the MFMA kernel is not faster by more than the spread: {len(worse)}")
    else:
        w(f"  sum over the step's conv calls: mfma {tm:.1f} ms")
    # the record keeps everything above the first marker (the asm_scan and test lines) and the other configuration's section
    mark = "# ---- measurements" + (" (tiny" if a.tiny else " (checkpoint configuration") + (f", rna_slc {a.rna_slc})" if a.rna_slc != 4 else ")")
    old = open(path_txt).read() if os.path.exists(path_txt) else ""
    parts = old.split("# ---- measurements")
    keep = [parts[0]] + ["# ---- measurements" + p for p in parts[1:] if not ("# ---- measurements" + p).startswith(mark)]
    open(path_txt, "w").write("".join(k if k.endswith("\n") or not k else k + "\n" for k in keep) + mark + "\n" + "\n".join(lines) + "\n")
    json.dump({"step": step, "layers": layers["layers"]}, open(path_json, "w"), indent=1)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--rna_slc", type=int, choices=(4, 8, 16), default=4, help="16: every conv at Z = 8, resident engine only")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--part", choices=("step", "layers"), default=None, help="internal: run one measurement part")
    ap.add_argument("--out", default=None)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per part")
    a = ap.parse_args()
    if a.part:
        return (part_step if a.part == "step" else part_layers)(a)
    os.makedirs(a.outdir, exist_ok=True)
    res = {}
    for part in ("step", "layers"):                                   # each under its own time limit; nothing runs after a failure
        out = os.path.join(a.outdir, f".bench_train_{part}.json")
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--part", part, "--out", out, "--batch",
               str(a.batch), "--steps", str(a.steps), "--iters", str(a.iters), "--reps", str(a.reps), "--rna_slc", str(a.rna_slc)] + (["--tiny"] if a.tiny else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"bench_train: part {part} ended with status {rc}; nothing further was started")
        res[part] = json.load(open(out))
        os.remove(out)
    sfx = ("_tiny" if a.tiny else "") + (f"_slc{a.rna_slc}" if a.rna_slc != 4 else "")
    report(a, res["step"], res["layers"], os.path.join(a.outdir, "train_wgrad_mfma.txt"), os.path.join(a.outdir, f"train_wgrad_mfma{sfx}.json"))


if __name__ == "__main__":
    main()
