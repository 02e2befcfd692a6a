"""bench.py's command line: `--dump-outputs DIR` (what the timed path computed in its last step, float32, bounded in size)
and the split between a plain run (the headline figures only) and `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_whole_or_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 100)          # 50 float32 elements per array for two arrays
    small = torch.arange(24, dtype=torch.bfloat16).reshape(2, 3, 4)
    big = torch.arange(1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big})
    bench.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big})
    s, g = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3, 4) and np.array_equal(s, small.float().numpy())
    # the sample: 50 elements of `big` in index order, the same ones on every call
    assert g.dtype == np.float32 and g.shape == (50,)
    assert np.all(np.diff(g) >= 0) and np.all((g >= 0) & (g < 1000) & (g == np.round(g)))
    assert np.array_equal(g, np.load(tmp_path / "b" / "big.npy"))
    assert s.nbytes + g.nbytes <= 4 * 100


def _run(args, out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(out)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_full_computes_the_same(tmp_path):
    plain = _run([], tmp_path / "plain")
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["dtype"] == "f32" and plain["higher_is_better"] is True
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "interior patch-steps/s"
    assert not {"roofline", "sweep", "extra", "cpu_baseline"} & set(plain)
    full = _run(["--full", "--no-sweep", "--no-cpu-baseline"], tmp_path / "full")
    assert 0 < full["roofline"]["frac"] <= 1.0 and full["roofline"]["launches_timed"] > 0
    for name, shape in (("state", (32, 4, 64, 64)), ("eps", (32, 4, 64, 64))):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
        assert np.array_equal(a, b), f"{name}: the hipEvent brackets of --full changed what the step computes"
