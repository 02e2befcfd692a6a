"""-m gpu: the deeper prefetch of window_attn_mfma_kernel (tm_attn.hip: statistics pass 8 channel blocks per batch of loads, Q.K^T
fragments 4 channel blocks ahead, V staging 2 chunks ahead) changes when loads are issued, never the order of a sum or of the
MFMAs: its outputs equal those of the shallow form (TM_WIN_PREFETCH=0) byte for byte.  The depth is fixed per process, so each
setting runs in a fresh child (tests/win_prefetch_child.py: C = 128 / 512 with half-resolution kv / 256, N = 1 / 2 / 3, T = 128),
one after the other, each under its own time limit.  The values themselves are held to a float64 model by
test_gpu_window_attn.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "win_prefetch_child.py")


def _child(path, prefetch):
    env = dict(os.environ)
    env.pop("TM_WIN_PREFETCH", None)
    if prefetch is not None:
        env["TM_WIN_PREFETCH"] = prefetch
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, path]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, f"child (TM_WIN_PREFETCH={prefetch}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return np.load(path)


@pytest.mark.gpu
def test_prefetch_depth_does_not_change_a_byte(tmp_path):
    shallow = _child(str(tmp_path / "shallow.npz"), "0")
    deep = _child(str(tmp_path / "deep.npz"), None)
    assert sorted(shallow.files) == sorted(deep.files) == ["case0", "case1", "case2"]
    for k in shallow.files:
        a, b = shallow[k], deep[k]
        assert a.shape == b.shape
        assert not np.isnan(a.view(np.float32)).any() and not np.isnan(b.view(np.float32)).any(), f"{k}: output elements not written"
        assert a.tobytes() == b.tobytes(), f"{k}: {int((a != b).sum())} of {a.size} words differ between the prefetch depths"
