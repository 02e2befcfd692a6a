"""Child process of test_gpu_window_attn_prefetch.py: runs tm_op_window_attn_kv (fp32) on fixed inputs for every case and saves the
raw output bytes.  The prefetch depth of window_attn_mfma_kernel is fixed per process (TM_WIN_PREFETCH, read at the first launch),
so the parent starts one child per setting.  usage: win_prefetch_child.py OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import teramind_amd  # noqa: E402,F401
import util  # noqa: E402
from teramind_amd import _lib  # noqa: E402

# (C, S, N, kv_half): windows of T = Z * (S / 2) ^ 2 = 128 tokens at Z = 2
CASES = [(128, 16, 1, 0), (512, 16, 2, 1), (256, 16, 3, 0)]
Z = 2


def main(path):
    dev = "cuda:0"
    outs = {}
    for i, (C_, S, N, kv_half) in enumerate(CASES):
        g = torch.Generator().manual_seed(40 + i)
        Sc = S // 2 if kv_half else S
        q = torch.randn((N, C_, Z, S, S), generator=g)
        kv = torch.randn((N, 2 * C_, Z, Sc, Sc), generator=g)
        qw, kw = torch.rand(C_, generator=g) + 0.5, torch.rand(C_, generator=g) + 0.5
        qc, kvc = util.to_cb8(q.to(dev)), util.to_cb8(kv.to(dev))
        qwd, kwd = qw.to(dev), kw.to(dev)
        out = torch.full((N, C_ // 8, Z, S, S, 8), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().tm_op_window_attn_kv(_lib.ptr(qc), _lib.ptr(kvc), _lib.ptr(qwd), _lib.ptr(kwd), _lib.ptr(out), N, C_, Z, S,
                                                   0, kv_half, _lib.current_stream_ptr()), "tm_op_window_attn_kv")
        outs[f"case{i}"] = out.cpu().numpy().view(np.uint32)
    np.savez(path, **outs)


if __name__ == "__main__":
    main(sys.argv[1])
