"""-m gpu: weight staging of the fp32 pair-form conv (conv3d_zpair) at real layer shapes with ragged edges.

The kernel brings the packed weights of a cin block into LDS by LDS-DMA, as a ring of three 9-tap slots that is refilled
product by product while the other products are being multiplied (one slot is rewritten once every wave has left it, and read
again only behind the wait and the barrier that retire its pieces).  A slot read too early, or refilled too early, shows up as
wrong sums in SOME cin blocks of SOME workgroups, so the cases are long K loops (Cin = 485, 741, 1253: 61, 93 and 157 cin
blocks, the last one padded to 8), launches whose last workgroup is partly empty (N = 1, 3, 5 against 2 and 4 patches per
workgroup), every tile width (S = 4 .. 64), the residual epilogues and the x2-upsample store.  Both tile variants must give
identical bits, and each must lie within the bound of test_gpu_conv_zpair._bound around float64 F.conv3d.  Outputs are
prefilled with NaN and every launch runs twice and must reproduce its bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import util
from teramind_amd import _lib
from test_gpu_conv_zpair import _bound, _residual, _up2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _launch(xc, w, b, N, Cin, Cout, S, variant, res=None, res_half=False, up2=False):
    """xc: CB8 input holding AT LEAST N patches.  Returns the raw CB8 output of two identical launches."""
    wh, bh = w.contiguous().float(), b.contiguous().float()
    So = 2 * S if up2 else S
    L = _lib.lib()
    outs = []
    for _ in range(2):
        yc = torch.full((N, (Cout + 7) // 8, 2, So, So, 8), float("nan"), dtype=torch.float32, device=DEV)
        rcb = None if res is None else util.to_cb8(res)
        rc = L.tm_op_conv_mfma_res(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                   None if rcb is None else _lib.ptr(rcb), int(res_half), N, Cin, Cout, 2, S, 3, 0, int(up2),
                                   variant, _lib.current_stream_ptr())
        _lib.check(rc, "tm_op_conv_mfma_res")
        outs.append(yc)
    assert not bool(torch.isnan(outs[0]).any()), "the kernel left output elements unwritten (or read a NaN)"
    assert torch.equal(outs[0], outs[1]), "two launches on the same input differ"
    return outs[0]


def _operands(N, Cin, Cout, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, Cin, 2, S, S), generator=g)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5
    b = torch.randn((Cout,), generator=g)
    return x, w, b


# (N, Cin, Cout, S, res_mode, up2)   res_mode as in test_gpu_conv_zpair._residual: 0 none, 1 full resolution, 2 half resolution
CASES = [(3, 485, 128, 8, 1, 0), (5, 741, 64, 8, 0, 1), (1, 1253, 72, 8, 2, 0), (3, 1253, 64, 4, 0, 0), (5, 485, 64, 4, 1, 0),
         (1, 741, 64, 16, 0, 1), (3, 485, 64, 16, 2, 0), (3, 96, 64, 32, 1, 0), (1, 224, 64, 64, 2, 0), (1, 64, 64, 64, 0, 1)]


@pytest.mark.parametrize("N,Cin,Cout,S,res_mode,up2", CASES)
def test_zpair_stage_layer_shapes(N, Cin, Cout, S, res_mode, up2):
    x, w, b = _operands(N, Cin, Cout, S, 31)
    res, res_full = _residual(res_mode, N, Cout, S, 32, False)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    bound = _bound(x, w, b, res_full)
    if res is not None:
        ref = ref + res_full.double()
    if up2:
        ref, bound = _up2(ref), _up2(bound)
    xc = util.to_cb8(x.to(DEV))
    raws = []
    for variant in (1, 2):
        raw = _launch(xc, w, b, N, Cin, Cout, S, variant, None if res is None else res.to(DEV), res_mode == 2, bool(up2))
        d = (util.from_cb8(raw, Cout).double().cpu() - ref).abs()
        print(f"zpair stage N{N} Cin{Cin} Cout{Cout} S{S} res{res_mode} up2={up2} v{variant}: max|d|={float(d.max()):.3e} "
              f"worst |d|/bound={float((d / bound).max()):.4f}")
        assert bool((d <= bound).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={float((d / bound).max()):.3g}"
        raws.append(raw)
    assert torch.equal(raws[0], raws[1]), "the 64- and 128-voxel tiles differ in bits"


@pytest.mark.parametrize("N,S", [(3, 8), (5, 4), (1, 16)])
def test_zpair_stage_nan_beyond_last_patch(N, S):
    """Patches beyond N in the input buffer hold NaN: the slots of a partly empty workgroup must contribute zeros, so the
    outputs are finite and the same bits as with a clean buffer."""
    Cin, Cout = 485, 64
    x, w, b = _operands(N, Cin, Cout, S, 41)
    tail = torch.full((4, Cin, 2, S, S), float("nan"))
    clean = util.to_cb8(x.to(DEV))
    dirty = util.to_cb8(torch.cat([x, tail]).to(DEV))
    for variant in (1, 2):
        a = _launch(clean, w, b, N, Cin, Cout, S, variant)
        d = _launch(dirty, w, b, N, Cin, Cout, S, variant)
        assert bool(torch.isfinite(d).all())
        assert torch.equal(a, d), "NaN beyond the last patch reached the outputs"
