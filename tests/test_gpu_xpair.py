"""-m gpu: conv3d_xpair, the x-pair form of the fp32 3x3x3 pad-1 conv at Z = 2, through tm_op_conv_xpair_f32, both tiles:
bit-equal to F.conv3d on integer operands, inside the derived bound of tests/xpair_cases.py on random data, identical bits
from the 64- and the 128-voxel tile.  The output lies between two NaN fences and is itself prefilled with NaN: the fences
must stay untouched and no NaN may be left inside; every launch is repeated and must reproduce its bits."""
import ctypes as C

import pytest
import torch

import util
import xpair_cases as XC
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 4096                                         # floats in front of and behind y
_REF = {}


def _case(case, kind):
    """inputs, reference(s) and bound of a case, computed once and left unchanged"""
    key = (case, kind)
    if key not in _REF:
        c = XC.make(case, kind)
        c["ref"] = XC.reference(c, torch.float32 if kind == "int" else torch.float64)
        if kind == "float":
            c["bound"] = XC.bound(c)
        _REF[key] = c
    return _REF[key]


def _run(c, variant):
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    rc8 = util.to_cb8(c["res"].to(DEV)) if c["res"] is not None else None
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    n = N * ((Cout + 7) // 8) * 2 * S * S * 8
    outs = []
    for _ in range(2):
        buf = torch.full((FENCE + n + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
        yc = buf[FENCE:FENCE + n].view(N, (Cout + 7) // 8, 2, S, S, 8)
        tile = _lib.lib().tm_op_conv_xpair_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                               _lib.ptr(rc8), 1 if c["res_half"] else 0, N, Cin, Cout, 2, S, variant,
                                               _lib.current_stream_ptr())
        if tile < 0:
            _lib.check(tile, "tm_op_conv_xpair_f32")
        assert tile == variant, f"asked for tile {variant}, the hook reports {tile}"
        assert bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + n:]).all()), "a fence around y was written"
        assert not bool(torch.isnan(yc).any()), "the kernel left output elements unwritten"
        outs.append(yc.clone())
    assert torch.equal(outs[0], outs[1]), "two launches on the same input differ"
    return util.from_cb8(outs[0], Cout).cpu(), outs[0]


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("case", XC.CASES, ids=XC.case_id)
def test_xpair_exact_integers(case, variant):
    c = _case(case, "int")
    got, _ = _run(c, variant)
    assert torch.equal(got, c["ref"]), util.report("xpair", got, c["ref"])


@pytest.mark.parametrize("case", XC.CASES, ids=XC.case_id)
def test_xpair_random_vs_float64(case):
    c = _case(case, "float")
    ref, bnd = c["ref"], c["bound"]
    raws = []
    for variant in (1, 2):
        got, raw = _run(c, variant)
        d = (got.double() - ref).abs()
        print(f"xpair random {XC.case_id(case)} v{variant}: max|d|={float(d.max()):.3e} worst |d|/bound={XC.worst(d, bnd):.4f}")
        assert bool((d <= bnd).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={XC.worst(d, bnd):.3g}"
        raws.append(raw)
    assert torch.equal(raws[0], raws[1]), "the 64- and 128-voxel tiles differ in bits"


def test_xpair_tile_by_launch_size():
    """tile_variant 0: the hook reports the tile the launch-size rule chose (64 voxels below 512 workgroups of 128)"""
    c = _case(XC.CASES[0], "int")
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    yc = torch.full((N, (Cout + 7) // 8, 2, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    tile = _lib.lib().tm_op_conv_xpair_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                           C.c_void_p(0), 0, N, Cin, Cout, 2, S, 0, _lib.current_stream_ptr())
    assert tile == 1
    assert torch.equal(util.from_cb8(yc, Cout).cpu(), c["ref"])


def test_xpair_refusals_leave_y_untouched():
    c = _case(XC.CASES[0], "int")
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    yc = torch.full((N, (Cout + 7) // 8, 2, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    f = _lib.lib().tm_op_conv_xpair_f32
    args = (_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc), C.c_void_p(0), 0)
    st = _lib.current_stream_ptr()
    assert f(*args, N, Cin, Cout, 4, S, 0, st) == -1           # Z != 2
    assert f(*args, N, Cin, Cout, 2, 4, 0, st) == -1           # S outside the set
    assert f(*args, N, Cin, Cout, 2, S, 3, st) == -1           # tile_variant
    assert f(*args[:5], 1, N, Cin, Cout, 2, S, 0, st) == -1    # res_half without a residual
    torch.cuda.synchronize()
    assert bool(torch.isnan(yc).all()), "a refused call wrote to y"
