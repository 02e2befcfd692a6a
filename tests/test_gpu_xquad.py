"""-m gpu: conv3d_xquad, the x-quad form of the fp32 3x3x3 pad-1 conv at Z = 2 (Winograd F(4,3) along x), through
tm_op_conv_xquad_f32, both tiles forced: bit-equal to float64 F.conv3d on the integer cases, inside the derived bound of
tests/xquad_cases.py on random data, identical bits from the two tiles.  The output lies between two NaN fences and is itself
prefilled with NaN: the fences must stay untouched and no NaN may be left inside; every launch is repeated and must reproduce
its bits."""
import ctypes as C

import pytest
import torch

import util
import xquad_cases as XQ
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 4096                                         # floats in front of and behind y
_REF = {}
_WORST = {}


def _case(case, kind):
    """inputs, reference and bound of a case, computed once and left unchanged"""
    key = (case, kind)
    if key not in _REF:
        c = XQ.make(case, kind)
        c["ref"] = XQ.reference(c)
        if kind == "float":
            c["bound"] = XQ.bound(c)
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
        tile = _lib.lib().tm_op_conv_xquad_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                               _lib.ptr(rc8), 1 if c["res_half"] else 0, N, Cin, Cout, 2, S, variant,
                                               _lib.current_stream_ptr())
        if tile < 0:
            _lib.check(tile, "tm_op_conv_xquad_f32")
        assert tile == variant, f"asked for tile {variant}, the hook reports {tile}"
        assert bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + n:]).all()), "a fence around y was written"
        assert not bool(torch.isnan(yc).any()), "the kernel left output elements unwritten"
        outs.append(yc.clone())
    assert torch.equal(outs[0], outs[1]), "two launches on the same input differ"
    return util.from_cb8(outs[0], Cout).cpu(), outs[0]


@pytest.mark.parametrize("case", XQ.CASES, ids=XQ.case_id)
def test_xquad_exact_integers(case):
    c = _case(case, "int")
    for variant in (1, 2):
        got, _ = _run(c, variant)
        assert torch.equal(got.double(), c["ref"]), util.report(f"xquad v{variant}", got.double(), c["ref"])


@pytest.mark.parametrize("case", XQ.CASES, ids=XQ.case_id)
def test_xquad_random_vs_float64(case):
    c = _case(case, "float")
    ref, bnd = c["ref"], c["bound"]
    raws = []
    for variant in (1, 2):
        got, raw = _run(c, variant)
        d = (got.double() - ref).abs()
        fam = "r%d" % case[4]
        _WORST[fam] = max(_WORST.get(fam, 0.0), XQ.worst(d, bnd))
        print(f"xquad random {XQ.case_id(case)} v{variant}: max|d|={float(d.max()):.3e} worst |d|/bound={XQ.worst(d, bnd):.4f} "
              f"(family {fam} so far {_WORST[fam]:.4f})")
        assert bool((d <= bnd).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={XQ.worst(d, bnd):.3g}"
        raws.append(raw)
    assert torch.equal(raws[0], raws[1]), "the two tiles differ in bits"


def test_xquad_tile_by_launch_size():
    """tile_variant 0: the hook reports the tile the launch-size rule chose (the small one below 256 workgroups of the large)"""
    c = _case(XQ.CASES[0], "int")
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    yc = torch.full((N, (Cout + 7) // 8, 2, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    tile = _lib.lib().tm_op_conv_xquad_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                           C.c_void_p(0), 0, N, Cin, Cout, 2, S, 0, _lib.current_stream_ptr())
    assert tile == 1
    assert torch.equal(util.from_cb8(yc, Cout).cpu().double(), c["ref"])


def test_xquad_refusals_leave_y_untouched():
    c = _case(XQ.CASES[0], "int")
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    yc = torch.full((N, (Cout + 7) // 8, 2, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    f = _lib.lib().tm_op_conv_xquad_f32
    args = (_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc), C.c_void_p(0), 0)
    st = _lib.current_stream_ptr()
    assert f(*args, N, Cin, Cout, 4, S, 0, st) == -1           # Z != 2
    assert f(*args, N, Cin, Cout, 2, 4, 0, st) == -1           # S = 4
    assert f(*args, N, Cin, Cout, 2, 10, 0, st) == -1          # S not a multiple of 4
    assert f(*args, N, Cin, Cout, 2, S, 3, st) == -1           # tile_variant
    assert f(*args[:5], 1, N, Cin, Cout, 2, S, 0, st) == -1    # res_half without a residual
    torch.cuda.synchronize()
    assert bool(torch.isnan(yc).all()), "a refused call wrote to y"
