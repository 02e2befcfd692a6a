"""-m gpu: the tail of conv3d_xquad (bias and residual quads requested ahead of the q-half exchange, outputs formed in the
residual's registers, sixteen stores that wait for nothing) through tm_op_conv_xquad_sched_f32 with both tiles and both schedules
forced, in the three residual modes: none, the output's geometry, half resolution (res_half).  The tail changes no pack, no order
of sums and no rounding, so: integer data is torch.equal to float64 F.conv3d plus the residual; random data stays inside the
bound tests/xquad_cases.py derives; the four (tile, schedule) combinations agree in every bit; three launches agree in every bit.
x, the residual and y each lie between two NaN fences, and y is prefilled with NaN: the fences around y must stay untouched, y
must come out finite -- a lane without a voxel or a cout block that used what it read past x or past the residual (instead of
element 0 of the tensor, or a zero) would leave a NaN there.  Cases: every case of tests/xquad_cases.py, plus (Cin 8, Cout 37,
S 16, N 3: a cout block that is not full and a patch group that is not full) and (Cin 16, Cout 32, S 8, N 1), each in the three
residual modes."""
import ctypes as C

import pytest
import torch

import util
import xquad_cases as XQ
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 4096                                         # floats in front of and behind x, the residual and y
CASES = XQ.CASES + [s + (r,) for s in ((8, 37, 16, 3), (16, 32, 8, 1)) for r in (0, 1, 2)]
COMBOS = [(tile, sched) for tile in (1, 2) for sched in (0, 1)]
_REF = {}


def _fenced(t):
    """a copy of the CB8 tensor t between two NaN fences"""
    buf = torch.full((FENCE + t.numel() + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
    v = buf[FENCE:FENCE + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _case(case, kind):
    """inputs (on the device, fenced), reference and bound of a case, computed once and left unchanged"""
    key = (case, kind)
    if key not in _REF:
        c = XQ.make(case, kind)
        c["ref"] = XQ.reference(c)
        if kind == "float":
            c["bound"] = XQ.bound(c)
        c["xc"] = _fenced(util.to_cb8(c["x"].to(DEV)))
        c["rc"] = _fenced(util.to_cb8(c["res"].to(DEV))) if c["res"] is not None else None
        c["wh"], c["bh"] = c["w"].contiguous().float(), c["b"].contiguous().float()
        _REF[key] = c
    return _REF[key]


def _launch(c, tile, sched):
    Cin, Cout, S, N = c["case"][:4]
    n = N * ((Cout + 7) // 8) * 2 * S * S * 8
    buf = torch.full((FENCE + n + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
    yc = buf[FENCE:FENCE + n].view(N, (Cout + 7) // 8, 2, S, S, 8)
    got = _lib.lib().tm_op_conv_xquad_sched_f32(_lib.ptr(c["xc"]), C.c_void_p(c["wh"].data_ptr()), C.c_void_p(c["bh"].data_ptr()),
                                                _lib.ptr(yc), _lib.ptr(c["rc"]), 1 if c["res_half"] else 0, N, Cin, Cout, 2, S, tile,
                                                sched, _lib.current_stream_ptr())
    if got < 0:
        _lib.check(got, "tm_op_conv_xquad_sched_f32")
    assert got == tile, f"asked for tile {tile}, the hook reports {got}"
    assert bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + n:]).all()), "a fence around y was written"
    assert bool(torch.isfinite(yc).all()), "y is not finite: an element was left unwritten, or a lane used what it must not read"
    return yc


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("case", CASES, ids=XQ.case_id)
def test_tail(case, kind):
    c = _case(case, kind)
    Cout = c["case"][1]
    ys = {}
    for tile, sched in COMBOS:
        y = _launch(c, tile, sched)
        if kind == "int":                            # three launches of every combination on the exact data
            for _ in range(2):
                assert torch.equal(_launch(c, tile, sched), y), f"tile {tile} schedule {sched}: launches differ"
        ys[(tile, sched)] = y
    first = ys[COMBOS[0]]
    for k in COMBOS[1:]:
        assert torch.equal(ys[k], first), util.report(f"tile {k[0]} schedule {k[1]} against tile 1 schedule 0",
                                                      util.from_cb8(ys[k], Cout).cpu().double(),
                                                      util.from_cb8(first, Cout).cpu().double())
    got = util.from_cb8(first, Cout).cpu().double()
    if kind == "int":
        assert torch.equal(got, c["ref"]), util.report("against float64", got, c["ref"])
    else:
        d = (got - c["ref"]).abs()
        print(f"xquad tail random {XQ.case_id(case)}: max|d|={float(d.max()):.3e} worst |d|/bound={XQ.worst(d, c['bound']):.4f}")
        assert bool((d <= c["bound"]).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={XQ.worst(d, c['bound']):.3g}"
