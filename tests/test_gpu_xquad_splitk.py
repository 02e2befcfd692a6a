"""-m gpu: split K of conv3d_xquad (ksplit workgroups per tile over disjoint ranges of the cin blocks, then xquad_split_reduce)
through tm_op_conv_xquad_split_f32 at Z = 2, operands as in tests/xquad_cases.py.  Shapes (Cin, Cout, S, N): (40, 37, 8, 3) five
cin blocks, so uneven ranges at both factors, a partial second cout tile and a missing patch; (37, 64, 16, 1) pad channels in
the last block of the last range; (64, 32, 8, 1) even ranges and one tile.  Every shape at ksplit 1 / 2 / 4, both tiles forced,
both schedules, without a residual, with one, and with the residual in y itself (res == y).

Integer data: torch.equal float64 F.conv3d (+ residual) at every factor.  Random data: inside xquad_cases.bound with ksplit - 1
added to its constant c, one rounding per add of the reduction: the chain of a partial is shorter than the unsplit chain L, so L
stays an upper bound and no measured tolerance enters.  ksplit 1 must equal tm_op_conv_xquad_sched_f32 bit for bit, three
launches of a factor must agree in every bit (no atomics: one order of the sum), the NaN fences around y must stay NaN and y
must come out finite although x and the residual lie between NaN fences of their own.

Sensitivity: a scratch build whose reduction skips the last partial fails every ksplit > 1 case of test_split_against_float64
and passes the ksplit 1 cases (profiles/fp32_xquad_splitk.txt has the count)."""
import ctypes as C

import pytest
import torch

import util
import xquad_cases as XQ
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 4096                                         # floats in front of and behind a tensor
SHAPES = [(40, 37, 8, 3), (37, 64, 16, 1), (64, 32, 8, 1)]
RES = ["none", "full", "inplace"]
COMBOS = [(variant, sched) for variant in (1, 2) for sched in (0, 1)]
_REF = {}


def _case(shape, res, kind):
    """inputs, float64 reference and the magnitude of the bound of a case, computed once and left unchanged"""
    key = (shape, res != "none", kind)
    if key not in _REF:
        c = XQ.make(shape + (0 if res == "none" else 1,), kind)
        c["ref"] = XQ.reference(c)
        if kind == "float":
            c["mag"] = XQ.magnitude(c)
        _REF[key] = c
    return _REF[key]


def _fenced(t):
    """t (a CB8 device tensor) between two NaN fences: the buffer and the view of t inside it"""
    n = t.numel()
    buf = torch.full((FENCE + n + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
    buf[FENCE:FENCE + n] = t.reshape(-1)
    return buf, buf[FENCE:FENCE + n].view(t.shape)


def _launch(c, res, variant, sched, ksplit, hook="split"):
    Cin, Cout, S, N = c["case"][:4]
    xbuf, xc = _fenced(util.to_cb8(c["x"].to(DEV)))
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    shape = (N, (Cout + 7) // 8, 2, S, S, 8)
    if res == "inplace":                             # y holds the residual and is updated in place
        ybuf, yc = _fenced(util.to_cb8(c["res"].to(DEV)))
        rc8 = yc
    else:
        ybuf, yc = _fenced(torch.full(shape, float("nan"), dtype=torch.float32, device=DEV))
        rc8 = _fenced(util.to_cb8(c["res"].to(DEV)))[1] if res == "full" else None
    args = (_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc), _lib.ptr(rc8), 0, N, Cin, Cout, 2, S,
            variant, sched)
    if hook == "split":
        got = _lib.lib().tm_op_conv_xquad_split_f32(*args, ksplit, _lib.current_stream_ptr())
        want = ksplit
    else:
        got = _lib.lib().tm_op_conv_xquad_sched_f32(*args, _lib.current_stream_ptr())
        want = variant
    if got < 0:
        _lib.check(got, "tm_op_conv_xquad_%s_f32" % hook)
    assert got == want, f"the hook reports {got}, expected {want}"
    n = yc.numel()
    assert bool(torch.isnan(ybuf[:FENCE]).all()) and bool(torch.isnan(ybuf[FENCE + n:]).all()), "a fence around y was written"
    assert bool(torch.isfinite(yc).all()), "y holds elements that are not finite (unwritten, or read from a fence)"
    assert bool(torch.isnan(xbuf[:FENCE]).all()) and bool(torch.isnan(xbuf[FENCE + xc.numel():]).all()), "a fence around x was written"
    return yc


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("ksplit", [1, 2, 4])
@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "Cin%d-Cout%d-S%d-N%d" % s)
def test_split_against_float64(shape, res, ksplit, kind):
    c = _case(shape, res, kind)
    Cin, Cout = shape[:2]
    L = (Cin + 7) // 8 * 8 * 3
    for variant, sched in COMBOS:
        what = f"ksplit {ksplit} tile {variant} schedule {sched}"
        ys = [_launch(c, res, variant, sched, ksplit) for _ in range(3)]
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]), f"{what}: three launches differ"
        got = util.from_cb8(ys[0], Cout).cpu().double()
        if kind == "int":
            assert torch.equal(got, c["ref"]), util.report(what + " against float64", got, c["ref"])
        else:
            bnd = XQ.SECOND * (L + 15 + (0 if res == "none" else 1) + ksplit - 1) * XQ.U * c["mag"]
            worst = XQ.worst((got - c["ref"]).abs(), bnd)
            print(f"{what}: worst error / bound = {worst:.3f}")
            assert worst <= 1.0, util.report(what + f" against float64, error / bound {worst:.3f}", got, c["ref"])


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "Cin%d-Cout%d-S%d-N%d" % s)
def test_ksplit_1_is_the_unsplit_launch(shape, res):
    c = _case(shape, res, "float")
    for variant, sched in COMBOS:
        y1 = _launch(c, res, variant, sched, 1)
        y0 = _launch(c, res, variant, sched, 1, hook="sched")
        assert torch.equal(y1, y0), f"tile {variant} schedule {sched}: ksplit 1 differs from tm_op_conv_xquad_sched_f32"


def test_the_rule_through_the_hook():
    """ksplit 0 takes tm_conv_xquad_ksplit's factor and computes the same bits as that factor forced"""
    shape = (64, 32, 8, 1)
    c = _case(shape, "full", "int")
    Cin, Cout, S, N = shape
    k = _lib.lib().tm_conv_xquad_ksplit(N, Cin, Cout, S, 0)
    assert k in (1, 2, 4)
    xc = util.to_cb8(c["x"].to(DEV))
    rc8 = util.to_cb8(c["res"].to(DEV))
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    yc = torch.full((N, (Cout + 7) // 8, 2, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    got = _lib.lib().tm_op_conv_xquad_split_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                                _lib.ptr(rc8), 0, N, Cin, Cout, 2, S, 0, 0, 0, _lib.current_stream_ptr())
    assert got == k, f"the hook took {got}, the rule says {k}"
    assert torch.equal(util.from_cb8(yc, Cout).cpu().double(), c["ref"])
