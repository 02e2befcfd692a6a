"""-m gpu: the pipelined schedule of conv3d_xquad (a ring of two sets of six q-planes staged under the products, three barriers
per cin block) through tm_op_conv_xquad_sched_f32, both tiles forced.  The schedule changes neither the pack nor the order of
sums inside an accumulator, so the claim is equal bits and no tolerance enters: schedule 1 torch.equal schedule 0 on integer
and on random data, integer data torch.equal float64 F.conv3d.  The output lies between two NaN fences and is itself prefilled
with NaN: the fences must stay untouched and no NaN may be left inside.  Three launches of schedule 1 on the same input must
agree in every bit: a stale weight slot or a stale plane of the ring shows as a difference there.  Cases: those of
tests/xquad_cases.py (Cin 37: five cin blocks, an odd product count in both rings), one cin block (the prologue meets the
last-block body directly) and two blocks with one exact cout tile."""
import ctypes as C

import pytest
import torch

import util
import xquad_cases as XQ
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 4096                                         # floats in front of and behind y
CASES = XQ.CASES + [(8, 37, 16, 3, 0), (16, 32, 8, 1, 0)]
_REF = {}


def _case(case, kind):
    """inputs and reference of a case, computed once and left unchanged"""
    key = (case, kind)
    if key not in _REF:
        c = XQ.make(case, kind)
        if kind == "int":
            c["ref"] = XQ.reference(c)
        _REF[key] = c
    return _REF[key]


def _launch(c, variant, sched):
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    rc8 = util.to_cb8(c["res"].to(DEV)) if c["res"] is not None else None
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    n = N * ((Cout + 7) // 8) * 2 * S * S * 8
    buf = torch.full((FENCE + n + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
    yc = buf[FENCE:FENCE + n].view(N, (Cout + 7) // 8, 2, S, S, 8)
    tile = _lib.lib().tm_op_conv_xquad_sched_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                                 _lib.ptr(rc8), 1 if c["res_half"] else 0, N, Cin, Cout, 2, S, variant, sched,
                                                 _lib.current_stream_ptr())
    if tile < 0:
        _lib.check(tile, "tm_op_conv_xquad_sched_f32")
    assert tile == variant, f"asked for tile {variant}, the hook reports {tile}"
    assert bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + n:]).all()), "a fence around y was written"
    assert not bool(torch.isnan(yc).any()), "the kernel left output elements unwritten"
    return yc


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("case", CASES, ids=XQ.case_id)
def test_pipelined_schedule_equals_the_four_barrier_one(case, kind):
    c = _case(case, kind)
    Cout = c["case"][1]
    for variant in (1, 2):
        y0 = _launch(c, variant, 0)
        y1 = [_launch(c, variant, 1) for _ in range(3)]
        assert torch.equal(y1[0], y1[1]) and torch.equal(y1[0], y1[2]), f"tile {variant}: launches of schedule 1 differ"
        assert torch.equal(y1[0], y0), util.report(f"tile {variant}: schedule 1 against 0", util.from_cb8(y1[0], Cout).cpu().double(),
                                                   util.from_cb8(y0, Cout).cpu().double())
        if kind == "int":
            got = util.from_cb8(y1[0], Cout).cpu().double()
            assert torch.equal(got, c["ref"]), util.report(f"tile {variant}: schedule 1 against float64", got, c["ref"])


def test_refusals_leave_y_untouched():
    c = _case(XQ.CASES[0], "int")
    Cin, Cout, S, N = c["case"][:4]
    xc = util.to_cb8(c["x"].to(DEV))
    yc = torch.full((N, (Cout + 7) // 8, 2, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    f = _lib.lib().tm_op_conv_xquad_sched_f32
    args = (_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc), C.c_void_p(0), 0)
    st = _lib.current_stream_ptr()
    assert f(*args, N, Cin, Cout, 2, S, 0, 2, st) == -1        # sched
    assert f(*args, N, Cin, Cout, 2, S, 0, -1, st) == -1
    assert f(*args, N, Cin, Cout, 4, S, 0, 1, st) == -1        # Z != 2
    assert f(*args, N, Cin, Cout, 2, 4, 0, 1, st) == -1        # S = 4
    assert f(*args, N, Cin, Cout, 2, S, 3, 1, st) == -1        # tile_variant
    torch.cuda.synchronize()
    assert bool(torch.isnan(yc).all()), "a refused call wrote to y"
