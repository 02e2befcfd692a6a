"""No GPU: the x-pair identity of tests/xpair_cases.py (pair form in z, Winograd F(2,3) along x) equals F.conv3d in float64,
is bit-equal to it on integer operands in float32, a float32 evaluation in the kernel's order stays inside the derived bound,
every deliberate error is caught, and the hook refuses what the kernel does not take before any device call."""
import ctypes as C

import pytest
import torch

import xpair_cases as XC
from teramind_amd import _lib


@pytest.mark.parametrize("case", XC.CASES, ids=XC.case_id)
def test_float64_model_equals_conv3d(case):
    c = XC.make(case, "float")
    ref = XC.reference(c)
    d = (XC.model(c) - ref).abs()
    # float64 roundings of the same expression: the bound's own count with 2^-53 in place of 2^-24
    lim = XC.bound(c) * (2.0 ** -53 / XC.U)
    print(f"{XC.case_id(case)}: max|d|={float(d.max()):.3e}")
    assert bool((d <= lim).all())


@pytest.mark.parametrize("case", XC.CASES, ids=XC.case_id)
def test_integer_operands_are_bit_equal(case):
    c = XC.make(case, "int")
    assert torch.equal(XC.model(c, torch.float32), XC.reference(c, torch.float32))


@pytest.mark.parametrize("case", XC.HOST_CASES, ids=XC.case_id)
def test_float32_in_kernel_order_stays_inside_the_bound(case):
    c = XC.make(case, "float")
    d = (XC.kernel_order_f32(c).double() - XC.reference(c)).abs()
    bnd = XC.bound(c)
    print(f"{XC.case_id(case)}: max|d|={float(d.max()):.3e} worst |d|/bound={XC.worst(d, bnd):.4f}")
    assert bool((d <= bnd).all())
    ci = XC.make(case, "int")
    assert torch.equal(XC.kernel_order_f32(ci), XC.reference(ci, torch.float32))


@pytest.mark.parametrize("wrong", XC.WRONG)
@pytest.mark.parametrize("case", XC.HOST_CASES, ids=XC.case_id)
def test_deliberate_errors_are_caught(case, wrong):
    c = XC.make(case, "float")
    d = (XC.model(c, torch.float64, wrong) - XC.reference(c)).abs()
    leaves = not bool((d <= XC.bound(c)).all())
    ci = XC.make(case, "int")
    breaks = not torch.equal(XC.model(ci, torch.float32, wrong), XC.reference(ci, torch.float32))
    print(f"{XC.case_id(case)} {wrong}: leaves the bound {leaves}, breaks integer equality {breaks}")
    assert leaves and breaks


def test_pack_rule_and_hook_refusals_need_no_device():
    L = _lib.lib()
    h = torch.zeros(64)
    p = C.c_void_p(h.data_ptr())
    n = C.c_void_p(0)
    f = L.tm_op_conv_xpair_f32
    assert f(p, p, p, p, n, 0, 1, 8, 64, 4, 8, 0, None) == -1      # Z != 2
    assert f(p, p, p, p, n, 0, 1, 8, 64, 1, 8, 0, None) == -1
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 4, 0, None) == -1      # S = 4 stays on the pair form
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 12, 0, None) == -1     # S not a tile size
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 8, 3, None) == -1      # tile_variant
    assert f(p, p, p, p, n, 1, 1, 8, 64, 2, 8, 0, None) == -1      # res_half without a residual
    assert f(p, p, p, n, n, 0, 1, 8, 64, 2, 8, 0, None) == -1      # no output
    assert f(p, p, p, p, n, 0, 0, 8, 64, 2, 8, 0, None) == -1      # N < 1
    assert L.tm_last_error()
