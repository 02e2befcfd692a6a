"""No GPU, no library: the x-pair identity of tests/xpair_cases.py (pair form in z, Winograd F(2,3) along x) equals F.conv3d in
float64, is bit-equal to it on integer operands in float32, a float32 evaluation in the order of the retired conv3d_xpair stays
inside the derived bound, and every deliberate error is caught."""
import pytest
import torch

import xpair_cases as XC


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
