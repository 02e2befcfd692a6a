"""No GPU: the pair identity of the upsampled-input conv (tests/ups_pair_cases.py) evaluated in float32 on the CPU equals
F.conv3d on the upsampled input bit for bit on integers and stays inside the derived bound on random data; the hook refuses
what the kernel does not take before any device call."""
import ctypes as C

import pytest
import torch

import ups_pair_cases as UC
from teramind_amd import _lib


@pytest.mark.parametrize("case", UC.CASES, ids=UC.case_id)
def test_pair_identity_exact_on_integers(case):
    c = UC.make(case, "int")
    assert torch.equal(UC.pair_f32(c), UC.reference(c, torch.float32))


@pytest.mark.parametrize("case", UC.CASES, ids=UC.case_id)
def test_bound_holds_for_a_float32_evaluation(case):
    c = UC.make(case, "float")
    d = (UC.pair_f32(c).double() - UC.reference(c)).abs()
    bnd = UC.bound(c)
    print(f"{UC.case_id(case)}: max|d|={float(d.max()):.3e} worst |d|/bound={float((d / bnd).max()):.4f}")
    assert bool((d <= bnd).all())


def test_hook_refusals_need_no_device():
    L = _lib.lib()
    h = torch.zeros(64)
    p = C.c_void_p(h.data_ptr())
    assert L.tm_op_conv_ups_pair_f32(p, p, p, p, 1, 8, 64, 4, 8, 0, None) == -1     # Z != 2
    assert L.tm_op_conv_ups_pair_f32(p, p, p, p, 1, 8, 64, 1, 8, 0, None) == -1
    assert L.tm_op_conv_ups_pair_f32(p, p, p, p, 1, 8, 64, 2, 12, 0, None) == -1    # S not a tile size
    assert L.tm_op_conv_ups_pair_f32(p, p, p, p, 1, 8, 64, 2, 8, 3, None) == -1     # tile_variant
    assert L.tm_op_conv_ups_pair_f32(p, p, p, None, 1, 8, 64, 2, 8, 0, None) == -1
