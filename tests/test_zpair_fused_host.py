"""No GPU: the error bound of the fused mid-section (tests/zpair_fused_cases.py) is held by a float32 evaluation of the same
operation on the CPU, the two wrong variants the GPU tests are meant to catch leave it, and the hook's argument checks answer
before any device call."""
import ctypes as C

import pytest
import torch

import zpair_fused_cases as ZC
from teramind_amd import _lib


@pytest.mark.parametrize("case", ZC.CASES, ids=ZC.case_id)
@pytest.mark.parametrize("kind", ["float", "int"])
def test_bound_holds_for_a_float32_evaluation(case, kind):
    c = ZC.make(case, kind)
    ref = ZC.reference(c)
    bnd = ZC.bound(c)
    d = (ZC.emulate_f32(c).double() - ref).abs()
    print(f"{ZC.case_id(case)} {kind}: max|d|={float(d.max()):.3e} worst |d|/bound={ZC.worst(d, bnd):.4f}")
    assert bool((d <= bnd).all())


# the neighbour image's modulation row can only be taken where a launch has more than one image
WRONG = [(c, "drop_lane_group") for c in ZC.CASES] + [(c, "wrong_image_row") for c in ZC.CASES if -(-c[2] // c[3]) > 1]


@pytest.mark.parametrize("case,wrong", WRONG, ids=lambda v: v if isinstance(v, str) else ZC.case_id(v))
def test_bound_rejects_the_wrong_variants(case, wrong):
    """Half the sum of squares missing, or the neighbour image's modulation row: both leave the bound."""
    c = ZC.make(case, "float")
    d = (ZC.reference(c, wrong) - ZC.reference(c)).abs()
    assert not bool((d <= ZC.bound(c)).all())


def test_hook_refusals_need_no_device():
    """TM_ERR_ARG (-1) for every form the fused kernel does not take; no pointer is touched (all of them are dummies)."""
    L = _lib.lib()
    h = torch.zeros(64)
    p = C.c_void_p(h.data_ptr())

    def call(N=1, Cin=8, Cout=64, Z=2, S=16, per_image=1, variant=2, res=None, a2_sep=None, h1=None):
        return L.tm_op_conv_zpair_fused_f32(p, p, p, p, p, p, res, p, h1, a2_sep, N, Cin, Cout, Z, S, per_image, variant, None)

    assert call(Cout=128) == -1 and call(Cout=32) == -1          # Cout != 64
    assert call(res=p) == -1                                     # a residual
    assert call(variant=1) == -1                                 # the 64-voxel (HALF) tile, forced
    assert call(variant=0) == -1                                 # ... and chosen by the launch size (512 voxels)
    assert call(S=4) == -1                                       # S = 4 has the 64-voxel tile only
    assert call(Z=1) == -1 and call(Z=4) == -1                   # Z != 2
    assert call(per_image=0) == -1 and call(variant=3) == -1
    assert call(a2_sep=p) == -1                                  # the separate pass needs h1
