"""-m gpu: conv3d_zpair_ups, the pair form of the fp32 upsampled-input conv, through tm_op_conv_ups_pair_f32: bit-equal to
F.conv3d on the nearest-upsampled input with integer operands, inside the derived bound of tests/ups_pair_cases.py on random
data, identical bits from both tiles.  Outputs are prefilled with NaN; every launch is repeated and must reproduce its bits."""
import ctypes as C

import pytest
import torch

import util
import ups_pair_cases as UC
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(c, variant):
    Cin, Cout, S, N = c["case"]
    xc = util.to_cb8(c["x"].to(DEV))
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    outs = []
    for _ in range(2):
        yc = torch.full((N, (Cout + 7) // 8, 2, 2 * S, 2 * S, 8), float("nan"), dtype=torch.float32, device=DEV)
        rc = _lib.lib().tm_op_conv_ups_pair_f32(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                                N, Cin, Cout, 2, S, variant, _lib.current_stream_ptr())
        _lib.check(rc, "tm_op_conv_ups_pair_f32")
        outs.append(yc)
    assert not bool(torch.isnan(outs[0]).any()), "the kernel left output elements unwritten"
    assert torch.equal(outs[0], outs[1]), "two launches on the same input differ"
    return util.from_cb8(outs[0], Cout).cpu(), outs[0]


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("case", UC.CASES, ids=UC.case_id)
def test_ups_pair_exact_integers(case, variant):
    c = UC.make(case, "int")
    got, _ = _run(c, variant)
    ref = UC.reference(c, torch.float32)
    assert torch.equal(got, ref), util.report("ups pair", got, ref)


@pytest.mark.parametrize("case", UC.CASES, ids=UC.case_id)
def test_ups_pair_random_vs_float64(case):
    c = UC.make(case, "float")
    ref, bnd = UC.reference(c), UC.bound(c)
    raws = []
    for variant in (1, 2):
        got, raw = _run(c, variant)
        d = (got.double() - ref).abs()
        print(f"ups pair random {UC.case_id(case)} v{variant}: max|d|={float(d.max()):.3e} worst |d|/bound={float((d / bnd).max()):.4f}")
        assert bool((d <= bnd).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={float((d / bnd).max()):.3g}"
        raws.append(raw)
    assert torch.equal(raws[0], raws[1]), "the 64- and 128-voxel tiles differ in bits"
