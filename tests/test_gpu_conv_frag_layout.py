"""-m gpu: the two fp32 z-pair LDS-DMA conv kernels on their k-half operand images (tm_conv_frag.h) -- conv3d_zpair (plain and
with the fused mid-section) and conv3d_zpair_ups through their single-op hooks (conv3d_xquad, the third kernel on these images,
has tests/test_gpu_xquad*.py), at the smallest shapes that reach every lane -> address map: S = 8, 16, 32 (one per tile width),
N = 1 and 3 (3 leaves a partial workgroup at S = 8), Cin 5 and 37 (one block and five, pad channels in the last), Cout 37 and
128 (pad slots, two cout tiles), both tiles.  Integer operands: bit-equal to float64 F.conv3d.  Random operands: inside the bounds of the kernels' own case modules
(imported, not restated).  Both tiles give identical bits.  Every output lies between NaN fences that must stay NaN, is prefilled
with NaN and must come back without one.  A wrong weight image, activation image, staging store or lane map changes which
operands meet in the MFMA: the integer cases then differ from F.conv3d."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_zpair as ZT
import ups_pair_cases as UC
import util
import xpair_cases as XC
import zpair_fused_cases as ZC
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE = 4096
# (S, N, Cin, Cout)
CASES = [(S, N, Cin, Cout) for S in (8, 16, 32) for N in (1, 3) for Cin, Cout in ((5, 37), (37, 128))]
FUSED = [(Cin, S, N, 1) for S in (8, 16, 32) for N in (1, 3) for Cin in (5, 37)]
_DATA = {}


def _id(c):
    return "S%d-N%d-Cin%d-Cout%d" % c


def _data(case, kind):
    """x, w, b and the float64 references of a case, made once and left unchanged"""
    if (case, kind) not in _DATA:
        S, N, Cin, Cout = case
        c = XC.make((Cin, Cout, S, N, 1, 0), kind)               # integers in [-8, 8] x [-4, 4] or normal data, bias, no residual
        c["ref"] = F.conv3d(c["x"].double(), c["w"].double(), c["b"].double(), padding=1)
        c["ref_ups"] = F.conv3d(UC.up2(c["x"]).double(), c["w"].double(), c["b"].double(), padding=1)
        _DATA[(case, kind)] = c
    return _DATA[(case, kind)]


def _launch(kernel, c, variant):
    """One launch between fences; returns (NCDHW on the CPU, raw CB8)."""
    S, N, Cin, Cout = c["x"].shape[-1], c["x"].shape[0], c["x"].shape[1], c["w"].shape[0]
    So = 2 * S if kernel == "ups" else S
    xc = util.to_cb8(c["x"].to(DEV))
    wh, bh = c["w"].contiguous().float(), c["b"].contiguous().float()
    n = N * ((Cout + 7) // 8) * 2 * So * So * 8
    buf = torch.full((FENCE + n + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
    yc = buf[FENCE:FENCE + n].view(N, (Cout + 7) // 8, 2, So, So, 8)
    L, st = _lib.lib(), _lib.current_stream_ptr()
    args = (_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc))
    if kernel == "zpair":
        _lib.check(L.tm_op_conv_mfma(*args, N, Cin, Cout, 2, S, 3, 0, 0, variant, st), "tm_op_conv_mfma")
    else:
        _lib.check(L.tm_op_conv_ups_pair_f32(*args, N, Cin, Cout, 2, S, variant, st), "tm_op_conv_ups_pair_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + n:]).all()), "a fence around y was written"
    assert not bool(torch.isnan(yc).any()), "the kernel left output elements unwritten"
    if Cout % 8:
        assert float(yc[:, -1, ..., Cout % 8:].abs().max()) == 0.0, "pad slots of the last cout block"
    return util.from_cb8(yc, Cout).cpu(), yc.clone()


@pytest.mark.parametrize("kernel", ["zpair", "ups"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_integers_equal_float64_conv3d(case, kernel):
    c = _data(case, "int")
    ref = c["ref_ups"] if kernel == "ups" else c["ref"]
    raws = []
    for variant in (1, 2):
        got, raw = _launch(kernel, c, variant)
        assert torch.equal(got.double(), ref), f"tile {variant}: " + util.report(kernel, got, ref.float())
        raws.append(raw)
    assert torch.equal(raws[0], raws[1]), "the two tiles differ in bits"


@pytest.mark.parametrize("kernel", ["zpair", "ups"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_random_inside_the_case_modules_bounds(case, kernel):
    c = _data(case, "float")
    if kernel == "zpair":
        ref, bnd = c["ref"], ZT._bound(c["x"], c["w"], c["b"], None)
    else:
        ref, bnd = c["ref_ups"], UC.bound(c)
    raws = []
    for variant in (1, 2):
        got, raw = _launch(kernel, c, variant)
        d = (got.double() - ref).abs()
        print(f"{kernel} {_id(case)} v{variant}: max|d|={float(d.max()):.3e} worst |d|/bound={float((d / bnd).max()):.4f}")
        assert bool((d <= bnd).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={float((d / bnd).max()):.3g}"
        raws.append(raw)
    assert torch.equal(raws[0], raws[1]), "the two tiles differ in bits"


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("case", FUSED, ids=ZC.case_id)
def test_fused_mid_section(case, kind):
    """conv3d_zpair<0, TW, true>: inside the case module's bound, equal in bits to the plain launch + separate norm pass, and the
    plain launch of the same call exact on integers"""
    Cin, S, N, per_image = case
    c = ZC.make(case, kind)
    xc = util.to_cb8(c["x"].to(DEV))
    hs = [c[k].contiguous().float() for k in ("w", "b", "nw", "sc", "sh")]
    n = N * 8 * 2 * S * S * 8
    buf = torch.full((FENCE + n + FENCE,), float("nan"), dtype=torch.float32, device=DEV)
    a2 = buf[FENCE:FENCE + n]
    h1 = torch.full((N, 8, 2, S, S, 8), float("nan"), device=DEV)
    sep = torch.full((N, 8, 2, S, S, 8), float("nan"), device=DEV)
    rc = _lib.lib().tm_op_conv_zpair_fused_f32(_lib.ptr(xc), *[C.c_void_p(t.data_ptr()) for t in hs], None, _lib.ptr(a2), _lib.ptr(h1),
                                               _lib.ptr(sep), N, Cin, ZC.COUT, 2, S, per_image, 2, _lib.current_stream_ptr())
    _lib.check(rc, "tm_op_conv_zpair_fused_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[FENCE + n:]).all()), "a fence around a2 was written"
    assert not bool(torch.isnan(a2).any())
    got = util.from_cb8(a2.view(N, 8, 2, S, S, 8), ZC.COUT).cpu()
    if kind == "int":
        assert torch.equal(util.from_cb8(h1, ZC.COUT).cpu().double(), F.conv3d(c["x"].double(), c["w"].double(), c["b"].double(), padding=1))
    bnd = ZC.bound(c, 0.0) if kind == "int" else ZC.bound(c)
    d = (got.double() - ZC.reference(c)).abs()
    print(f"fused {kind} {ZC.case_id(case)}: worst |d|/bound={ZC.worst(d, bnd):.4f}")
    assert bool((d <= bnd).all()), f"worst |d|/bound={ZC.worst(d, bnd):.3g}"
    assert torch.equal(got, util.from_cb8(sep, ZC.COUT).cpu()), "fused and separate mid-section differ in bits"
