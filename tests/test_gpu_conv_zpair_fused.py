"""-m gpu: conv3d_zpair<0, TW, true> -- the fp32 pair-form conv with out_layers' RMSNorm -> modulate -> SiLU in its epilogue --
through tm_op_conv_zpair_fused_f32, against the float64 reference and inside the derived bound of tests/zpair_fused_cases.py.
The output sits between guard zones and is prefilled with NaN; every launch is repeated and must reproduce its bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import util
import zpair_fused_cases as ZC
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096            # floats in front of and behind a2
FENCE = -12345.0


def _run(c, with_plain):
    """Returns (a2 NCDHW, h1 NCDHW or None, a2_sep NCDHW or None), all on the CPU."""
    Cin, S, N, per_image = c["case"]
    xc = util.to_cb8(c["x"].to(DEV))
    hs = [c[k].contiguous().float() for k in ("w", "b", "nw", "sc", "sh")]
    n = N * 8 * 2 * S * S * 8
    L = _lib.lib()
    outs = []
    for _ in range(2):
        buf = torch.full((n + 2 * GUARD,), FENCE, dtype=torch.float32, device=DEV)
        a2 = buf[GUARD:GUARD + n]
        a2.fill_(float("nan"))
        h1 = torch.full((N, 8, 2, S, S, 8), float("nan"), device=DEV) if with_plain else None
        sep = torch.full((N, 8, 2, S, S, 8), float("nan"), device=DEV) if with_plain else None
        rc = L.tm_op_conv_zpair_fused_f32(_lib.ptr(xc), *[C.c_void_p(t.data_ptr()) for t in hs], None, _lib.ptr(a2), _lib.ptr(h1),
                                          _lib.ptr(sep), N, Cin, ZC.COUT, 2, S, per_image, 2, _lib.current_stream_ptr())
        _lib.check(rc, "tm_op_conv_zpair_fused_f32")
        assert bool((buf[:GUARD] == FENCE).all()) and bool((buf[GUARD + n:] == FENCE).all()), "a store outside a2"
        assert not bool(torch.isnan(a2).any()), "the kernel left elements of a2 unwritten"
        outs.append((a2.clone().view(N, 8, 2, S, S, 8), h1, sep))
    assert torch.equal(outs[0][0], outs[1][0]), "two launches on the same input differ"
    a2, h1, sep = outs[0]
    cpu = lambda t: None if t is None else util.from_cb8(t, ZC.COUT).cpu()
    return cpu(a2), cpu(h1), cpu(sep)


@pytest.mark.parametrize("case", ZC.CASES, ids=ZC.case_id)
def test_fused_random_vs_float64(case):
    c = ZC.make(case, "float")
    a2, _, sep = _run(c, True)
    bnd = ZC.bound(c)
    d = (a2.double() - ZC.reference(c)).abs()
    print(f"zpair fused float {ZC.case_id(case)}: max|d|={float(d.max()):.3e} worst |d|/bound={ZC.worst(d, bnd):.4f} "
          f"equal bits to the separate pass in {float((a2 == sep).float().mean()) * 100:.2f} %")
    assert bool((d <= bnd).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={ZC.worst(d, bnd):.3g}"
    # the epilogue adds the squares in prep_kernel's order: a layer gives the same bits whether a launch fuses or not
    assert torch.equal(a2, sep), "fused and separate mid-section differ in bits"


@pytest.mark.parametrize("case", ZC.CASES, ids=ZC.case_id)
def test_fused_integers_equal_the_separate_pass(case):
    """Integer x and w, zero bias: the conv sums are exact, so the plain launch's H1 equals F.conv3d bit for bit; the fused a2
    and the separate norm pass on that H1 are both inside the mid-section's own bound (conv error 0) -- and equal in bits,
    because the epilogue adds the 64 squares in the separate pass's order."""
    c = ZC.make(case, "int")
    a2, h1, sep = _run(c, True)
    assert torch.equal(h1, F.conv3d(c["x"], c["w"], c["b"], padding=1)), "the plain launch is not exact on integers"
    ref = ZC.reference(c)
    bnd = ZC.bound(c, 0.0)
    d, ds, dd = (a2.double() - ref).abs(), (sep.double() - ref).abs(), (a2.double() - sep.double()).abs()
    print(f"zpair fused int {ZC.case_id(case)}: fused worst |d|/bound={ZC.worst(d, bnd):.4f} separate {ZC.worst(ds, bnd):.4f} "
          f"fused vs separate max|d|={float(dd.max()):.3e} ({ZC.worst(dd, bnd):.4f} of the bound), "
          f"equal bits in {float((a2 == sep).float().mean()) * 100:.1f} %")
    assert bool((d <= bnd).all()), f"fused: worst |d|/bound={ZC.worst(d, bnd):.3g}"
    assert bool((ds <= bnd).all()), f"separate pass: worst |d|/bound={ZC.worst(ds, bnd):.3g}"
    assert torch.equal(a2, sep), "fused and separate mid-section differ in bits"


def test_refusals_launch_nothing():
    """Cout != 64, a residual, the 64-voxel (HALF) tile and Z != 2 are refused with TM_ERR_ARG; a2 keeps its NaN prefill."""
    L = _lib.lib()
    c = ZC.make(ZC.CASES[0], "float")
    Cin, S, N, per_image = c["case"]
    xc = util.to_cb8(c["x"].to(DEV))
    hs = [C.c_void_p(c[k].contiguous().float().data_ptr()) for k in ("w", "b", "nw", "sc", "sh")]
    keep = [c[k] for k in ("w", "b", "nw", "sc", "sh")]
    a2 = torch.full((N, 16, 2, S, S, 8), float("nan"), device=DEV)
    st = _lib.current_stream_ptr()
    for kw in ({"Cout": 128}, {"res": _lib.ptr(xc)}, {"variant": 1}, {"variant": 0}, {"Z": 4}, {"Z": 1}):
        a = {"Cout": 64, "res": None, "variant": 2, "Z": 2}
        a.update(kw)
        rc = L.tm_op_conv_zpair_fused_f32(_lib.ptr(xc), *hs, a["res"], _lib.ptr(a2), None, None, N, Cin, a["Cout"], a["Z"], S,
                                          per_image, a["variant"], st)
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(a2).all())
    del keep
