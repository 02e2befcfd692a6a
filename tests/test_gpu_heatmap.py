"""-m gpu: tm_heat_field against the float64 model within the derived bound of heatmap_cases.py (every case: both kernel
forms, every mode, K = 1, 2, 8, radii 0 .. 16, more than two workgroup tiles each way), in place on a pitched, channel-strided
view with the destination's surroundings untouched, and with equal bits on a second call; tm_heat_render byte for byte against
the float32 restatement (every scale, both table lengths, floor, out-of-range values and NaN, planar and interleaved, pitched
both ways); argument errors as TM_ERR_ARG texts before any device call.

Measured on an MI355X: max|d| of tm_heat_field 6e-8 .. 7e-7 over the cases, |d| / bound 0.004 .. 0.23 (the worst at r = 0, where
the bound is the logarithm's alone); the bound is derived in heatmap_cases.py and was not tuned on these figures, which every
run prints (-s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import heatmap_cases as hc
from teramind_amd import _lib, heatmap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = list(hc.FIELD_CASES)


def call_field(src, Cn, H, W, spitch, schan, sum0, nsum, wei, mask0, nmask, taps, r, dst, dpitch):
    t = np.ascontiguousarray(taps, dtype=np.float32)
    return _lib.lib().tm_heat_field(C.c_void_p(src), Cn, H, W, spitch, schan, sum0, nsum, wei, mask0, nmask,
                                    t.ctypes.data_as(C.POINTER(C.c_float)), r, C.c_void_p(dst), dpitch, _lib.current_stream_ptr())


def gpu_field(name):
    K, H, W, sigma, mode, gene = hc.FIELD_CASES[name]
    src = torch.from_numpy(np.array(hc.mosaic_slice(name))).to(DEV)
    return heatmap.field(src, K, mode, hc.WEI, sigma, gene)


@pytest.mark.parametrize("name", NAMES)
def test_field_is_the_float64_model_within_the_derived_bound(name):
    ref, bound = hc.field_reference(name)
    a = gpu_field(name)
    b = gpu_field(name)
    got = a.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    d = np.abs(got.astype(np.float64) - ref).max()
    print(f"{name}: max|d| = {d:.3e}, bound {bound:.3e}, ratio {d / bound:.3f}")
    assert d <= bound
    assert torch.equal(a, b), "two calls give the same bits"
    for v in hc.variants_of(name):                                  # the kernel is none of the wrong variants
        with np.errstate(invalid="ignore"):
            assert np.nanmax(np.abs(hc.variant_field(name, v) - got)) > bound, v


def test_numpy_slice_is_uploaded_and_gives_the_same_field():
    name = "odd_17x33"
    K, H, W, sigma, mode, gene = hc.FIELD_CASES[name]
    assert torch.equal(heatmap.field(np.array(hc.mosaic_slice(name)), K, mode, hc.WEI, sigma, gene), gpu_field(name))


@pytest.mark.parametrize("name", ["tiles_70x150", "tiles_s4_70x150", "expr_17x33"])
def test_field_reads_a_strided_view_in_place_and_writes_only_its_cells(name):
    K, H, W, sigma, mode, gene = hc.FIELD_CASES[name]
    sum0, nsum, wei, mask0, nmask, r, taps = hc.field_args(name)
    big = torch.full((4 * K + 1, H + 5, W + 7), 7.0, dtype=torch.float16, device=DEV)     # junk around the window
    view = big[1:, 3:3 + H, 2:2 + W]
    view.copy_(torch.from_numpy(np.array(hc.mosaic_slice(name))))
    assert not view.is_contiguous()
    want = gpu_field(name)
    assert torch.equal(heatmap.field(view, K, mode, hc.WEI, sigma, gene), want)           # the wrapper passes the strides on
    dst = torch.full((H + 3, W + 9), -777.0, dtype=torch.float32, device=DEV)             # a pitched destination, sentinel around
    sub = dst[1:1 + H, 4:4 + W]
    rc = call_field(view.data_ptr(), 4 * K, H, W, view.stride(1), view.stride(0), sum0, nsum, wei, mask0, nmask, taps, r,
                    sub.data_ptr(), dst.stride(0))
    _lib.check(rc, "tm_heat_field")
    torch.cuda.synchronize()
    assert torch.equal(sub, want)
    keep = torch.ones_like(dst, dtype=torch.bool)
    keep[1:1 + H, 4:4 + W] = False
    assert bool((dst[keep] == -777.0).all()), "cells of dst outside [H][W] keep the sentinel"


# ---- render ------------------------------------------------------------------------------------------------------------
def luts(N):
    return heatmap.INFERNO if N == 256 else hc.two_colour((0, 1, 0.82), N)


@pytest.fixture(scope="module")
def fields():
    return {s: torch.from_numpy(np.array(hc.render_field(s))).to(DEV) for s in hc.RENDER_SHAPES}


@pytest.mark.parametrize("floor", [0, 3])
@pytest.mark.parametrize("N", [256, 100])
@pytest.mark.parametrize("scale", hc.SCALES)
@pytest.mark.parametrize("shape", hc.RENDER_SHAPES)
def test_render_equals_the_float32_restatement_byte_for_byte(fields, shape, scale, N, floor):
    lut = luts(N)
    want = hc.render_ref(hc.render_field(shape), lut, hc.VMIN, hc.VMAX, scale, floor)
    planes = heatmap.render(fields[shape], lut, hc.VMIN, hc.VMAX, scale, floor)
    inter = heatmap.render(fields[shape], lut, hc.VMIN, hc.VMAX, scale, floor, interleaved=True)
    got = inter.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ"
    assert torch.equal(torch.stack(planes, -1), inter), "planar and interleaved agree"
    if scale == 1:
        with np.errstate(invalid="ignore"):
            idx = hc.index_ref(hc.render_field(shape), hc.VMIN, hc.VMAX, N)
        assert idx[0, 0] == 0 and idx[0, 1] == N - 1 and idx[1, 0] == N - 1 and idx[1, 1] == 0


def call_render(fld, lut, scale, floor, planes=None, pitches=None, inter=None, ipitch=0, N=None, H=None, W=None, fpitch=None):
    H = fld.shape[0] if H is None else H
    W = fld.shape[1] if W is None else W
    lut = np.ascontiguousarray(lut)
    pp = None if planes is None else (C.c_void_p * 3)(*planes)
    pt = None if pitches is None else (C.c_int64 * 3)(*pitches)
    inv = float(np.float32(1.0 / (hc.VMAX - hc.VMIN)))
    return _lib.lib().tm_heat_render(C.c_void_p(fld.data_ptr()), H, W, fld.stride(0) if fpitch is None else fpitch, scale, hc.VMIN, inv,
                                     lut.ctypes.data_as(C.c_void_p), len(lut) if N is None else N, floor, pp, pt,
                                     None if inter is None else C.c_void_p(inter), ipitch, _lib.current_stream_ptr())


@pytest.mark.parametrize("odd", [0, 1], ids=["dword_pitch", "odd_pitch"])
@pytest.mark.parametrize("scale", [1, 4])
def test_render_into_pitched_destinations_and_from_a_pitched_field(fields, scale, odd):
    """Destinations inside larger buffers, at pitches and offsets that are (the dword stores) and are not (the byte stores)
    multiples of 4; the field itself is a window of a wider tensor.  Bytes outside the image keep a sentinel."""
    shape = (33, 17)
    H, W = shape
    h, w = H * scale, W * scale
    lut = luts(256)
    want = hc.render_ref(hc.render_field(shape), lut, hc.VMIN, hc.VMAX, scale, 3)
    wide = torch.zeros((H, W + 6), dtype=torch.float32, device=DEV)
    fld = wide[:, 5:5 + W]
    fld.copy_(fields[shape])
    off = 4 + odd
    bufs = [torch.full((h + 2, (w + 15) // 4 * 4 + odd), 99, dtype=torch.uint8, device=DEV) for _ in range(3)]
    subs = [b[1:1 + h, off:off + w] for b in bufs]
    _lib.check(call_render(fld, lut, scale, 3, planes=[s.data_ptr() for s in subs], pitches=[b.stride(0) for b in bufs]), "planar")
    ibuf = torch.full((h + 2, (3 * w + 19) // 4 * 4 + odd), 99, dtype=torch.uint8, device=DEV)
    isub = ibuf[1:1 + h, off:off + 3 * w]
    _lib.check(call_render(fld, lut, scale, 3, inter=isub.data_ptr(), ipitch=ibuf.stride(0)), "interleaved")
    torch.cuda.synchronize()
    for c in range(3):
        assert np.array_equal(subs[c].cpu().numpy(), want[..., c]), f"plane {c}"
        rest = bufs[c].clone()
        rest[1:1 + h, off:off + w] = 99
        assert bool((rest == 99).all()), f"plane {c}: bytes outside the image were written"
    assert np.array_equal(isub.cpu().numpy().reshape(h, w, 3), want)
    rest = ibuf.clone()
    rest[1:1 + h, off:off + 3 * w] = 99
    assert bool((rest == 99).all())


# ---- argument errors: TM_ERR_ARG with a text, no device call (the pointers below are never dereferenced) -----------------
def test_field_argument_errors():
    L = _lib.lib()
    src = torch.zeros((8, 16, 16), dtype=torch.float16, device=DEV)
    dst = torch.full((16, 16), -1.0, dtype=torch.float32, device=DEV)
    r2, t2 = hc.gaussian_taps(2.0)
    ok = dict(src=src.data_ptr(), Cn=8, H=16, W=16, spitch=16, schan=256, sum0=4, nsum=2, wei=229.0, mask0=6, nmask=2, taps=t2, r=r2,
              dst=dst.data_ptr(), dpitch=16)
    bad = [(dict(nsum=0), "nsum"), (dict(nsum=9), "nsum"), (dict(r=17, taps=np.ones(35)), "radius"), (dict(H=7, schan=7 * 16), "below the radius"),
           (dict(W=7, spitch=7, dpitch=7), "below the radius"), (dict(src=0), "null"), (dict(dst=0), "null"), (dict(nmask=9), "nmask"),
           (dict(sum0=7), "sum range"), (dict(mask0=7), "mask range"), (dict(spitch=15), "source pitch"), (dict(dpitch=15), "destination pitch"),
           (dict(schan=255), "channel stride"), (dict(H=0), "positive")]
    for change, text in bad:
        rc = call_field(**{**ok, **change})
        assert rc == -1, change
        assert text in L.tm_last_error().decode(), (change, L.tm_last_error().decode())
    assert L.tm_heat_field(C.c_void_p(src.data_ptr()), 8, 16, 16, 16, 256, 4, 2, 229.0, 6, 2, None, 8, C.c_void_p(dst.data_ptr()), 16, None) == -1
    torch.cuda.synchronize()
    assert bool((dst == -1.0).all()), "a refused call launches nothing"
    _lib.check(call_field(**ok), "tm_heat_field")
    with pytest.raises(ValueError, match="4 K"):
        heatmap.field(src, 3, "att_all")
    with pytest.raises(RuntimeError, match="below the radius"):
        heatmap.field(src[:, :7], 2, "att_all", sigma=2.0)


def test_render_argument_errors(fields):
    L = _lib.lib()
    fld = fields[(7, 5)]
    out = torch.full((7, 5, 3), 9, dtype=torch.uint8, device=DEV)
    lut = luts(256)
    p3 = [out.data_ptr()] * 3
    bad = [(dict(scale=3, inter=out.data_ptr(), ipitch=15), "scale"), (dict(scale=0, inter=out.data_ptr(), ipitch=15), "scale"),
           (dict(scale=1, N=1, inter=out.data_ptr(), ipitch=15), "table length"), (dict(scale=1, N=257, inter=out.data_ptr(), ipitch=15), "table length"),
           (dict(scale=1), "one of the two"), (dict(scale=1, inter=out.data_ptr(), ipitch=15, planes=p3, pitches=[5] * 3), "one of the two"),
           (dict(scale=1, planes=[out.data_ptr(), 0, out.data_ptr()], pitches=[5] * 3), "null"), (dict(scale=1, inter=out.data_ptr(), ipitch=14), "pitch"),
           (dict(scale=2, planes=p3, pitches=[10, 9, 10]), "pitch"), (dict(scale=1, floor=-1, inter=out.data_ptr(), ipitch=15), "floor"),
           (dict(scale=1, inter=out.data_ptr(), ipitch=15, fpitch=4), "field pitch"), (dict(scale=1, inter=out.data_ptr(), ipitch=15, H=0), "positive")]
    for change, text in bad:
        kw = dict(floor=0)
        kw.update(change)
        rc = call_render(fld, lut, **kw)
        assert rc == -1, change
        assert text in L.tm_last_error().decode(), (change, L.tm_last_error().decode())
    inv = float(np.float32(1.0))
    assert L.tm_heat_render(None, 7, 5, 5, 1, 0.0, inv, lut.ctypes.data_as(C.c_void_p), 256, 0, None, None, C.c_void_p(out.data_ptr()), 15, None) == -1
    assert L.tm_heat_render(C.c_void_p(fld.data_ptr()), 7, 5, 5, 1, 0.0, inv, None, 256, 0, None, None, C.c_void_p(out.data_ptr()), 15, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 9).all()), "a refused call launches nothing"
    with pytest.raises(ValueError, match="scale"):
        heatmap.render(fld, lut, 0.0, 1.0, scale=3)
    with pytest.raises(ValueError, match="vmax"):
        heatmap.render(fld, lut, 1.0, 1.0)
