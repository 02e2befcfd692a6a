"""The wide resident form of the fp32 block-input pass (tm_kernels.hip: prep_kernel with 16 waves per 64 voxels, the form
launch_prep takes for 33..160 channel blocks) through tm_op_prep_f32, against the four-wave two-pass kernel prep_kernel<1, false>
(variant 1), which stays the fallback and the reference: the wide form reads every source once and must not change a bit.

  * variant 2 == variant 1 in bits, `out` and `raw`, at 33 / 61 / 157 / 160 channel blocks, with one,
    two and three sources, collaged sources, a half-empty last workgroup, Z = 1, nearest x2 sources, and every modulation mode;
  * 161 blocks: the automatic choice is the four-wave kernel, variant 2 is refused (TM_ERR_ARG) before any device call;
  * variant 0 against a float64 torch model within the bound of test_gpu_train_ops.py::test_modnorm_forward on the
    pre-activation, ((C + 5) U + 5 U) |n (1 + s)| + 2 U |m|; through SiLU (|silu'| <= 1.1) 1.1 times that plus 6 U |ref| for
    the hardware exp2 / rcp (tm_device.h silu_h16).  test_reference_inside_bound (no GPU) first holds a float32 emulation of
    the kernel's own chain order to that bound on the same inputs, so the bound is not one an honest fp32 evaluation misses;
  * two calls give the same bits; the outputs start as NaN, so every element must be written.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import util
from oracle import teramind_cpu as tc
from teramind_amd import _lib

DEV = "cuda:0"
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
EPS = 1e-6
B, P1, P2 = 3, 2, 2                    # 3 images on a 2 x 2 encoder grid: N = 3 output patches, collaged sources have 12

# channel counts per source, collage flags -> 33, 61, 157, 160 channel blocks
SIZES = {
    "cb33": ((264,), (0,)),
    "cb61": ((256, 229), (0, 0)),
    "cb157": ((512, 512, 229), (0, 1, 1)),
    "cb160": ((1280,), (0,)),
}
# mod, act, per_image, mod_half
MODES = {
    "norm_silu": (0, 1, 1, 0),
    "image_1": (1, 1, 1, 0),
    "image_3": (1, 1, 3, 0),
    "voxel": (2, 0, 1, 0),
    "voxel_half": (2, 0, 1, 1),
}


def _inputs(cins, flags, Z, S, up2, mod, per_image, mod_half, seed=11):
    """Sources (NCDHW, on the CPU), norm weights per source, scale / shift, and the gathered concat the kernel normalises."""
    g = torch.Generator().manual_seed(seed)
    N, Ne = B * (P1 - 1) * (P2 - 1), B * P1 * P2
    Ss = S // 2 if up2 else S
    xs, parts = [], []
    for c, f in zip(cins, flags):
        x = torch.randn((Ne if f else N, c, Z, Ss, Ss), generator=g) * 1.5
        xs.append(x)
        y = tc.collage(x, B, P1, P2) if f else x
        if up2:
            y = y.repeat_interleave(2, 3).repeat_interleave(2, 4)
        parts.append(y)
    xcat = torch.cat(parts, 1)
    ws = [torch.rand((c,), generator=g) + 0.5 for c in cins]
    Ct = xcat.shape[1]
    scale = shift = None
    if mod == 1:
        scale, shift = torch.randn((N // per_image, Ct), generator=g) * 0.3, torch.randn((N // per_image, Ct), generator=g) * 0.3
    elif mod == 2:
        Sm = S // 2 if mod_half else S
        scale, shift = torch.randn((N, Ct, Z, Sm, Sm), generator=g) * 0.3, torch.randn((N, Ct, Z, Sm, Sm), generator=g) * 0.3
    return xs, ws, scale, shift, xcat


def _full_mod(t, mod, per_image, mod_half, N):
    """scale / shift broadcast to the output geometry"""
    if mod == 1:
        return t[torch.arange(N) // per_image][:, :, None, None, None]
    return t.repeat_interleave(2, 3).repeat_interleave(2, 4) if mod_half else t


def _reference(xcat, ws, scale, shift, mod, act, per_image, mod_half):
    """float64 result and the bound on |device - result|"""
    N, Ct = xcat.shape[:2]
    xd, wd = xcat.double(), torch.cat(ws).double()
    n = tc.rms_norm_channels(xd, wd)
    sc = _full_mod(scale.double(), mod, per_image, mod_half, N) if mod else torch.zeros(())
    sh = _full_mod(shift.double(), mod, per_image, mod_half, N) if mod else torch.zeros(())
    m = n * (1 + sc) + sh
    bound = ((Ct + 5) * U + 5 * U) * (n * (1 + sc)).abs() + 2 * U * m.abs()
    if not act:
        return m, bound + FLT_MIN
    ref = F.silu(m)
    return ref, 1.1 * bound + 6 * U * ref.abs() + FLT_MIN


def _fma(a, b, c):
    """fl32(a * b + c) for float32 tensors: the product of two floats is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def _emulate_f32(xcat, ws, scale, shift, mod, act, per_image, mod_half):
    """The kernel's evaluation in float32 arithmetic: 8-term fused chains per channel block, four chains over the blocks r, r + 4,
    ... from 0, c0 + c1 + c2 + c3, rstd = 1 / sqrt(fma(t, 1 / C, eps)), wn (x rstd), fma(v, 1 + s, sh), SiLU."""
    N, Ct = xcat.shape[:2]
    pad = (-Ct) % 8
    xp = torch.cat([xcat, torch.zeros((N, pad) + tuple(xcat.shape[2:]))], 1) if pad else xcat
    blk = xp.reshape(N, -1, 8, *xcat.shape[2:])
    e = blk[:, :, 0] * blk[:, :, 0]
    for j in range(1, 8):
        e = _fma(blk[:, :, j], blk[:, :, j], e)
    chains = []
    for r in range(4):
        c = torch.zeros_like(e[:, 0])
        for gb in range(r, e.shape[1], 4):
            c = c + e[:, gb]
        chains.append(c)
    t = ((chains[0] + chains[1]) + chains[2]) + chains[3]
    rstd = 1.0 / torch.sqrt(_fma(t, torch.tensor(1.0 / Ct, dtype=torch.float32), torch.tensor(EPS, dtype=torch.float32)))
    v = torch.cat(ws)[None, :, None, None, None] * (xcat * rstd[:, None])
    if mod:
        v = _fma(v, 1.0 + _full_mod(scale, mod, per_image, mod_half, N), _full_mod(shift, mod, per_image, mod_half, N))
    return F.silu(v) if act else v


def _run(xs, cins, flags, Z, S, up2, ws, mod, scale, shift, per_image, mod_half, act, variant, want_raw=True):
    """One tm_op_prep_f32 call on NaN-filled outputs.  Returns (rc, out CB8, raw CB8 or None)."""
    N = B * (P1 - 1) * (P2 - 1)
    xc = [util.to_cb8(x.to(DEV)) for x in xs]
    cbs = [(c + 7) // 8 for c in cins]
    nw = torch.zeros(sum(cbs) * 8, dtype=torch.float32, device=DEV)
    o = 0
    for w, c, cb in zip(ws, cins, cbs):
        nw[o:o + c] = w.to(DEV)
        o += cb * 8
    sc = sh = None
    stride = 0
    if mod == 1:
        # rows over the PADDED concat channel order, as the executor's emb rows are laid out
        sc, sh = torch.zeros((scale.shape[0], sum(cbs) * 8), device=DEV), torch.zeros((scale.shape[0], sum(cbs) * 8), device=DEV)
        o = oc = 0
        for c, cb in zip(cins, cbs):
            sc[:, o:o + c], sh[:, o:o + c] = scale[:, oc:oc + c].to(DEV), shift[:, oc:oc + c].to(DEV)
            o, oc = o + cb * 8, oc + c
        stride = sc.shape[1]
    elif mod == 2:
        sc, sh = _concat_cb8(scale, cins), _concat_cb8(shift, cins)
        stride = sc[0].numel()
    out = torch.full((N, sum(cbs), Z, S, S, 8), float("nan"), dtype=torch.float32, device=DEV)
    raw = torch.full_like(out, float("nan")) if want_raw else None
    ptrs = (C.c_void_p * len(xc))(*[t.data_ptr() for t in xc])
    cin = (C.c_int * len(xc))(*cins)
    col = (C.c_int * len(xc))(*[int(f) for f in flags])
    rc = _lib.lib().tm_op_prep_f32(ptrs, cin, col, len(xc), N, Z, S, P1, P2, int(up2), _lib.ptr(nw), sum(cins), mod, _lib.ptr(sc),
                                   _lib.ptr(sh), stride, int(mod_half), per_image, int(act), variant, _lib.ptr(out), _lib.ptr(raw),
                                   1, None, _lib.current_stream_ptr())
    return rc, out, raw


def _concat_cb8(t, cins):
    """NCDHW tensor over the concat's real channels -> CB8 with every source padded to whole blocks (the output's layout)"""
    parts, o = [], 0
    for c in cins:
        parts.append(util.to_cb8(t[:, o:o + c].contiguous().to(DEV)))
        o += c
    return torch.cat(parts, 1).contiguous()


def _split(t, cins):
    """CB8 output -> NCDHW over the real channels; the pad channels of every source must be written too (not NaN)"""
    assert not torch.isnan(t).any(), f"{int(torch.isnan(t).sum())} output elements not written"
    res, o = [], 0
    for c in cins:
        cb = (c + 7) // 8
        res.append(util.from_cb8(t[:, o:o + cb].contiguous(), c))
        o += cb
    return torch.cat(res, 1).cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _case(cins, flags, Z, S, up2, mode, check_ref=True):
    mod, act, per_image, mod_half = MODES[mode]
    xs, ws, scale, shift, xcat = _inputs(cins, flags, Z, S, up2, mod, per_image, mod_half)
    args = (xs, cins, flags, Z, S, up2, ws, mod, scale, shift, per_image, mod_half, act)
    rc1, out1, raw1 = _run(*args, 1)
    assert rc1 == 0, _lib.lib().tm_last_error()
    out0 = None
    for variant in (2, 0, 2):                           # the second variant 2 call: two calls, the same bits
        rc, out, raw = _run(*args, variant)
        out0 = out if variant == 0 else out0
        assert rc == 0, _lib.lib().tm_last_error()
        assert _same_bits(out, out1), f"variant {variant}: out differs from the four-wave kernel, " + util.report("out", out, out1)
        assert _same_bits(raw, raw1), f"variant {variant}: raw differs from the four-wave kernel"
    rc, out, raw = _run(*args, 2, want_raw=False)
    assert rc == 0 and raw is None and _same_bits(out, out1), "without the raw copy"
    assert torch.equal(_split(raw1, cins), xcat), "raw must be the gathered input, bit for bit"
    if check_ref:
        ref, bound = _reference(xcat, ws, scale, shift, mod, act, per_image, mod_half)
        got = _split(out0, cins).double()
        err = (got - ref).abs()
        print(f"{mode} {cins}: max err / bound = {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), util.report("variant 0 against float64", got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("mode", list(MODES))
def test_wide_form_equals_four_wave_kernel(size, mode):
    """N = 3, Z = 2, S = 4: 96 voxels, the second workgroup half empty."""
    cins, flags = SIZES[size]
    _case(cins, flags, 2, 4, False, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("size,Z,S,up2,mode", [
    ("cb61", 1, 6, False, "norm_silu"),                # 36 voxels: one workgroup, 28 lanes past the end
    ("cb157", 1, 6, False, "image_3"),
    ("cb61", 2, 4, True, "norm_silu"),                 # sources at S / 2 (the up block's input)
    ("cb33", 2, 4, True, "voxel_half")])
def test_wide_form_geometry(size, Z, S, up2, mode):
    cins, flags = SIZES[size]
    _case(cins, flags, Z, S, up2, mode)


@pytest.mark.gpu
def test_161_blocks_stay_with_the_four_wave_kernel():
    cins, flags = (1288,), (0,)
    mod, act, per_image, mod_half = MODES["norm_silu"]
    xs, ws, scale, shift, xcat = _inputs(cins, flags, 2, 4, False, mod, per_image, mod_half)
    args = (xs, cins, flags, 2, 4, False, ws, mod, scale, shift, per_image, mod_half, act)
    rc1, out1, raw1 = _run(*args, 1)
    rc0, out0, raw0 = _run(*args, 0)
    assert rc1 == 0 and rc0 == 0, _lib.lib().tm_last_error()
    assert _same_bits(out0, out1) and _same_bits(raw0, raw1)
    rc, out, _ = _run(*args, 2)
    assert rc == -1 and b"wide form" in _lib.lib().tm_last_error()
    assert torch.isnan(out).all(), "a refused call must not launch"


def test_wide_form_refusal_needs_no_device():
    """TM_ERR_ARG before any device call: the pointers are never dereferenced.  32 blocks (the cached four-wave form's), 161
    blocks, and a call that fits by size but is not one the wide form takes."""
    L = _lib.lib()
    buf = torch.zeros(8)
    p = _lib.ptr(buf)
    ptrs = (C.c_void_p * 1)(buf.data_ptr())
    col = (C.c_int * 1)(0)
    for c in (256, 1288):
        cin = (C.c_int * 1)(c)
        rc = L.tm_op_prep_f32(ptrs, cin, col, 1, 1, 2, 4, 2, 2, 0, p, c, 0, None, None, 0, 0, 1, 1, 2, p, None, 1, None, None)
        assert rc == -1 and b"wide form" in L.tm_last_error(), (c, rc, L.tm_last_error())
    cin = (C.c_int * 1)(264)
    assert L.tm_op_prep_f32(ptrs, cin, col, 1, 1, 2, 4, 2, 2, 0, p, 264, 0, None, None, 0, 0, 1, 1, 3, p, None, 1, None, None) == -1
    assert L.tm_op_prep_f32(ptrs, cin, col, 1, 1, 2, 4, 2, 2, 0, p, 264, 0, None, None, 0, 0, 1, 1, 2, None, None, 1, None, None) == -1


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("mode", list(MODES))
def test_reference_inside_bound(size, mode):
    """No GPU: the float32 emulation of the kernel's chain order sits inside the bound the GPU test applies, on its inputs."""
    cins, flags = SIZES[size]
    mod, act, per_image, mod_half = MODES[mode]
    xs, ws, scale, shift, xcat = _inputs(cins, flags, 2, 4, False, mod, per_image, mod_half)
    ref, bound = _reference(xcat, ws, scale, shift, mod, act, per_image, mod_half)
    emu = _emulate_f32(xcat, ws, scale, shift, mod, act, per_image, mod_half).double()
    assert bool(((emu - ref).abs() <= bound).all()), util.report("float32 emulation against float64", emu, ref)
