"""-m gpu: the 3x3x3 convs at the z sizes the Z = 2 tests never reach (rna_slc 1 / 8 / 16: Z = 1 / 4 / 8, plus Z = 3), one
kernel per call through the C-ABI, against F.conv3d(padding=1) on the CPU.

16-bit: at Z != 2 the 8-wave form is the 32x32x16 ping-pong kernel (conv27_pp), whose stage walk -- npl = 1, 2 or 3 input
planes per channel-block pair, boundary and interior planes in one launch, odd stage counts, a one-stage main loop -- and whose
block-id arithmetic (pg / (Z * tiles), zo, the tail split's unit and bid0) Z = 2 never varies.  fp32: the three-plane form
(conv3d_mfma<3, ..>, zoff = -1) with bias and residual in both tile variants, and the in-plane form at Z = 1 / 4 / 8.
Integer operands (tests/conv_z_cases.py: every sum below 2^24) make torch.equal the criterion; every output buffer is
prefilled with NaN, so an element or a pad slot the kernel leaves unwritten fails."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_z_cases as cz
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _flat(table):
    return [(Z,) + c for Z, cs in sorted(table.items()) for c in cs]


@functools.lru_cache(maxsize=None)
def _operands(N, Cin, Cout, Z, S, seed, kz=3):
    """Integer x, w, b, residual and the exact conv + bias (computed once per shape, shared by the dtypes / forms; read only)."""
    x = util.rand_int((N, Cin, Z, S, S), -cz.X_R, cz.X_R, seed)
    w = util.rand_int((Cout, Cin, kz, 3, 3), -cz.W_R, cz.W_R, seed + 1)
    b = util.rand_int((Cout,), -cz.B_R, cz.B_R, seed + 2)
    res = util.rand_int((N, Cout, Z, S, S), -cz.RES_R, cz.RES_R, seed + 3)
    ref = F.conv3d(x, w, b, padding=(kz // 2, 1, 1))
    return x, w, b, res, ref


def _pads_zero(raw, Cout):
    return Cout % 8 == 0 or float(raw[:, -1, ..., Cout % 8:].abs().max()) == 0.0


# ---- 16-bit 3x3x3, forced workgroup forms --------------------------------------------------------------------------
@pytest.mark.parametrize("Z,N,Cin,Cout,S", _flat(cz.H16_CASES))
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv27_h16_exact_integers(Z, N, Cin, Cout, S, waves, dtype):
    """fp32 CB8 output of the 4-wave kernel (conv27_bf16<.., 4>) and the 8-wave ping-pong kernel (conv27_pp), bit for bit."""
    x, w, b, _, ref = _operands(N, Cin, Cout, Z, S, 141)
    got, raw = util.conv27_h16_z(x.to(DEV), w, b, dtype, waves)
    assert torch.equal(got.cpu(), ref), util.report(f"conv27 {dtype} Z={Z} waves={waves}", got, ref)
    assert _pads_zero(raw, Cout), "output pad slots must read zero"


@pytest.mark.parametrize("Z,N,Cin,Cout,S", [(Z,) + c for Z, c in sorted(cz.H16_LOCKSTEP.items())])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv27_h16_lockstep_form_exact_integers(Z, N, Cin, Cout, S, dtype):
    """waves = 9: the lockstep 8-wave kernel (conv27_bf16<.., 8>), kept for A/B against the ping-pong one."""
    x, w, b, _, ref = _operands(N, Cin, Cout, Z, S, 141)
    got, raw = util.conv27_h16_z(x.to(DEV), w, b, dtype, 9)
    assert torch.equal(got.cpu(), ref), util.report(f"conv27 lockstep {dtype} Z={Z}", got, ref)
    assert _pads_zero(raw, Cout), "output pad slots must read zero"


# ---- the model's forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,N,Cin,Cout,S", _flat(cz.STREAM_CASES))
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv27_h16_stream_epilogue(Z, N, Cin, Cout, S, waves, dtype):
    """16-bit CB8 residual in, 16-bit CB8 result out: conv + bias + res is exact in fp32, rounded once to the 16-bit type."""
    td = util.H16[dtype][1]
    x, w, b, res, conv = _operands(N, Cin, Cout, Z, S, 171)
    ref = (conv + res).to(td).float()
    got, raw = util.conv27_h16_z(x.to(DEV), w, b, dtype, waves, res=res.to(DEV), out16=True)
    assert torch.equal(got.cpu(), ref), util.report(f"conv27 stream {dtype} Z={Z} waves={waves}", got, ref)
    assert _pads_zero(raw, Cout), "output pad slots must read zero"


@pytest.mark.parametrize("Z,N,Cin,Cout,S,per_image", _flat(cz.FUSED_CASES))
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv27_h16_fused_norm_modulate_silu_epilogue(Z, N, Cin, Cout, S, per_image, waves, dtype):
    """conv + bias -> RMSNorm(C) * w -> x(1 + scale) + shift -> SiLU -> 16-bit, at the criterion of the Z = 2 test
    (test_gpu_ops.test_conv27_fused_norm_modulate_silu_epilogue): half a 16-bit ulp of the final rounding plus the fp32
    rounding of the norm."""
    g = torch.Generator().manual_seed(61)
    x, w, b, _, v = _operands(N, Cin, Cout, Z, S, 161)
    nimg = (N + per_image - 1) // per_image
    nw = torch.rand(Cout, generator=g) + 0.5
    sc, sh = torch.randn((nimg, Cout), generator=g) * 0.3, torch.randn((nimg, Cout), generator=g) * 0.3
    img = torch.arange(N) // per_image
    ref = v * torch.rsqrt(v.pow(2).mean(1, keepdim=True) + 1e-6) * nw.view(1, -1, 1, 1, 1)
    ref = ref * (1 + sc[img].view(N, Cout, 1, 1, 1)) + sh[img].view(N, Cout, 1, 1, 1)
    ref = ref * torch.sigmoid(ref)
    got = util.conv27_fused_z(x.to(DEV), w, b, nw, sc, sh, per_image, dtype, waves).cpu()
    ulp = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    err = ((got - ref).abs() / (ref.abs() * ulp + 1e-4)).max().item()
    assert err <= 1.01, (err, util.report(f"fused {dtype} Z={Z}", got, ref))       # NaN (unwritten) fails: nan <= 1.01 is False


# ---- automatic form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cin,Cout,Z,S", cz.TAIL_SPLIT_CASES)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv27_h16_tail_split_launch(N, Cin, Cout, Z, S, dtype):
    """waves = 0 on launches that split on this device: `full` 8-wave workgroups on the ping-pong kernel, the remaining
    patch groups as 4-wave workgroups from block id 2 * full (unit = ntile * Z * tiles8).  The union must be exactly the
    layer, with the 16-bit residual / output epilogue."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    r = cz.tail_split(N, Cout, Z, S, ncu)
    assert r["split"], f"this launch does not split on {ncu} CUs: {r}"
    td = util.H16[dtype][1]
    x, w, b, res, conv = _operands(N, Cin, Cout, Z, S, 191)
    ref = (conv + res).to(td).float()
    got, _ = util.conv27_h16_z(x.to(DEV), w, b, dtype, 0, res=res.to(DEV), out16=True)
    assert torch.equal(got.cpu(), ref), util.report(f"conv27 tail split {dtype} Z={Z}", got, ref)


@pytest.mark.parametrize("N,Cin,Cout,Z,S", cz.AUTO_SMALL_CASES)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv27_h16_automatic_small_launch(N, Cin, Cout, Z, S, dtype):
    """waves = 0 on a launch of fewer than 256 8-wave workgroups: the launcher's 4-wave choice."""
    assert not cz.tail_split(N, Cout, Z, S, torch.cuda.get_device_properties(0).multi_processor_count)["w8"]
    td = util.H16[dtype][1]
    x, w, b, res, conv = _operands(N, Cin, Cout, Z, S, 191)
    ref = (conv + res).to(td).float()
    got, _ = util.conv27_h16_z(x.to(DEV), w, b, dtype, 0, res=res.to(DEV), out16=True)
    assert torch.equal(got.cpu(), ref), util.report(f"conv27 auto {dtype} Z={Z}", got, ref)


# ---- random operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cin,Cout,Z,S", cz.RANDOM_CASES)
def test_conv27_h16_random_vs_float64(N, Cin, Cout, Z, S):
    """Random operands rounded to the 16-bit type (products exact in fp32), against F.conv3d in float64 on the same operands.
    Bound per element: K * 2^-23 * (conv(|x|, |w|) + |b|) with K = 27 * 16 * Cbp + 1 terms -- the worst-case bound of a sum
    of K terms in ANY order with a truncating unit roundoff (the MFMA's internal accumulation order and rounding are not
    ours to state).  One dropped product is typically 1 / K of the magnitude sum: 2^23 / K^2 = 2.8 times the bound at
    K = 1729 (Cin = 64).  Prints max(error / bound) per form (recorded in profiles/conv_zsizes_tests.txt)."""
    g = torch.Generator().manual_seed(17 + Z)
    K = 27 * 16 * cz.cbp_of(Cin) + 1
    for dtype in ("bf16", "f16"):
        td = util.H16[dtype][1]
        x = torch.randn((N, Cin, Z, S, S), generator=g).to(td).float()
        w = (torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5).to(td).float()
        b = torch.randn((Cout,), generator=g)
        ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
        mag = F.conv3d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
        bound = K * 2.0 ** -23 * mag
        for waves in (4, 8):
            got, _ = util.conv27_h16_z(x.to(DEV), w, b, dtype, waves)
            ratio = ((got.cpu().double() - ref).abs() / bound).max().item()
            print(f"conv27 random Z={Z} {dtype} waves={waves}: max error / bound = {ratio:.3e}")
            assert ratio <= 1.0, (ratio, util.report(f"conv27 random {dtype} Z={Z} waves={waves}", got, ref))


# ---- fp32 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cin,Cout,Z,S", cz.F32_CASES)
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("with_res", [False, True])
def test_conv3_f32_three_plane_form_exact_integers(N, Cin, Cout, Z, S, variant, with_res):
    """tm_op_conv_mfma_res, zmode 0 at Z != 2: conv3d_mfma<3, ..> with zoff = -1 (planes in the zero padding skipped), with
    bias, with and without the epilogue's residual, in both tile variants (S = 4 has one)."""
    x, w, b, res, conv = _operands(N, Cin, Cout, Z, S, 111)
    ref = conv + res if with_res else conv
    got, raw = util.conv_mfma_res(x.to(DEV), w, b, res.to(DEV) if with_res else None, variant)
    assert torch.equal(got.cpu(), ref), util.report(f"conv3 fp32 Z={Z} v{variant}", got, ref)
    assert _pads_zero(raw, Cout), "output pad slots must read zero"


@pytest.mark.parametrize("N,Cin,Cout,Z,S", cz.F32_INPLANE_CASES)
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("up2", [False, True])
def test_conv_inplane_f32_exact_integers(N, Cin, Cout, Z, S, variant, up2):
    """1x3x3 in-plane conv (zmode 1: the RNA pyramid, and the centre slice of a 3x3x3 pad-1 conv at Z = 1) with and without
    the fused nearest-x2 store."""
    x, w, b, _, ref = _operands(N, Cin, Cout, Z, S, 121, kz=1)
    if up2:
        ref = ref.repeat_interleave(2, -2).repeat_interleave(2, -1)
    got, raw = util.conv_mfma(x.to(DEV), w, b, 3, variant, zmode=1, up2=up2)
    assert torch.equal(got.cpu(), ref), util.report(f"conv 1x3x3 Z={Z} v{variant}", got, ref)
    assert _pads_zero(raw, Cout), "output pad slots must read zero"


def test_inplane_form_is_the_centre_slice_of_the_pad1_conv_at_z1():
    """At Z = 1 only kz = 1 of a 3x3x3 pad-1 filter meets data: the three-plane form on the full filter and the in-plane form
    on its centre slice must give the same bits."""
    N, Cin, Cout, Z, S = 3, 24, 64, 1, 8
    x, w, b, _, ref = _operands(N, Cin, Cout, Z, S, 111)
    full, _ = util.conv_mfma_res(x.to(DEV), w, b)
    centre, _ = util.conv_mfma(x.to(DEV), w[:, :, 1:2].contiguous(), b, 3, zmode=1)
    assert torch.equal(full, centre) and torch.equal(full.cpu(), ref)
