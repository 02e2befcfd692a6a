"""-m gpu: the pair form of the fp32 3x3x3 pad-1 conv at Z = 2 (conv3d_zpair) through the single-op hooks.

With W0, W1, W2 the kz slices of the filter and X0, X1 the two input planes the kernel computes three in-plane products per
plane pair, P1 = W1 * (X0 + X1), P2 = (W2 - W1) * X1, P3 = (W0 - W1) * X0, and Y0 = P1 + P2, Y1 = P1 + P3.  Small-integer
operands keep every intermediate exact in fp32, so those cases must equal F.conv3d bit for bit; random floats are held to a
bound derived from the kernel's fixed accumulation order (see _bound).  Every output buffer is prefilled with NaN (a voxel or
a pad slot the kernel does not write fails the comparison) and every launch is repeated and must reproduce its bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24            # fp32 unit roundoff (round to nearest)


def _run(x, w, b, variant, res=None, res_half=False):
    """x [N, Cin, 2, S, S] cuda, w / b host; res NCDHW cuda at S (or S / 2 with res_half).  Returns (NCDHW, raw CB8)."""
    N, Cin, Z, S, _ = x.shape
    Cout = w.shape[0]
    xc = util.to_cb8(x)
    wh, bh = w.contiguous().float(), b.contiguous().float()
    L = _lib.lib()
    outs = []
    for _ in range(2):
        yc = torch.full((N, (Cout + 7) // 8, Z, S, S, 8), float("nan"), dtype=torch.float32, device=x.device)
        if res is None:
            rc = L.tm_op_conv_mfma(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                   N, Cin, Cout, Z, S, 3, 0, 0, variant, _lib.current_stream_ptr())
        else:
            rcb = util.to_cb8(res)
            rc = L.tm_op_conv_mfma_res(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                       _lib.ptr(rcb), int(res_half), N, Cin, Cout, Z, S, 3, 0, 0, variant,
                                       _lib.current_stream_ptr())
        _lib.check(rc, "tm_op_conv_mfma")
        outs.append(yc)
    assert not bool(torch.isnan(outs[0]).any()), "the kernel left output elements unwritten"
    assert torch.equal(outs[0], outs[1]), "two launches on the same input differ"
    return util.from_cb8(outs[0], Cout), outs[0]


def _up2(r):
    return r.repeat_interleave(2, dim=-1).repeat_interleave(2, dim=-2)


def _residual(mode, N, Cout, S, seed, integers):
    """mode 0: none, 1: at the output's resolution, 2: at half the in-plane resolution (read at (z, y >> 1, x >> 1))"""
    if mode == 0:
        return None, None
    Sr = S // 2 if mode == 2 else S
    if integers:
        r = util.rand_int((N, Cout, 2, Sr, Sr), -9, 9, seed)
    else:
        r = torch.randn((N, Cout, 2, Sr, Sr), generator=torch.Generator().manual_seed(seed))
    return r, (_up2(r) if mode == 2 else r)


# (N, Cin, Cout, S): every S the launcher takes; N = 3, 5 leave the last workgroup of the S = 4 / 8 tiles partly empty (4, 2 or 1
# patches per workgroup); Cin / Cout off the multiples of 8 (pad slots), Cout > 64 (several cout tiles), Cin > 8 (several stages)
INT_CASES = [(5, 13, 32, 4), (3, 16, 72, 4), (3, 24, 128, 8), (5, 13, 37, 8), (1, 8, 64, 16), (2, 40, 192, 16),
             (1, 72, 64, 32), (2, 11, 70, 32), (1, 8, 64, 64), (2, 16, 136, 64), (1, 9, 72, 128)]


@pytest.mark.parametrize("res_mode", [0, 1, 2])
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,S", INT_CASES)
def test_zpair_exact_integers(N, Cin, Cout, S, variant, res_mode):
    x = util.rand_int((N, Cin, 2, S, S), -3, 3, 11)
    w = util.rand_int((Cout, Cin, 3, 3, 3), -2, 2, 12)
    b = util.rand_int((Cout,), -4, 4, 13)
    res, res_full = _residual(res_mode, N, Cout, S, 14, True)
    ref = F.conv3d(x, w, b, padding=1)
    if res is not None:
        ref = ref + res_full
    got, raw = _run(x.to(DEV), w, b, variant, None if res is None else res.to(DEV), res_mode == 2)
    assert torch.equal(got.cpu(), ref), util.report("zpair", got, ref)
    if Cout % 8:
        assert float(raw[:, -1, ..., Cout % 8:].abs().max()) == 0.0         # pad slots of the last cout block


def _bound(x, w, b, res_full):
    """(L + c) U mag per output element.

    The kernel accumulates each product in one fixed fp32 order over the padded Cin x 9 in-plane taps, and adds two
    products at the end: L = 8 ceil(Cin / 8) * 9 + 1 roundings, each at most U times the running sum of |terms|.  c counts the
    roundings outside that chain: the pack-time weight difference (1), the plane add X0 + X1 (1), the bias add (1), the
    residual add (1, when there is one), and 1 for the second-order terms of (1 + U)^n.  mag is the three-product expression on
    absolute values in float64: |W1| * (|X0| + |X1|) + (|W2| + |W1|) * |X1| + |b| for plane 0, the same with (W0, X0) for
    plane 1, plus |res|."""
    Cin = x.shape[1]
    L = (Cin + 7) // 8 * 8 * 9 + 1
    c = 4 + (1 if res_full is not None else 0)
    xa, wa = x.double().abs(), w.double().abs()
    x0, x1 = xa[:, :, 0], xa[:, :, 1]
    w0, w1, w2 = wa[:, :, 0], wa[:, :, 1], wa[:, :, 2]
    p1 = F.conv2d(x0 + x1, w1, padding=1)
    m0 = p1 + F.conv2d(x1, w2 + w1, padding=1)
    m1 = p1 + F.conv2d(x0, w0 + w1, padding=1)
    mag = torch.stack([m0, m1], dim=2) + b.double().abs().view(1, -1, 1, 1, 1)
    if res_full is not None:
        mag = mag + res_full.double().abs()
    return (L + c) * U * mag


FLOAT_CASES = [(2, 96, 64, 16, 0), (1, 741, 512, 8, 0), (1, 224, 64, 64, 0), (3, 61, 130, 8, 1), (1, 40, 72, 32, 2),
               (5, 29, 64, 4, 1)]


@pytest.mark.parametrize("N,Cin,Cout,S,res_mode", FLOAT_CASES)
def test_zpair_random_vs_float64(N, Cin, Cout, S, res_mode):
    g = torch.Generator().manual_seed(21)
    x = torch.randn((N, Cin, 2, S, S), generator=g)
    w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5
    b = torch.randn((Cout,), generator=g)
    res, res_full = _residual(res_mode, N, Cout, S, 22, False)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    if res is not None:
        ref = ref + res_full.double()
    bound = _bound(x, w, b, res_full)
    outs = []
    for variant in (1, 2):
        got, raw = _run(x.to(DEV), w, b, variant, None if res is None else res.to(DEV), res_mode == 2)
        d = (got.double().cpu() - ref).abs()
        print(f"zpair random N{N} Cin{Cin} Cout{Cout} S{S} res{res_mode} v{variant}: max|d|={float(d.max()):.3e} "
              f"worst |d|/bound={float((d / bound).max()):.4f}")
        assert bool((d <= bound).all()), f"max|d|={float(d.max()):.3e}, worst |d|/bound={float((d / bound).max()):.3g}"
        outs.append(raw)
    # both tiles run every output element through the same order: cin block, product, tap, k
    assert torch.equal(outs[0], outs[1]), "the 64- and 128-voxel tiles differ in bits"


def test_zpair_residual_hook_argument_checks():
    """The residual hook rejects the forms without a residual epilogue before any launch (TM_ERR_ARG = -1)."""
    L = _lib.lib()
    t = torch.zeros(4096, device=DEV)
    h = torch.zeros(4096)
    p, hp = _lib.ptr(t), C.c_void_p(h.data_ptr())
    assert L.tm_op_conv_mfma_res(p, hp, hp, p, p, 0, 1, 8, 8, 2, 4, 1, 0, 0, 0, None) == -1      # 1x1x1
    assert L.tm_op_conv_mfma_res(p, hp, hp, p, p, 0, 1, 8, 8, 2, 4, 3, 3, 0, 0, None) == -1      # upsampled-input form
    assert L.tm_op_conv_mfma_res(p, hp, hp, p, None, 1, 1, 8, 8, 2, 4, 3, 0, 0, 0, None) == -1   # res_half without res
