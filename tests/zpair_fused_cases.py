"""Cases, float64 reference and error bound of the fp32 pair-form conv with the ResBlock mid-section in its epilogue
(conv3d_zpair<0, TW, true>, hook tm_op_conv_zpair_fused_f32).  Shared by tests/test_zpair_fused_host.py (no GPU: the bound is held
by a float32 evaluation on the CPU) and tests/test_gpu_conv_zpair_fused.py.

The operation, per voxel, with h = conv3d(x, w, pad 1) + b over 64 channels (Z = 2):
    m = mean_c(h_c^2) + eps        r = 1 / sqrt(m)        y_c = nw_c (h_c r)        v_c = y_c (1 + sc_c) + sh_c
    a2_c = v_c rcp(1 + exp2(-log2(e) v_c))                                          (silu_h16, tm_device.h)
eps = 1e-6, scale / shift rows per image (patch n uses row n // per_image): prep_kernel's formulas, term for term.

BOUND on |a2 - float64 reference|, per element, first order in U = 2^-24 with the factor SECOND for the (1 + U)^n tails:
  e_c    the conv bound of tests/test_gpu_conv_zpair.py, (L + 4) U mag_c, L = 8 ceil(Cin / 8) * 9 + 1 (pack-time weight difference,
         plane add, bias add, second-order term: c = 4; no residual here);
  dS     error of the sum of squares S = sum_c h_c^2: sum_c (2 |h_c| e_c + e_c^2) from the conv error, plus 12 U S for forming
         it -- every term is a square, so the running sum of |terms| is S, and a term passes through its own rounded product
         (1), at most 7 adds of its 8-channel chain, 1 add of two chains and 3 adds of the four partial sums: 12 roundings
         (the kernel and the separate pass add in the same order: prep_kernel's);
  rel_r  relative error of r: (dS / 64) / (2 m) from S (d sqrt = half the relative error), U for S / 64 + eps (one fused or two
         separate roundings: U on m is U / 2 .. U on r), 2 U for sqrt (correctly rounded: U / 2) and the division (U / 2),
         taken as one ulp each;
  dy     |nw_c| r e_c + |y_c| (rel_r + 2 U)          (two multiplies);
  dv     |1 + sc_c| dy + 3 U (|y_c (1 + sc_c)| + |sh_c|)      (1 + sc, the product, the sum);
  da2    1.1 dv + rel_silu |silu(v)| + FLT_MIN        (|silu'| <= 1.0999; rel_silu below).
silu_h16 on an exact fp32 v: t = v * c with c = -log2(e) rounded (U / 2 relative) and the product rounded (U): exp2's argument is
off by 2 U |t| at most, its value by 2 U |v| relative, plus one ulp (2 U) of v_exp_f32; 1 + e: U, and the relative error of e
enters 1 / (1 + e) with the weight e / (1 + e) = 1 - sigma(v); v_rcp_f32 one ulp (2 U); the final product U:
    rel_silu = U (2 (|v| + 1) (1 - sigma(v)) + 4).
FLT_MIN covers results below the normal range (exp2 overflows to inf for v < -88: the kernel gives -0 where silu is ~1e-38).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-6
FLT_MIN = 2.0 ** -126
SECOND = 1.001
COUT = 64

# (Cin, S, N, per_image): Z = 2, Cout = 64.  Cin 37 leaves pad channels in the last block; S = 16 is the smallest plane that is one
# 128-voxel tile, S = 32 has several tiles per plane; per_image 2 with N = 4 makes the modulation row differ within a launch
CASES = [(8, 16, 1, 1), (37, 16, 1, 1), (96, 16, 3, 1), (96, 16, 4, 2), (96, 32, 1, 1), (96, 32, 2, 1), (96, 32, 2, 2)]


def case_id(c):
    return "Cin%d-S%d-N%d-pi%d" % c


def make(case, kind):
    """kind "float": normal x, w / sqrt(27 Cin), normal b.  kind "int": small-integer x and w, ZERO bias: every conv sum is exact
    in fp32, whatever its association.  norm_w, scale, shift are random floats either way."""
    Cin, S, N, per_image = case
    g = torch.Generator().manual_seed(1000 + Cin * 7 + S * 3 + N * 11 + per_image)
    nimg = (N + per_image - 1) // per_image
    if kind == "int":
        x = torch.randint(-3, 4, (N, Cin, 2, S, S), generator=g).float()
        w = torch.randint(-2, 3, (COUT, Cin, 3, 3, 3), generator=g).float()
        b = torch.zeros(COUT)
    else:
        x = torch.randn((N, Cin, 2, S, S), generator=g)
        w = torch.randn((COUT, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5
        b = torch.randn((COUT,), generator=g)
    nw = 1.0 + 0.25 * torch.randn((COUT,), generator=g)
    sc = 0.5 * torch.randn((nimg, COUT), generator=g)
    sh = 0.5 * torch.randn((nimg, COUT), generator=g)
    return {"case": case, "x": x, "w": w, "b": b, "nw": nw, "sc": sc, "sh": sh, "per_image": per_image}


def _rows(t, N, per_image):
    """[nimg, C] modulation rows -> [N, C, 1, 1, 1] (patch n uses row n // per_image)"""
    idx = torch.arange(N) // per_image
    return t[idx].view(N, -1, 1, 1, 1)


def mid_section(h, c, dtype=torch.float64, wrong=None):
    """norm -> modulate -> SiLU of h [N, 64, 2, S, S] in `dtype`, the kernel's order of operations (exact sigmoid)."""
    N = h.shape[0]
    h = h.to(dtype)
    hs = h
    if wrong == "drop_lane_group":               # the sum of squares without the partner lane's quads (channels 8 g + 4 .. 8 g + 7)
        keep = (torch.arange(COUT) % 8) < 4
        hs = h * keep.view(1, -1, 1, 1, 1).to(dtype)
    m = (hs * hs).sum(1, keepdim=True) * (1.0 / COUT) + EPS
    r = 1.0 / m.sqrt()
    y = c["nw"].to(dtype).view(1, -1, 1, 1, 1) * (h * r)
    pi = c["per_image"]
    sc, sh = c["sc"], c["sh"]
    if wrong == "wrong_image_row":               # every patch takes the NEXT image's row
        sc, sh = sc.roll(-1, 0), sh.roll(-1, 0)
    v = y * (1.0 + _rows(sc, N, pi).to(dtype)) + _rows(sh, N, pi).to(dtype)
    return v * torch.sigmoid(v)


def conv64(c):
    return F.conv3d(c["x"].double(), c["w"].double(), c["b"].double(), padding=1)


def reference(c, wrong=None):
    return mid_section(conv64(c), c, torch.float64, wrong)


def conv_bound(c):
    """(L + 4) U mag: tests/test_gpu_conv_zpair.py::_bound without a residual."""
    x, w, b = c["x"], c["w"], c["b"]
    Cin = x.shape[1]
    L = (Cin + 7) // 8 * 8 * 9 + 1
    xa, wa = x.double().abs(), w.double().abs()
    x0, x1 = xa[:, :, 0], xa[:, :, 1]
    w0, w1, w2 = wa[:, :, 0], wa[:, :, 1], wa[:, :, 2]
    p1 = F.conv2d(x0 + x1, w1, padding=1)
    m0 = p1 + F.conv2d(x1, w2 + w1, padding=1)
    m1 = p1 + F.conv2d(x0, w0 + w1, padding=1)
    mag = torch.stack([m0, m1], dim=2) + b.double().abs().view(1, -1, 1, 1, 1)
    return (L + 4) * U * mag


def bound(c, e_conv=None):
    """The module docstring's da2, float64.  e_conv: the conv's own error bound (None: conv_bound; 0 where the sums are exact)."""
    h = conv64(c)
    N = h.shape[0]
    e = conv_bound(c) if e_conv is None else torch.as_tensor(e_conv, dtype=torch.float64).expand_as(h)
    S = (h * h).sum(1, keepdim=True)
    dS = (2.0 * h.abs() * e + e * e).sum(1, keepdim=True) + 12.0 * U * S
    m = S / COUT + EPS
    r = 1.0 / m.sqrt()
    rel_r = (dS / COUT) / (2.0 * m) + 3.0 * U
    nw = c["nw"].double().view(1, -1, 1, 1, 1)
    y = nw * (h * r)
    dy = nw.abs() * r * e + y.abs() * (rel_r + 2.0 * U)
    sc1 = 1.0 + _rows(c["sc"], N, c["per_image"]).double()
    sh = _rows(c["sh"], N, c["per_image"]).double()
    v = y * sc1 + sh
    dv = sc1.abs() * dy + 3.0 * U * ((y * sc1).abs() + sh.abs())
    sg = torch.sigmoid(v)
    rel_silu = U * (2.0 * (v.abs() + 1.0) * (1.0 - sg) + 4.0)
    return SECOND * (1.1 * dv + rel_silu * (v * sg).abs()) + FLT_MIN


def emulate_f32(c):
    """The whole operation in float32 on the CPU: F.conv3d in float32 (its own association: inside conv_bound like any other
    fp32 order of these sums), then the mid-section step by step in float32 with silu_h16's exp2 form."""
    h = F.conv3d(c["x"], c["w"], c["b"], padding=1)
    N = h.shape[0]
    m = (h * h).sum(1, keepdim=True) * np.float32(1.0 / COUT) + np.float32(EPS)
    r = 1.0 / m.sqrt()
    y = c["nw"].view(1, -1, 1, 1, 1) * (h * r)
    v = y * (1.0 + _rows(c["sc"], N, c["per_image"])) + _rows(c["sh"], N, c["per_image"])
    e = torch.exp2(v * np.float32(-1.4426950408889634))
    return v * (1.0 / (1.0 + e))


def worst(d, bnd):
    return float((d / bnd).max())
