"""Float64 references of the training-slice operators (include/teramind_hip.h, tera-mind_amd/csrc/tm_train.hip) and the fp32
error bounds the op-level tests hold the HIP kernels to.  Pure torch on the CPU, shared by tests/test_gpu_train_ops.py; the
closed-form backward passes are checked against torch.autograd in tests/test_train_op_ref.py.

Bounds are first-order: U = 2^-24 is the fp32 unit roundoff, a sum of terms that passes through at most L fp32 additions
(fixed order) is off by at most L * U * (sum of |terms|), and every other rounding adds U relative to its own result."""
import math

import torch

from oracle import teramind_cpu as tc

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
EPS = 1e-6                      # TM_EPS (tm_device.h) = the oracle's EPS

KB, KK = 0.7978845608028654, 0.044715     # tanh-GELU constants


def depth_wave(D):
    """Additions a value of a row sum passes through in a wave-per-row reduction: D / 64 per lane, then 6 shuffle levels."""
    return (D + 63) // 64 + 6


def depth_two_stage(n_wg):
    """prep_bwd_reduce_dw_kernel: eight chains over the workgroup partials, then three levels; plus the 64-lane wave_sum."""
    return (n_wg + 7) // 8 + 3 + 6


# ---- row ops (tm_op_rows) ------------------------------------------------------------------------------------------------
def rms_rows(x, w):
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    return x * r * w, r


def rms_rows_bwd(x, w, g):
    """dL/dx and dL/dw of y = RMSNorm_D(x) * w (rows of x), closed form."""
    y, r = rms_rows(x, w)
    xh = x * r
    dot = (g * w * xh).mean(-1, keepdim=True)
    return r * (g * w - xh * dot), (g * xh).reshape(-1, x.shape[-1]).sum(0)


def softmax_bwd(p, g):
    return p * (g - (g * p).sum(-1, keepdim=True))


# ---- elementwise (tm_op_ew) ----------------------------------------------------------------------------------------------
def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(KB * (x + KK * x ** 3)))


def gelu_tanh_grad(x):
    th = torch.tanh(KB * (x + KK * x ** 3))
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * KB * (1.0 + 3.0 * KK * x * x)


def silu(x):
    return tc.silu(x)


def silu_grad(x):
    sg = torch.sigmoid(x)
    return sg * (1.0 + x * (1.0 - sg))


# ---- per-voxel modulate(norm) (tm_op_modnorm / _bwd) and the ResBlock prep (tm_op_prep_train / _bwd) on NCDHW -----------
def modnorm(x, w, scale, shift):
    return tc.rms_norm_channels(x, w) * (1.0 + scale) + shift


def prep_train(x, w, scale, shift, per_image, mask=None, p=0.0):
    """Dropout(SiLU(RMSNorm_C(x) w (1 + scale[img]) + shift[img])), scale / shift [images][C] or None.  Returns (y, m), m the
    pre-activation."""
    m = tc.rms_norm_channels(x, w)
    if scale is not None:
        img = torch.arange(x.shape[0]) // per_image
        m = m * (1.0 + scale[img][:, :, None, None, None]) + shift[img][:, :, None, None, None]
    y = silu(m)
    if mask is not None:
        y = y * mask / (1.0 - p)
    return y, m


# ---- windowed attention core (tm_op_window_attn_train) -------------------------------------------------------------------
def to_windows(t, Z, S):
    """NCDHW [N, C, Z, S, S] -> [N, 4, Z (S/2)^2, C]: the 2 x 2 (h, w) windows over all z, tokens (z, h, w) in window order
    (oracle windowed_cross_attention's to_win with n_h = 2)."""
    N, C = t.shape[:2]
    h = S // 2
    t = t.permute(0, 2, 3, 4, 1).reshape(N, Z, 2, h, 2, h, C).permute(0, 2, 4, 1, 3, 5, 6)
    return t.reshape(N, 4, Z * h * h, C)


def from_windows(t, Z, S):
    N, C = t.shape[0], t.shape[-1]
    h = S // 2
    t = t.reshape(N, 2, 2, Z, h, h, C).permute(0, 6, 3, 1, 4, 2, 5)
    return t.reshape(N, C, Z, S, S)


def window_attn(q, k, v, qw, kw, Z, S):
    """o = softmax(qh kh^T / C) v per window, qh / kh = RMSNorm_C(q / k) * qw / kw; NCDHW in and out."""
    C = q.shape[1]
    qh = tc.rms_norm_last(to_windows(q, Z, S), qw)
    kh = tc.rms_norm_last(to_windows(k, Z, S), kw)
    p = torch.softmax(qh @ kh.transpose(-2, -1) / C, dim=-1)
    return from_windows(p @ to_windows(v, Z, S), Z, S)


def window_attn_mag(q, k, v, qw, kw, dout, Z, S):
    """Magnitudes for the error bounds: the same computation with every sum taken over |terms| (float64, NCDHW outputs
    o, dq, dk, dv and [C] dqw, dkw), and the largest |logit| bound factor sum_c |qh kh| / C per window."""
    C = q.shape[1]
    W = lambda t: to_windows(t, Z, S)
    qs, ks, vs, ds = W(q), W(k), W(v), W(dout)
    rq = torch.rsqrt(qs.pow(2).mean(-1, keepdim=True) + EPS)
    rk = torch.rsqrt(ks.pow(2).mean(-1, keepdim=True) + EPS)
    qh, kh = qs * rq * qw, ks * rk * kw
    p = torch.softmax(qh @ kh.transpose(-2, -1) / C, dim=-1)
    lmag = qh.abs() @ kh.abs().transpose(-2, -1) / C
    o = p @ vs.abs()
    dv = p.transpose(-2, -1) @ ds.abs()
    dp = ds.abs() @ vs.abs().transpose(-2, -1)
    rowdot = (dp * p).sum(-1, keepdim=True)
    dS = p * (dp + rowdot) / C
    dqh = dS @ kh.abs()
    dkh = dS.transpose(-2, -1) @ qh.abs()

    def rms_bwd_mag(x, r, w, dxh):
        gw = dxh * w.abs()
        dot = (gw * x.abs() * r).mean(-1, keepdim=True)
        return r * gw + x.abs() * r * dot, (dxh * x.abs() * r).reshape(-1, C).sum(0)
    dq, dqw = rms_bwd_mag(qs, rq, qw, dqh)
    dk, dkw = rms_bwd_mag(ks, rk, kw, dkh)
    F = lambda t: from_windows(t, Z, S)
    return dict(o=F(o), dq=F(dq), dk=F(dk), dv=F(dv), dqw=dqw, dkw=dkw), float(lmag.max())


# ---- optimizer (tm_op_sumsq / tm_op_adam) --------------------------------------------------------------------------------
def adam(p, g, m, v, lr, b1, b2, eps, wd, step, gscale):
    """torch.optim.Adam._single_tensor_adam (amsgrad off) with the gradient scaled first; float64 in, float64 out.
    b1 / b2 / eps / lr / wd / gscale are taken at their float32 values (the C ABI's type)."""
    f = lambda a: float(torch.tensor(a, dtype=torch.float32))
    lr, b1, b2, eps, wd, gscale = map(f, (lr, b1, b2, eps, wd, gscale))
    g2 = g * gscale + wd * p
    m2 = m + (g2 - m) * (1.0 - b1)
    v2 = b2 * v + (1.0 - b2) * g2 * g2
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    upd = (lr / bc1) * (m2 / (torch.sqrt(v2) / math.sqrt(bc2) + eps))
    return p - upd, m2, v2, g2, upd


def exp_rel_bound(t):
    """Relative error bound of the device expf(t): the weaker of a 2-ulp exp (4 U) and an exp2 of the rounded product
    t log2 e (two roundings, 2 U |t| after exp2) with a 2-ulp exp2: 2 U |t| + 4 U."""
    return 2 * U * t.abs() + 4 * U


# ---- the hardware SiLU of prep_kernel ------------------------------------------------------------------------------------
def silu_hw_rel_bound(m):
    """Relative error bound of silu_h16 (tm_device.h): x * v_rcp(1 + v_exp(x * -log2 e)), v_exp_f32 and v_rcp_f32 1 ulp
    (2U) each.  The exponent t = fl(x * fl(-log2 e)) carries two roundings, 2U |t|, which exp2 turns into 2U |t| ln 2 = 2U |x|
    relative in e; 1 + e rounds once (U) and passes on e / (1 + e) of e's error; then the reciprocal (2U) and the product (U):
        rel <= (2U |x| + 2U) e / (1 + e) + U + 2U + U."""
    e = torch.exp(-m)
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (1.0 + e))
    return (2 * U * m.abs() + 2 * U) * frac + 4 * U
