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


# ---- inference attention cores (tm_op_window_attn_kv: tm_attn.hip window_attn_*, tm_conv_bf16.hip window_attn_bf16 / _long) --
# 16-bit type -> (torch dtype, smallest normal number)
H16 = {"bf16": (torch.bfloat16, 2.0 ** -126), "f16": (torch.float16, 2.0 ** -14)}
ATTN_WRONG = ("scale", "drop_key", "swap_v", "kw_is_qw", "hwz", "kv_mod")      # the deliberate errors of window_attn_fwd


def r16(t, dt):
    """Round to the nearest value of the 16-bit type (ties to even), returned as float64."""
    return t.to(H16[dt][0]).double()


def kv_full(t, S, mod=False):
    """Half-resolution k / v [N, C, Z, S/2, S/2] -> what query token (z, y, x) reads: entry (z, y >> 1, x >> 1).
    mod: the wrong read (y, x) mod S/2."""
    i = torch.arange(S) % t.shape[-1] if mod else torch.arange(S) >> 1
    return t[:, :, :, i][:, :, :, :, i]


def to_windows_hwz(t, Z, S):
    """to_windows with the tokens of a window ordered (h, w, z): the wrong partition."""
    N, C = t.shape[:2]
    h = S // 2
    t = t.permute(0, 2, 3, 4, 1).reshape(N, Z, 2, h, 2, h, C).permute(0, 2, 4, 3, 5, 1, 6)
    return t.reshape(N, 4, Z * h * h, C)


def window_attn_fwd(q, kv, qw, kw, Z, S, dt=None, kv_half=False, wrong=None, mag=False):
    """The inference attention core as the kernels compute it, in float64, and the bound a kernel's result must meet.

    q [N, C, Z, S, S], kv [N, 2C, Z, Sc, Sc] (k = channels [0, C), v = [C, 2C); Sc = S / 2 with kv_half) float64 NCDHW;
    qw, kw fp32 [C].  dt None: the fp32 kernels, no rounding in the model.  dt "bf16" / "f16": the 16-bit kernels, with their
    roundings where they place them:
      * q, k, v are rounded to the type on entry (the q / kv Linears emit them so);
      * the Q operand is round16(fl32(q * fl32(q_norm.w * k_norm.w))), K is used as it is;
      * both rstd factors and 1 / C multiply the fp32 logits; the softmax is fp32;
      * P is rounded to the type, P.V accumulates in fp32 and the output is rounded once.
    Returns (o, bound), NCDHW float64: |kernel - o| <= bound element by element.  mag: also the magnitude companion, a dict
    of the same sums over |terms| (lmag [N, 4, T, T] for the logits l, omag NCDHW for the output before its rounding).

    Derivation, first order in U = 2^-24 (the matrix unit's adder is taken as 2 U per addition, not round to nearest):
      logit: a C-term sum (2 C U of its magnitude), two rstd factors ((C + 5) U each: C-term sum of squares, mean, + eps,
        sqrt and reciprocal, halved by the square root) and at most 10 single roundings (q_norm.w k_norm.w, its product with
        the operand, 1 / C, the three scale products): |dl| <= (4 C + 20) U lmag, lmag = sum_c |Q K| rq rk / C.  16-bit
        operands below the smallest normal number may be flushed by the matrix unit: their terms are added to |dl| whole.
      e = exp(l - m): |dl| from the logit, U |l - m| from the subtraction, exp_rel_bound(l - m) from the device expf.
      p = e / sum: e's error, the p-weighted mean of all e errors of the row (the sum), T additions, the reciprocal and its
        product (3 U).  The two-pass long-window kernels walk the keys in T / 128 blocks and rescale the running sum by
        exp(m_old - m_new) per block: 3 U span + 7 U more per block, span = max |l - m| of the row, which also replaces
        |l - m| there (pass 1 subtracts the running maximum, not the final one).
      fp32: o = sum_u p v over T terms: sum_u |dp| |v| + (2 T + 2) U sum_u p |v|.
      16-bit: rounding is monotone, so the kernel's P lies between round16(p (1 - e_p)) and round16(p (1 + e_p)): dP is the
        larger distance to round16(p) (zero wherever the interval holds no rounding boundary; down to 0 where P is below the
        smallest normal number).  The fp32 output before its rounding is then within b = sum_u dP |v| + (2 T + 2) U sum_u P |v|
        (+ the terms of flushed v), and the stored value between round16(o - b) and round16(o + b); b is widened by 2 U |o|
        for the fp32 value the accumulator holds and the float64 -> float32 -> 16-bit path of the conversion used here.
    wrong: one of ATTN_WRONG, a deliberately wrong variant (tests/test_window_attn_ref.py shows the bound rejects each)."""
    assert wrong is None or wrong in ATTN_WRONG
    C = q.shape[1]
    T = Z * (S // 2) ** 2
    k, v = kv[:, :C], kv[:, C:]
    if dt:
        q, k, v = r16(q, dt), r16(k, dt), r16(v, dt)
    if kv_half:
        k, v = kv_full(k, S, wrong == "kv_mod"), kv_full(v, S, wrong == "kv_mod")
    qs = (to_windows_hwz if wrong == "hwz" else to_windows)(q, Z, S)
    ks, vs = to_windows(k, Z, S), to_windows(v, Z, S)
    rq = torch.rsqrt(qs.pow(2).mean(-1, keepdim=True) + EPS)
    rk = torch.rsqrt(ks.pow(2).mean(-1, keepdim=True) + EPS).transpose(-2, -1)
    kw_used = qw if wrong == "kw_is_qw" else kw
    if dt:
        w2 = qw.float() * kw_used.float()                              # fp32, as the kernel forms it
        qf = (qs.float() * w2).to(H16[dt][0]).double()
    else:
        qf = qs * (qw.double() * kw_used.double())
    scale = C ** -0.5 if wrong == "scale" else 1.0 / C
    fac = rq * rk * scale
    l = (qf @ ks.transpose(-2, -1)) * fac
    lmag = (qf.abs() @ ks.abs().transpose(-2, -1)) * fac
    dl = (4 * C + 20) * U * lmag
    if dt:
        tiny = H16[dt][1]
        sub = lambda t: t.abs() * (t.abs() < tiny)
        dl = dl + (sub(qf) @ ks.abs().transpose(-2, -1) + qf.abs() @ sub(ks).transpose(-2, -1)) * fac
    if wrong == "drop_key" and T > 1:
        l = l.clone()
        l[..., T - 1] = -math.inf
    p = torch.softmax(l, dim=-1)
    t = (l - l.max(-1, keepdim=True).values).abs()
    t = torch.where(torch.isinf(t), torch.zeros_like(t), t)
    kbn = T // 128 if T in (256, 512) else 0
    if kbn:
        t = t.max(-1, keepdim=True).values.expand_as(t)
    e_e = dl + U * t + exp_rel_bound(t)
    e_p = e_e + (p * e_e).sum(-1, keepdim=True) + (T + 3) * U + kbn * (3 * U * t + 7 * U)
    e_p = e_p / (1.0 - e_p).clamp_min(0.5)                            # the product of the (1 + e) factors, not only their sum
    if wrong == "swap_v" and T > 1:
        vs = vs.clone()
        vs[:, :, [0, T - 1]] = vs[:, :, [T - 1, 0]]       # first and last token: distinct k / v entries at half resolution too
    if not dt:
        o = p @ vs
        omag = p @ vs.abs()
        b = (p * e_p) @ vs.abs() + (2 * T + 2) * U * omag + FLT_MIN
        res = (from_windows(o, Z, S), from_windows(b, Z, S))
        return res + (dict(l=l, lmag=lmag, omag=from_windows(omag, Z, S)),) if mag else res
    p16, lo, hi = r16(p, dt), r16(p * (1.0 - e_p), dt), r16(p * (1.0 + e_p), dt)
    lo = torch.where(hi < tiny, torch.zeros_like(lo), lo)
    dp = torch.maximum(hi - p16, p16 - lo)
    o = p16 @ vs
    omag = p16 @ vs.abs()
    b = dp @ vs.abs() + (2 * T + 2) * U * omag + p16 @ sub(vs)
    o16, olo, ohi = r16(o, dt), r16(o - b - 2 * U * o.abs(), dt), r16(o + b + 2 * U * o.abs(), dt)
    bound = torch.maximum(ohi - o16, o16 - olo)
    res = (from_windows(o16, Z, S), from_windows(bound, Z, S))
    return res + (dict(l=l, lmag=lmag, omag=from_windows(omag, Z, S)),) if mag else res


def attn_inputs(N, C, Z, S, kv_half=False, kind="plain", seed=0):
    """fp32 q [N, C, Z, S, S], kv [N, 2C, Z, Sc, Sc], qw, kw [C] of an attention-core case.  k is correlated with the q of the
    voxel it is read for, so the softmax is far from uniform.  kind "sharp": q_norm.weight times 60, the logits span several
    tens and the softmax is close to one-hot (q w2 stays below 2000, inside f16).  kind "zeros": the first row of q, the first
    column of k / v and the whole last patch of k / v are zero: rms(0) = 0 * rsqrt(1e-6) = 0, those rows get a uniform
    softmax (the zero half-patch borders of a sweep)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + 3 * S + Z + (50 if kv_half else 0))
    Sc = S // 2 if kv_half else S
    q = torch.randn((N, C, Z, S, S), generator=g) * 1.5
    k = torch.randn((N, C, Z, Sc, Sc), generator=g) * 2.1 + 0.5 * (q[..., ::2, ::2] if kv_half else q)
    v = torch.randn((N, C, Z, Sc, Sc), generator=g)
    qw, kw = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    kv = torch.cat([k, v], 1)
    if kind == "sharp":
        qw = qw * 60.0
    if kind == "zeros":
        q[:, :, :, 0, :] = 0.0
        kv[:, :, :, :, 0] = 0.0
        kv[N - 1] = 0.0
    return q, kv, qw, kw


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
