"""Cases, float64 model and bounds of the timestep-embedding kernels on their own (tm_kernels.hip time_embed_kernel,
emb_all_kernel; hooks tm_op_time_embed / tm_op_emb_all).  Shared by tests/test_embed_cases_host.py (no GPU) and
tests/test_gpu_embed.py.

TIME_EMBED, one workgroup of 256 threads per image; the strided loops make more than one trip at ch = 320 and at E = 512, 1024:
    fr_k  = expf(-logf(10000.f) * (float)k / (float)half)      k = i mod half, half = ch / 2
    sinu  = cosf(t fr_k) (i < half) | sinf(t fr_k)
    hid_o = silu_f(b1_o + sum_k w1_ok sinu_k)                  one fmaf per k, ascending, from b1
    te_o  = b2_o + sum_k w2_ok hid_k, te_act = silu_f(te)      silu_f(x) = x / (1 + expf(-x)), an IEEE division
The model below is the same chain in float64 with exact functions; the bound follows every rounding point, first order in
U = 2^-24 (an ulp is 2 U relative):
  q = -ln(1e4) k / half: the device logf is taken as 2 ulp (4 U), the product and the quotient round once each: 6 U |q|, which exp
      turns into a relative error of fr; expf itself is train_op_ref.exp_rel_bound(q) = 2 U |q| + 4 U:   e_fr = 8 U |q| + 4 U.
  arg = fl(t fr) is off by |t fr| (e_fr + U): an error in the argument is amplified by the argument, up to 999 here.  sinf / cosf
      are taken as 2 ulp of their result (4 U |sinu|), the assumption the project writes into exp_rel_bound for expf:
      d_sinu = |t fr| (e_fr + U) + 4 U |sinu|.
  THE 2-ULP FIGURES ARE ASSUMPTIONS, NOT MEASUREMENTS.  The "probe" weights (w1 selects one sinusoid per output, b1 = 0, w2 the
      identity) leave d_sinu as nearly the whole bound; a worst ratio above 1 there is a finding about the device functions.
  Linear: d_pre = sum_k |w1| d_sinu + L U (|b| + sum_k |w| |v|), L the chain's fmafs with a non-zero weight (fmaf(0, v, acc) is acc,
      exactly); silu_f: |silu'| <= 1.1, relative error
      (2 U |x| + 4 U) e / (1 + e) + 2 U, e = exp(-x) (expf, the rounded 1 + e, the division).
EMB_ALL, one wave per output row e, lane l holds w[e][j 64 + l], j < per = E / 64:
    ss[i][e] = wave_sum(chain of per fmafs from 0.f) + ball[e]; bound (per + 6 + 1) U mag: the lane's chain, six butterfly
    additions, the bias add; mag on absolute values.  Integer operands (|w| <= 2, |te_act| <= 3, |b| <= 4: sums below 2^24) must
    come back bit for bit.  tot = 1, 5, 130: the last workgroup runs 1, 1, 2 of its 4 waves.
No constant comes from an observed error.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from test_gpu_prep_wide import _fma

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
T_VALUES = (0, 1, 137, 999)

# (ch, E, b, kind): b = 1 takes t = 999, b = 3 takes 0, 1, 137
TE_CASES = [(ch, E, b, kind) for ch, E in ((64, 256), (128, 512), (320, 1024)) for b in (1, 3) for kind in ("rand", "probe")]
TE_WRONG = ["cos_sin_swapped", "half_is_ch", "no_hidden_silu"]
# (E, tot, b, kind)
EA_CASES = [(E, tot, b, "int") for E in (64, 256, 1024) for tot in (1, 5, 130) for b in (1, 3)] + \
           [(1024, 130, 3, "rand"), (256, 5, 3, "rand"), (64, 130, 1, "rand")]
EA_WRONG = ["row_stride_E", "bias_per_lane", "lane_major"]


def te_id(c):
    return "te-ch%d-E%d-b%d-%s" % c


def ea_id(c):
    return "ea-E%d-tot%d-b%d-%s" % c


# ---- time_embed ----------------------------------------------------------------------------------------------------------------
def te_make(c):
    ch, E, b, kind = c
    g = torch.Generator().manual_seed(900 + ch + 3 * E + 7 * b + (1 if kind == "probe" else 0))
    t = torch.tensor([999] if b == 1 else [0, 1, 137], dtype=torch.int64)
    if kind == "probe":
        w1 = torch.zeros((E, ch))
        w1[torch.arange(E), torch.arange(E) % ch] = 1.0
        b1, w2, b2 = torch.zeros(E), torch.eye(E), torch.zeros(E)
    else:
        w1, b1 = torch.randn((E, ch), generator=g) / ch ** 0.5, torch.randn((E,), generator=g) * 0.2
        w2, b2 = torch.randn((E, E), generator=g) / E ** 0.5, torch.randn((E,), generator=g) * 0.2
    return t, w1, b1, w2, b2


def _silu_f_rel(x):
    e = torch.exp(-x)
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (1.0 + e))
    return (2 * U * x.abs() + 4 * U) * frac + 2 * U


def _fmafs(w):
    """the fmafs of a row's chain that can round: a zero weight leaves the accumulator as it is"""
    return (w != 0).sum(1).double()[None, :]


def te_reference(c, t, w1, b1, w2, b2, wrong=None):
    """((te, te_act), (bound_te, bound_te_act)) float64 [b, E]"""
    ch, E, b, kind = c
    half = ch // 2
    k = torch.arange(ch, dtype=torch.float64) % half
    q = -math.log(10000.0) * k / (ch if wrong == "half_is_ch" else half)
    arg = t.double()[:, None] * torch.exp(q)[None, :]
    first = torch.arange(ch)[None, :] < half
    if wrong == "cos_sin_swapped":
        first = ~first
    sinu = torch.where(first, torch.cos(arg), torch.sin(arg))
    e_fr = 8 * U * q.abs() + 4 * U
    d_sinu = arg.abs() * (e_fr + U)[None, :] + 4 * U * sinu.abs()
    w1d, w2d = w1.double(), w2.double()
    pre = b1.double() + sinu @ w1d.T
    d_pre = d_sinu @ w1d.abs().T + _fmafs(w1) * U * (b1.double().abs() + sinu.abs() @ w1d.abs().T)
    hid = pre if wrong == "no_hidden_silu" else F.silu(pre)
    d_hid = 1.1 * d_pre + _silu_f_rel(pre) * hid.abs()
    te = b2.double() + hid @ w2d.T
    d_te = d_hid @ w2d.abs().T + _fmafs(w2) * U * (b2.double().abs() + hid.abs() @ w2d.abs().T) + FLT_MIN
    act = F.silu(te)
    d_act = 1.1 * d_te + _silu_f_rel(te) * act.abs() + FLT_MIN
    return (te, act), (d_te, d_act)


def _chain(w, v, b):
    """acc = b; acc = fma(w[:, k], v[:, k], acc), k ascending: float32, [b, E]"""
    acc = b[None, :].expand(v.shape[0], -1).contiguous()
    for k in range(w.shape[1]):
        acc = _fma(w[None, :, k], v[:, k, None], acc)
    return acc


def te_emulate_f32(c, t, w1, b1, w2, b2):
    """the kernel's chain in float32 (numpy's float32 functions for logf / expf / cosf / sinf)"""
    ch, E, b, kind = c
    half = ch // 2
    k = (np.arange(ch) % half).astype(np.float32)
    fr = np.exp(-np.log(np.float32(10000.0)) * k / np.float32(half))
    assert fr.dtype == np.float32
    arg = t.numpy().astype(np.float32)[:, None] * fr[None, :]
    sinu = torch.from_numpy(np.where(np.arange(ch)[None, :] < half, np.cos(arg), np.sin(arg)).astype(np.float32))
    silu_f = lambda x: x / (1.0 + torch.exp(-x))
    hid = silu_f(_chain(w1, sinu, b1))
    te = _chain(w2, hid, b2)
    return te, silu_f(te)


# ---- emb_all -------------------------------------------------------------------------------------------------------------------
def ea_make(c):
    E, tot, b, kind = c
    g = torch.Generator().manual_seed(1700 + E + 11 * tot + 5 * b)
    if kind == "int":
        return (torch.randint(-3, 4, (b, E), generator=g).float(), torch.randint(-2, 3, (tot, E), generator=g).float(),
                torch.randint(-4, 5, (tot,), generator=g).float())
    return torch.randn((b, E), generator=g), torch.randn((tot, E), generator=g) / E ** 0.5, torch.randn((tot,), generator=g)


def ea_reference(c, te_act, wall, ball, wrong=None):
    """(ss, bound) float64 [b, tot]"""
    E, tot, b, kind = c
    per = E // 64
    x, w, bias = te_act.double(), wall.double(), ball.double()
    if wrong == "lane_major":                          # te_act[j 64 + l] read as te_act[l per + j]
        x = x.reshape(b, 64, per).transpose(1, 2).reshape(b, E)
    ss = x @ w.T + (64 * bias if wrong == "bias_per_lane" else bias)
    if wrong == "row_stride_E":                        # ss[i][e] written at i E + e of the [b][tot] buffer
        flat = torch.full((max(b * tot, (b - 1) * E + tot),), float("nan"), dtype=torch.float64)
        for i in range(b):
            flat[i * E:i * E + tot] = ss[i]
        ss = flat[:b * tot].reshape(b, tot)
    bound = torch.zeros_like(ss) if kind == "int" else (per + 6 + 1) * U * (x.abs() @ w.abs().T + bias.abs()) + FLT_MIN
    return ss, bound


def ea_emulate_f32(c, te_act, wall, ball):
    """lane chains of per fmafs from 0.f, the xor butterfly (offsets 32 .. 1), + bias: float32"""
    E, tot, b, kind = c
    per = E // 64
    acc = torch.zeros((b, tot, 64))
    for j in range(per):
        acc = _fma(wall[None, :, j * 64:(j + 1) * 64], te_act[:, None, j * 64:(j + 1) * 64], acc)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    return acc[:, :, 0] + ball[None, :]
