"""Cases, inputs, error bounds and a float32 emulation of the short-window training attention core (tm_op_window_attn_train at
windows of 4 / 8 / 16 tokens: attn_short_kernel in csrc/tm_train.hip), shared by tests/test_gpu_window_attn_train_short.py
(which holds the kernel to the bounds) and tests/test_window_attn_train_short_ref.py (which shows that the bounds reject wrong
variants); and the case tables of the fixtures tools/make_train_short_golden.py mints for tests/test_gpu_train_short.py.

The bounds are first order in U = 2^-24 and follow the kernel's accumulation orders as its header comment states them (VALU
fmaf chains: U per addition; v_rsq_f32 and v_rcp_f32 are 1 ulp = 2 U).  With T the window, NB = 64 / T the lanes of a token,
Cb = ceil(C / 8), Lr = 8 ceil(Cb / NB) + log2(NB) the additions of a per-token channel sum, lmax = the largest
sum_c |qh kh| / C of the case and mag = train_op_ref.window_attn_mag (every sum over |terms|):

  r      = rsq(ss / C + eps): the squares (U), the Lr-addition sum, the factor 1 / C (U) and its fused product-sum (U), eps as a
         float (U), rsq (2 U); the square root halves the first four, which is not claimed: e_r = (Lr + 6) U.
  logit  s = (sum_c qh kh) / C, qh = (q r) qw: operands (e_r + 2 U) each, a C-term chain (C U), 1 / C and its product (2 U):
         |ds| <= (C + 2 Lr + 18) U lmax = dl.
  P      = expf(s - m) * rcp(l), m the maximum of the computed logits (a shift common to a row cancels, its rounding does not):
         2 dl from the logits of the row, the subtraction (U |s - m|) and train_op_ref.exp_rel_bound (2 U |s - m| + 4 U) with
         |s - m| <= 2 lmax, once for the element and once more for the row sum it is divided by; the row sum's T terms; the
         reciprocal (2 U) and two products:  e_P = 2 dl + (12 lmax + T + 12) U.
  o, dv  a T-term chain of P times data:  (e_P + (T + 1) U) mag.
  dP     = do . v, a C-term chain: C U.  D = rowsum(dP o P): the products and a T-term chain: e_P + (C + T + 1) U of sum_j P |dP|.
  dS     = P (dP - D) / C:  2 e_P + (C + T + 5) U of P (|dP| + sum P |dP|) / C, which is mag's dS.
  dqh    = dS kh (dkh = dS^T qh), a T-term chain of dS times operands that carry e_r + 2 U:  e_dS + (Lr + T + 8) U.
  dq     = r dqh qw - q r^3 md, md = (sum_c dqh qw q) / C: the factor r and two products (e_r + 2 U) on the first term; on the
         second r^3 (3 e_r + 2 U), the dot's products, its Lr additions and 1 / C (Lr + 4) U, two products and the subtraction
         (3 U):  E = e_dqh + (4 Lr + 27) U = 2 e_P + (C + 2 T + 5 Lr + 40) U  of mag dq / dk.
  dqw    = sum over tokens of dqh q r: the products (e_r + 2 U), log2(T) butterfly levels inside the window, then the 4 N window
         partials through prep_bwd_reduce_dw_kernel (eight chains, three levels):
         Ew = e_dqh + (Lr + 8 + log2(T) + ceil(4 N / 8) + 3) U  of mag dqw / dkw.
"""
import math

import torch

import train_op_ref as R
from train_cases import ATTN_SHAPES, make_inputs
from train_long_cases import KINDS  # noqa: F401  (plain, sharp = near one-hot, zeros = zero rows)

U = R.U

# (N, C, Z, S): T = Z (S/2)^2 = 4 (C off the CB8 block and two patches; the widest C), 8 (from two planes, and from eight planes of
# one token each), 16 (one plane of S = 8: the rna_slc 1 middle block; four planes of S = 4 at the widest C)
SHORT_CASES = [(2, 13, 1, 4), (1, 512, 1, 4), (1, 64, 2, 4), (2, 40, 8, 2), (1, 128, 1, 8), (1, 512, 4, 4)]
WRONG = ("scale", "drop_key", "no_rowdot", "hwz", "swap_window")
OUTPUTS = ("o", "dq", "dk", "dv", "dqw", "dkw")


def inputs(N, C, Z, S, kind):
    """fp32 q, k, v, qw, kw of train_op_ref.attn_inputs in `kind`, and a seeded dout."""
    q, kv, qw, kw = R.attn_inputs(N, C, Z, S, False, kind, seed=17)
    d = torch.randn((N, C, Z, S, S), generator=torch.Generator().manual_seed(31 * C + S + Z))
    return q, kv[:, :C].contiguous(), kv[:, C:].contiguous(), qw, kw, d


def reference(q, k, v, qw, kw, d, Z, S):
    """float64 autograd of train_op_ref.window_attn, and the magnitudes: (dict of the six outputs, mag, lmax)."""
    leaves = [t.double().clone().requires_grad_(True) for t in (q, k, v, qw, kw)]
    o = R.window_attn(*leaves, Z, S)
    o.backward(d.double())
    ref = dict(o=o.detach(), dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad, dqw=leaves[3].grad, dkw=leaves[4].grad)
    mag, lmax = R.window_attn_mag(*(t.double() for t in (q, k, v, qw, kw, d)), Z, S)
    return ref, mag, lmax


def bounds(N, C, Z, S, mag, lmax):
    """Element-wise bounds of the six outputs (module docstring)."""
    T = Z * (S // 2) ** 2
    assert T in (4, 8, 16)
    NB = 64 // T
    Lr = 8 * (((C + 7) // 8 + NB - 1) // NB) + int(math.log2(NB))
    dl = (C + 2 * Lr + 18) * U * lmax
    eP = 2 * dl + (12 * lmax + T + 12) * U
    E = 2 * eP + (C + 2 * T + 5 * Lr + 40) * U
    e_dqh = 2 * eP + (C + T + 5) * U + (Lr + T + 8) * U
    Ew = e_dqh + (Lr + 8 + int(math.log2(T)) + (4 * N + 7) // 8 + 3) * U
    return dict(o=(eP + (T + 1) * U) * mag["o"], dv=(eP + (T + 1) * U) * mag["dv"], dq=E * mag["dq"], dk=E * mag["dk"],
                dqw=Ew * mag["dqw"], dkw=Ew * mag["dkw"])


def emulate_f32(q, k, v, qw, kw, d, Z, S, wrong=None):
    """The core in float32 torch the way the kernel walks it (per window: r by rsqrt, logits times 1 / C, max, exp, sum,
    reciprocal, products; every later product from the stored P and dS), NCDHW in, the six outputs as float64.
    wrong: one of WRONG, a deliberate error."""
    assert wrong is None or wrong in WRONG
    C = q.shape[1]
    T = Z * (S // 2) ** 2
    W = lambda t: R.to_windows(t.float(), Z, S)
    qs, ks, vs, ds = (R.to_windows_hwz(q.float(), Z, S) if wrong == "hwz" else W(q)), W(k), W(v), W(d)
    one_c = torch.tensor(1.0 / C, dtype=torch.float32)
    rq = torch.rsqrt(qs.pow(2).sum(-1, keepdim=True) * one_c + R.EPS)
    rk = torch.rsqrt(ks.pow(2).sum(-1, keepdim=True) * one_c + R.EPS)
    qh, kh = qs * rq * qw, ks * rk * kw
    inv_c = torch.tensor(1.0 / C ** 0.5, dtype=torch.float32) if wrong == "scale" else one_c
    s = (qh @ kh.transpose(-2, -1)) * inv_c
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    if wrong == "drop_key":
        e = e.clone()
        e[..., T - 1] = 0.0
    p = e * (1.0 / e.sum(-1, keepdim=True))
    o = p @ vs
    dv = p.transpose(-2, -1) @ ds
    dp = ds @ vs.transpose(-2, -1)
    D = torch.zeros_like(dp[..., :1]) if wrong == "no_rowdot" else (dp * p).sum(-1, keepdim=True)
    dS = p * (dp - D) * inv_c
    dqh = dS @ kh
    dkh = dS.transpose(-2, -1) @ qh

    def rms_bwd(x, r, w, dxh):
        dot = (dxh * w * x).sum(-1, keepdim=True) * one_c
        return r * dxh * w - x * r * r * r * dot, (dxh * x * r).reshape(-1, C).sum(0)
    dq, dqw = rms_bwd(qs, rq, qw, dqh)
    dk, dkw = rms_bwd(ks, rk, kw, dkh)
    # "swap_window": every window's rows are written to its horizontal neighbour
    sw = (lambda t: t[:, [1, 0, 3, 2]]) if wrong == "swap_window" else (lambda t: t)
    F = lambda t: R.from_windows(sw(t), Z, S).double()
    return dict(o=F(o), dq=F(dq), dk=F(dk), dv=F(dv), dqw=dqw.double(), dkw=dkw.double())


# ---- fixtures (tools/make_train_short_golden.py mints both from the reference) ---------------------------------------------------
# tests/golden/train_grad_short_ref.npz: the tiny model (net_ch 16, 37 genes) at the configurations whose middle-block AttnBlock
# has windows of 16 tokens (rna_slc 1, patch 64: Z 1, S 8), 8 tokens (rna_slc 4, patch 32: Z 2, S 4) and, never run in training
# before, patch 128 (planes of S = 128, an 8 x 8 gene grid, gene_hidden 256); content of train_grad_ref.npz.
# Three cases share one file under the size limit of a committed fixture, and a zip member costs more than the five numbers it
# would hold: per case the norms and the projections are stored packed -- "<case>/keys" (the parameter names), "<case>/norm" [P],
# "<case>/proj" [P, GRAD_PROBES] in that order -- and "<case>/loss", "<case>/full/<key>" as train_grad_ref.npz has them.
# name -> (PathConfig overrides, images b, seed, loss type, crop index (ix, iy))
GRAD_SHORT_CASES = {
    "slc1_p64": (dict(net_ch=16, rna_num=37, rna_slc=1, patch_size=64), 2, 4, "mse", (1, 0)),
    "slc4_p32": (dict(net_ch=16, rna_num=37, rna_slc=4, patch_size=32), 2, 5, "mse", (0, 1)),
    "slc4_p128": (dict(net_ch=16, rna_num=37, rna_slc=4, patch_size=128), 1, 6, "mse", (1, 0)),
}


def make_short_inputs(name):
    """-> (cfg overrides, loss type, crop, the tuple of train_cases.make_inputs at the case's patch size, channels and rna_slc)"""
    from teramind_amd.config import PathConfig
    over, b, seed, loss_type, crop = GRAD_SHORT_CASES[name]
    cfg = PathConfig(**over)
    return over, loss_type, crop, make_inputs(seed, b=b, ps=cfg.patch_size, C=cfg.n_stain * cfg.z_size, srna=cfg.rna_slc)


# tests/golden/train_attn_short_ref.npz: AttnBlocks at windows the model fixtures do not reach -- 4 tokens (Z 1, S 4) and 16 tokens
# from four planes of S = 4; G not a multiple of 8
ATTN_SHORT_CASES = {"c32_g20_z1_s4": dict(C=32, G=20, Z=1, S=4, N=4, seed=21),
                    "c32_g20_z4_s4": dict(C=32, G=20, Z=4, S=4, N=2, seed=23)}


def make_attn_short_inputs(name):
    """-> x [N,C,Z,S,S], cond [N,G,Z,S,S], dout like x, params {reference key suffix: tensor}; seeded as train_cases does."""
    from teramind_amd import synth
    c = ATTN_SHORT_CASES[name]
    C, G, Z, S, N, seed = c["C"], c["G"], c["Z"], c["S"], c["N"], c["seed"]
    x = synth.normal(f"attn/{name}/x", (N, C, Z, S, S), seed)
    cond = synth.normal(f"attn/{name}/cond", (N, G, Z, S, S), seed + 1)
    dout = synth.normal(f"attn/{name}/dout", (N, C, Z, S, S), seed + 2)
    params = {}
    for k, shp in ATTN_SHAPES(C, G).items():
        r = synth.normal(f"attn/{name}/{k}", shp, seed + 3)
        if k.endswith("norm.weight") or k in ("norm1.weight", "norm2.weight"):
            params[k] = 1.0 + 0.2 * r
        elif k.endswith(".bias"):
            params[k] = 0.1 * r
        else:
            params[k] = r / (shp[1] ** 0.5)
    return x, cond, dout, params
