"""Cases, inputs, error bounds and a float32 emulation of the long-window training attention core (tm_op_window_attn_train at
windows of 256 / 512 tokens: attn_long_* in csrc/tm_train.hip), shared by tests/test_gpu_window_attn_train_long.py (which holds
the kernels to the bounds) and tests/test_window_attn_train_long_ref.py (which shows that the bounds reject wrong variants).

The bounds are first order in U = 2^-24 and follow the kernels' accumulation orders as their header comment states them; the
matrix unit's adder is taken as 2 U per addition (train_op_ref.window_attn_fwd does the same).  With lmax = the largest
sum_c |qh kh| / C of the case and mag = train_op_ref.window_attn_mag (every sum over |terms|):

  r      = 1 / sqrt(sum_c x^2 / C + eps): a C-term sum, mean, + eps, sqrt, reciprocal: e_r = (C + 5) U.
  logit  s = (sum_c qh kh) / C, qh = (q r) qw: operands (e_r + 2 U) each, a C-term MFMA chain (2 C U), 1 / C and its product
         (2 U):  |ds| <= (4 C + 20) U lmax = dl.
  P      = expf(s - m) * (1 / l), m the maximum of the computed logits (a shift common to a row cancels, its rounding does not):
         2 dl from the logits of the row, the subtraction (U |s - m|) and train_op_ref.exp_rel_bound (2 U |s - m| + 4 U) with
         |s - m| <= 2 lmax, once for the element and once more for the row sum it is divided by; the row sum's T terms (64 in a
         lane, the other half-wave, T / 128 blocks: fewer than T additions); the reciprocal and two products:
         e_P = 2 dl + (12 lmax + T + 16) U.
  o, dv  a T-term MFMA chain of P times data:  (e_P + (2 T + 2) U) mag.
  dP     = do . v, a C-term chain: 2 C U.  D = rowsum(dP o P) = (sum_j e dP) / l: e_P + (2 C + T + 8) U of sum_j P |dP|.
  dS     = P (dP - D) / C:  2 e_P + (2 C + T + 12) U of P (|dP| + sum P |dP|) / C, which is mag's dS.
  dqh    = dS kh (dkh = dS^T qh), a T-term chain of dS times operands that carry e_r + 2 U:  e_dS + (C + 2 T + 7) U.
  dq     = r g - q r^3 mean_c(g q), g = dqh qw: four factors r, the C-term dot and a dozen single roundings: (5 C + 30) U more:
         E = 2 e_P + (8 C + 3 T + 60) U  of mag dq / dk.
  dqw    = sum over tokens of dqh q r: 64-lane wave sums, then the ceil(voxels / 64) workgroup partials in
         train_op_ref.depth_two_stage:  (E + depth U) of mag dqw / dkw.
"""
import torch

import train_op_ref as R

U = R.U

# (N, C, Z, S): T = Z (S/2)^2 = 256 (the fixture's width; C off the CB8 block and two patches; the checkpoint width; one plane,
# so the token map cannot assume Z = 4) and 512 (and at the widest C)
LONG_CASES = [(1, 64, 4, 16), (2, 13, 4, 16), (1, 256, 4, 16), (1, 8, 1, 32), (1, 40, 8, 16), (1, 256, 2, 32)]
KINDS = ("plain", "sharp", "zeros")
WRONG = ("scale", "drop_last_key_block", "stats_first_block", "no_rowdot", "dk_first_query_block", "hwz")
OUTPUTS = ("o", "dq", "dk", "dv", "dqw", "dkw")


def inputs(N, C, Z, S, kind):
    """fp32 q, k, v, qw, kw of train_op_ref.attn_inputs in `kind`, and a seeded dout."""
    q, kv, qw, kw = R.attn_inputs(N, C, Z, S, False, kind, seed=11)
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
    dl = (4 * C + 20) * U * lmax
    eP = 2 * dl + (12 * lmax + T + 16) * U
    E = 2 * eP + (8 * C + 3 * T + 60) * U
    Ew = E + R.depth_two_stage((N * Z * S * S + 63) // 64) * U
    return dict(o=(eP + (2 * T + 2) * U) * mag["o"], dv=(eP + (2 * T + 2) * U) * mag["dv"], dq=E * mag["dq"], dk=E * mag["dk"],
                dqw=Ew * mag["dqw"], dkw=Ew * mag["dkw"])


def emulate_f32(q, k, v, qw, kw, d, Z, S, wrong=None):
    """The core in float32 torch the way the kernels walk it (keys / queries in blocks of 128, max and sum in two passes),
    NCDHW in, the six outputs as float64.  wrong: one of WRONG, a deliberate error."""
    assert wrong is None or wrong in WRONG
    C = q.shape[1]
    T = Z * (S // 2) ** 2
    W = lambda t: R.to_windows(t.float(), Z, S)
    qs, ks, vs, ds = (R.to_windows_hwz(q.float(), Z, S) if wrong == "hwz" else W(q)), W(k), W(v), W(d)
    rq = 1.0 / torch.sqrt(qs.pow(2).sum(-1, keepdim=True) / C + R.EPS)
    rk = 1.0 / torch.sqrt(ks.pow(2).sum(-1, keepdim=True) / C + R.EPS)
    qh, kh = qs * rq * qw, ks * rk * kw
    inv_c = torch.tensor(1.0 / C ** 0.5 if wrong == "scale" else 1.0 / C, dtype=torch.float32)
    blocks = [slice(b, b + 128) for b in range(0, T, 128)]
    s = torch.cat([(qh @ kh[..., b, :].transpose(-2, -1)) * inv_c for b in blocks], -1)
    stat = blocks[:1] if wrong == "stats_first_block" else blocks
    m = torch.stack([s[..., b].max(-1).values for b in stat], -1).max(-1, keepdim=True).values
    e = torch.exp(s - m)
    lsum = blocks[:-1] if wrong == "drop_last_key_block" else stat
    l = sum(e[..., b].sum(-1, keepdim=True) for b in lsum)
    p = e * (1.0 / l)
    o = sum(p[..., b] @ vs[..., b, :] for b in blocks)
    dv = sum(p[..., b, :].transpose(-2, -1) @ ds[..., b, :] for b in blocks)
    dp = ds @ vs.transpose(-2, -1)
    D = torch.zeros_like(m) if wrong == "no_rowdot" else sum((e[..., b] * dp[..., b]).sum(-1, keepdim=True) for b in blocks) * (1.0 / l)
    dS = p * (dp - D) * inv_c
    dqh = sum(dS[..., b] @ kh[..., b, :] for b in blocks)
    kq = blocks[:1] if wrong == "dk_first_query_block" else blocks
    dkh = sum(dS[..., b, :].transpose(-2, -1) @ qh[..., b, :] for b in kq)

    def rms_bwd(x, r, w, dxh):
        dot = (dxh * w * x).sum(-1, keepdim=True) / C
        return r * dxh * w - x * r * r * r * dot, (dxh * x * r).reshape(-1, C).sum(0)
    dq, dqw = rms_bwd(qs, rq, qw, dqh)
    dk, dkw = rms_bwd(ks, rk, kw, dkh)
    F = lambda t: R.from_windows(t, Z, S).double()
    return dict(o=F(o), dq=F(dq), dk=F(dk), dv=F(dv), dqw=dqw.double(), dkw=dkw.double())


# ---- rna_slc 8 fixtures (tools/make_train_slc8_golden.py mints both from the reference) ----------------------------------------
# tests/golden/train_grad_slc8_ref.npz: GRAD_CFG of tests/train_cases.py with rna_slc = 8 (attention at C = 64 with 256-token
# windows, at C = 128 with 64-token windows; down_z at kz = 5), one case in the format of train_grad_ref.npz
SLC8_CFG = dict(net_ch=16, rna_num=37, rna_slc=8)
SLC8_CASES = {"mse_seed3": (3, "mse", (1, 0))}          # (seed, loss type, crop index (ix, iy))
# tests/golden/train_attn_long_ref.npz: one AttnBlock the model fixture does not reach -- 512-token windows from Z = 2, S = 32,
# G not a multiple of 8
ATTN_LONG_CASES = {"c32_g20_z2_s32": dict(C=32, G=20, Z=2, S=32, N=1, seed=13)}


def make_attn_long_inputs(name):
    """-> x [N,C,Z,S,S], cond [N,G,Z,S,S], dout like x, params {reference key suffix: tensor}; seeded as train_cases does."""
    from teramind_amd import synth
    from train_cases import ATTN_SHAPES
    c = ATTN_LONG_CASES[name]
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
