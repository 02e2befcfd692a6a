"""The gene-gene attention block (tera-mind_amd/csrc/tm_attn.hip: gene_attn_mfma_kernel, gene_attn_generic_kernel, rna_mid_kernel,
gene_readout_kernel, gene_readout_gather_kernel) behind the hooks tm_op_gene_attn / tm_op_rna_mid / tm_op_gene_readout: the
float64 model, its deliberately wrong variants, the fp32 error bounds, the data and the case tables of
tests/test_gpu_gene_attn.py.  No GPU is needed here; tests/test_gene_attn_cases_host.py checks the model against the oracle,
the bounds against a float32 evaluation and against every wrong variant, and the launch rules restated below.

The block (oracle.teramind_cpu.gene_attention_tokens), per patch, tokens = G genes x D = gn^2 zs features:
    tok[g][z gn^2 + hw] = rna[hw][z 500 + slot(g)]  (zero outside the slice mask [zlo, zhi)),  slot(g) = gidx[g] or g
    q = Wq tok + bq,  qn = w_q q rsqrt(mean q^2 + eps),  P = softmax(qn qn^T / D)                       -> attn_map [B][G][G]
    o = Wp (Wv (P tok) + bv) + bp,  h = w_2 o rsqrt(mean o^2 + eps),  y = W2 gelu_tanh(W1 h + b1) + b2   -> out_tok, CB8
The read-out (oracle pathway_readout on gene_attention_maps) keeps the K x K blocks `sub` of the four maps (slice pairs
[0, 2), [1, 3), [2, 4) and all slices) at the genes glst and contracts them with those genes' counts in the two middle slices.

The bounds (U = 2^-24, first order, propagated stage by stage in float64; no constant comes from an observed error)
-------------------------------------------------------------------------------------------------------------------
Linear chain y = W x + b of K terms (fma chain or matrix pipe, then the bias): every product passes through at most K + 1
additions and rounds at most once itself, and the input error passes through |W|:
    dy <= |W| dx + (K + 2) U (|W| |x| + |b|),      K = D (q, v, proj, fc1, the logits), G (P tok), 4 D (fc2).
The keys the MFMA kernel adds beyond G are exact zeros and round nothing; the read-out sums q as slice partials, chains of
the same length class.
RMSNorm y = w (x r), r = 1 / sqrt(mean x^2 + eps) (train_op_ref.window_attn_fwd's derivation, plus the input error that q
and o carry here): the D-term sum of squares, the mean and + eps are (D + 3) U relative on s = mean x^2 + eps, the input
moves s by 2 mean(|x| dx) / s relative; the square root halves both and adds SQRT_ULP, the division DIV_ULP (2 U per ulp):
    dr / r <= (mean(|x| dx) / s) + (D + 3) U / 2 + 2 U (SQRT_ULP + DIV_ULP),      dy <= |w| r dx + |y| (dr / r + 2 U).
Softmax (as there): with t = |l - max l|, e = exp(l - m) is off by e_e = dl + U t + R.exp_rel_bound(t) relative, and
p = e / sum by e_p = e_e + sum_u p e_e + (G + 1) U + 2 U DIV_ULP, taken as e_p / (1 - e_p): dp = p e_p.
GELU g(x) = 0.5 x (1 + tanhf(i)), i = kb (x + kk x^3) (gelu_tanh_f, tm_device.h): i carries at most 8 U of
kb (|x| + kk |x|^3) (two rounded literals, three products, one sum, the last product); tanhf is TANH_ULP ulp; 1 + tanh rounds
once, the two outer products once each; the pre-activation's own error passes through |g'| <= conv1_cases.GELU_SLOPE:
    dg <= GELU_SLOPE dx + 0.5 |x| ((1 - th^2) 8 U kb (|x| + kk |x|^3) + 2 U TANH_ULP |th| + U (1 + th)) + 2 U |g|
          + 2^-52 |x| + FLT_MIN          (the 2^-52 |x| is the float64 reference's own cancellation in 1 + tanh, as in conv1_cases).
The tail.  Up to pt = P tok the stages mix the genes of a patch and the bounds above are chained as they stand (an error
bound dx enters the next stage through |W|, the worst case of errors known only by magnitude).  From pt on every stage acts on
one gene's row alone, and chaining magnitudes there gives a bound larger than the output itself (|W| has row sums of
0.8 sqrt(K) while the values stay O(1): 6.0 against |y| <= 2.8 at G = 229, D = 64, 'mid').  So the tail is linearised exactly:
each stage s commits a local error e_s with |e_s| <= m_s (the formulas above with dx = 0), the first-order error of y is
sum_s J_s e_s with J_s = dy / d(stage s) of that row, and its worst case over |e_s| <= m_s is
    dy <= m_y + |W2| m_g + |W2 G' W1| m_h + |W2 G' W1 Jr| m_op + |W2 G' W1 Jr Wp| m_ov + |W2 G' W1 Jr Wp Wv| dpt,
G' = diag(gelu'(y1)), Jr = diag(w_2 r) (I - xh xh^T / D) the RMSNorm's Jacobian at xh = o r; the absolute value is taken of the
products, once.  m_g already holds GELU_SLOPE m_y1 (fc1's local error passes through no further matrix than W2).  The same
seven local bounds, no new constant: 0.002 .. 0.007 at D = 64 and 0.25 at D = 512 instead of 6 and more.
Read-out: sub is a block of P (dp); out = sum_g sub count_g over K genes: sum_g dp |count| + (K + 2) U sum_g p |count|; the
raw-count rows are exact.

What these worst-case bounds cannot see: erf-GELU instead of tanh-GELU moves y by about 1e-3.  That is 18 .. 78 times the bound
at D = 4, but only 2 .. 9 times at D = 16 and 0.1 .. 0.7 of the bound at D >= 64, even in an all-zero patch (where dpt = 0 and
only fc1's and fc2's own chains are left): `applies` names the variant for D = 4 alone, the fused kernel (D = 64) never.

The allowances in ulp.  TANH_ULP = 2 is what tests/test_gpu_train_ops.py (test_ew_float) already grants tanhf.  SQRT_ULP and
DIV_ULP = 1: the HIP math API reference (ROCm documentation, "HIP math API", single precision) lists sqrtf at 1 ulp, and hipcc
compiles fp32 sqrt and division correctly rounded by default (-fhip-fp32-correctly-rounded-divide-sqrt); 1 ulp covers both."""
import functools
import math
import zlib

import torch

import conv1_cases as K1
import train_op_ref as R
from oracle import teramind_cpu as tc

U = R.U
EPS = R.EPS
SQRT_ULP, DIV_ULP, TANH_ULP = 1, 1, 2
SLOTS = 500                                   # gene slots per slice of the dense tensor
GROWS = 232                                   # genes the MFMA kernel keeps in LDS
RO_CHUNK = 8                                  # patches per chunk of the gather route

# the twelve host arrays of the hooks, in their order (tm_model_finalize's packing order)
W_KEYS = ("attn.q.weight", "attn.q.bias", "attn.v.weight", "attn.v.bias", "attn.q_norm.weight", "attn.proj.weight",
          "attn.proj.bias", "norm2.weight", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
KINDS = {"plain": 1.0, "mid": 2.5, "sharp": 6.0}      # factor on q_norm.weight


# ------------------------------------------------------------------------------------------------------- launch rules, restated
def form_of(D, G, gidx):
    """form 0 of the hooks = the model's rule (gene_mfma_rule): 1 = the fused D = 64 kernels, 2 = the generic kernel."""
    return 1 if D == 64 and G <= GROWS and gidx is None else 2


def generic_split(B):
    """gene_generic_split: workgroups per patch of the generic kernel."""
    return 1 if B >= 512 else (2 if B >= 256 else 4)


def mfma_split(B):
    return 1 if B >= 256 else 2


def shares_of(form, B):
    return mfma_split(B) if form == 1 else generic_split(B)


def share_rows(form, G, shares, share):
    """The query rows (genes) that workgroup `share` of a patch writes.  MFMA: wave w of share y owns query blocks of 32 genes
    qb = w + 4 y, + 4 gridDim.y, ...; generic: wave w owns the groups of 4 rows (w + 4 y) + 4 gridDim.y j."""
    g = torch.arange(G)
    if form == 1:
        return g[((g // 32) // 4) % shares == share]
    return g[((g // 4) // 4) % shares == share]


# ------------------------------------------------------------------------------------------------------------------- cases
class Case(dict):
    """gn, zs, G, B, form (the hook's argument), kind, zlo, zhi, outs ('tok', 'map' or 'both'), table (None, 'm2h', 'fold')."""
    __getattr__ = dict.__getitem__

    @property
    def D(self):
        return self.gn * self.gn * self.zs

    @property
    def run_form(self):
        return self.form or form_of(self.D, self.G, gidx_of(self))

    @property
    def id(self):
        return (f"f{self.form}-gn{self.gn}z{self.zs}-G{self.G}-B{self.B}-{self.kind}-m{self.zlo}_{self.zhi}-{self.outs}"
                + (f"-{self.table}" if self.table else ""))


def case(gn, zs, G, B, form=0, kind="mid", mask=None, outs="both", table=None):
    zlo, zhi = mask or (0, zs)
    return Case(gn=gn, zs=zs, G=G, B=B, form=form, kind=kind, zlo=zlo, zhi=zhi, outs=outs, table=table)


def gidx_of(c):
    """The gene slot table of a case (int32 [G]) or None.  'm2h': the 81 shared genes of the human-brain panel; 'fold': G > 500
    genes folded back onto the 500 slots (3 g + 7) mod 500, so some genes share a slot."""
    if c.table == "m2h":
        assert c.G == len(tc.M2H)
        return torch.tensor(tc.M2H, dtype=torch.int32)
    if c.table == "fold":
        return ((3 * torch.arange(c.G) + 7) % SLOTS).to(torch.int32)
    return None


def mfma_cases():
    """The fused kernel (D = 64).  G = 232 is GROWS exactly, 225 the first gene of the last query block, at 200 that block lies
    wholly beyond G, 33 / 32 are one gene past / exactly one query block; B = 256 flips gridDim.y from 2 to 1."""
    cs = [case(4, 4, 229, 3, kind=k) for k in KINDS]
    cs += [case(8, 1, 229, 1), case(2, 16, 229, 3), case(8, 1, 33, 1, outs="map"), case(2, 16, 232, 1, outs="map")]
    cs += [case(4, 4, 229, 1, outs="tok"), case(4, 4, 229, 1, outs="map")]
    cs += [case(4, 4, 232, 3), case(4, 4, 225, 1, outs="tok"), case(4, 4, 200, 3, outs="map"), case(4, 4, 200, 1),
           case(4, 4, 33, 3), case(4, 4, 32, 1), case(4, 4, 1, 3)]
    cs += [case(4, 4, 229, 256), case(4, 4, 33, 256, outs="map")]
    cs += [case(4, 4, 229, 1, mask=(1, 3)), case(4, 4, 229, 3, mask=(3, 4)), case(4, 4, 229, 1, form=1, mask=(1, 3), outs="map")]
    return cs


def generic_cases():
    """The generic kernel.  G = 64 and 512 are G == Gp (no pad key columns), 3 and 1 are below GG_RB = 4 rows, (8, 8) at G = 512
    asks for exactly 160 KB of LDS; B = 256 / 512 run 2 / 1 workgroups per patch; G = 229 at (4, 4) is the checkpoint geometry
    with form 2 forced."""
    cs = [case(2, 1, 3, 5), case(2, 1, 1, 1), case(2, 1, 500, 1), case(4, 1, 64, 5), case(4, 1, 65, 1), case(4, 1, 81, 5, table="m2h"),
          case(4, 1, 229, 1, mask=(0, 1)), case(4, 1, 40, 256), case(4, 1, 40, 512), case(4, 1, 40, 512, outs="map")]
    cs += [case(4, 8, 229, 1, mask=(1, 3)), case(4, 8, 500, 1, outs="tok"), case(4, 8, 64, 5, mask=(1, 3), outs="map"),
           case(4, 16, 65, 5), case(4, 16, 3, 1), case(8, 4, 229, 1), case(8, 4, 512, 1, table="fold"),
           case(8, 8, 512, 1, table="fold"), case(8, 8, 3, 1), case(8, 8, 65, 1, mask=(1, 3))]
    cs += [case(4, 4, 229, 5, form=2, kind=k) for k in KINDS]
    cs += [case(4, 4, 500, 1), case(4, 4, 229, 1, form=2, mask=(1, 3), outs="map"), case(4, 4, 1, 1, form=2)]
    return cs


def attn_cases():
    return mfma_cases() + generic_cases()


def readout_cases():
    """(case, glst, want_sub).  Fused (form 1 by the model's rule): G in {229, 232, 33}, every K in 1 .. 8, glst unsorted with 0 and
    G - 1, B in {1, 7}.  Gather route: G = 500 at (4, 4), G = 229 at (8, 4), B = 11 = one chunk of 8 and a tail of 3."""
    out = []
    for i, Kn in enumerate(range(1, 9)):
        G = (229, 232, 33)[i % 3]
        out.append((case(4, 4, G, (1, 7)[i % 2]), glst_of(G, Kn), i % 3 != 1))
    out.append((case(4, 4, 229, 7, kind="sharp"), glst_of(229, 8), True))
    out.append((case(4, 4, 229, 1, kind="plain"), glst_of(229, 5), False))
    out.append((case(4, 4, 500, 11), glst_of(500, 4), True))
    out.append((case(8, 4, 229, 11), glst_of(229, 8), False))
    out.append((case(4, 4, 229, 11, form=2, kind="plain"), glst_of(229, 3), True))
    return out


def glst_of(G, Kn):
    """K distinct genes, unsorted, with G - 1 first and 0 among them (K >= 2)."""
    pool = [G - 1, 0, G // 3, 5, G // 2 + 1, 2, G - 4, 9]
    got = []
    for g in pool:
        if 0 <= g < G and g not in got:
            got.append(g)
    assert len(got) >= Kn
    return got[:Kn]


# -------------------------------------------------------------------------------------------------------------------- data
def special_genes(G):
    """(all-zero gene or None, (a, b) identical genes or None)."""
    return (G // 2 if G >= 3 else None), ((0, G - 1) if G >= 2 else None)


@functools.lru_cache(maxsize=4)
def _make(key):
    c = Case(key)
    g = torch.Generator().manual_seed(zlib.crc32(repr(sorted((k, v) for k, v in c.items() if k not in ("form", "outs"))).encode()))
    D, G, B = c.D, c.G, c.B
    shape = (B, c.gn, c.gn, c.zs, SLOTS)
    rna = torch.randint(0, 8, shape, generator=g).float() * (torch.rand(shape, generator=g) < 0.4).float()
    gidx = gidx_of(c)
    slot = (lambda gene: int(gidx[gene])) if gidx is not None else (lambda gene: gene)
    zero, same = special_genes(G)
    if same is not None:
        rna[..., slot(same[1])] = rna[..., slot(same[0])]
    if zero is not None:
        rna[..., slot(zero)] = 0.0
    if B > 1:
        rna[B // 2] = 0.0
    rn = lambda *s: torch.randn(s, generator=g)
    uni = lambda n: torch.rand(n, generator=g) + 0.5
    W = [rn(D, D) / math.sqrt(D), 0.3 * rn(D), rn(D, D) / math.sqrt(D), 0.3 * rn(D), uni(D) * KINDS[c.kind],
         rn(D, D) / math.sqrt(D), 0.3 * rn(D), uni(D), rn(4 * D, D) / math.sqrt(D), 0.3 * rn(4 * D),
         rn(D, 4 * D) / math.sqrt(4 * D), 0.3 * rn(D)]
    return dict(rna=rna.reshape(B, c.gn, c.gn, c.zs * SLOTS).contiguous(), W=[w.contiguous() for w in W], gidx=gidx)


def make(c):
    """fp32 inputs of a case: rna [B, gn, gn, zs 500] (integer counts 0 .. 7 at density 0.4 in EVERY slot, so a wrong slot is a
    wrong count; one all-zero gene, one pair of identical genes, with B > 1 one all-zero patch), W = the twelve arrays of W_KEYS
    (randn / sqrt(in), biases 0.3 randn, norm weights in [0.5, 1.5], q_norm.weight times KINDS[kind]) and gidx.  The data depend
    on the geometry, kind and mask, not on form / outs."""
    return _make(tuple(sorted(c.items())))


# ------------------------------------------------------------------------------------------------------------------- model
WRONG = ("scale", "drop_key", "pad_keys", "zlo_off", "zhi_off", "no_bv", "no_norm2_w", "erf_gelu", "feat_order", "swap_cb8",
         "share_unwritten", "no_gidx")
RO_WRONG = ("glst_sorted", "map3_pair", "mid_swap")


def tokens(rna, c, gidx, zlo, zhi, wrong=None, dtype=torch.float64):
    """Dense rna [B, gn, gn, zs 500] -> tokens [B, G, D], feature d = z gn^2 + hw (rna_h.reshape(B, G, -1) of the oracle)."""
    B = rna.shape[0]
    r = rna.to(dtype).reshape(B, c.gn * c.gn, c.zs, SLOTS)
    slots = gidx.long() if gidx is not None and wrong != "no_gidx" else torch.arange(c.G) % SLOTS
    t = r[..., slots].clone()                                          # [B, hw, z, G]
    lo = zlo + 1 if wrong == "zlo_off" else zlo
    hi = zhi - 1 if wrong == "zhi_off" else zhi
    z = torch.arange(c.zs)
    t[:, :, (z < lo) | (z >= hi)] = 0.0
    if wrong == "feat_order":
        return t.permute(0, 3, 1, 2).reshape(B, c.G, c.D)              # d = hw zs + z: the dense tensor's own order
    return t.permute(0, 3, 2, 1).reshape(B, c.G, c.D)


def _linear(x, dx, w, b, Kn):
    y = x @ w.T + b
    return y, dx @ w.abs().T + (Kn + 2) * U * (x.abs() @ w.abs().T + b.abs())


def _rms(x, dx, w):
    Dn = x.shape[-1]
    s = x.pow(2).mean(-1, keepdim=True) + EPS
    r = torch.rsqrt(s)
    y = w * (x * r)
    dr = (x.abs() * dx).mean(-1, keepdim=True) / s + (Dn + 3) * U / 2 + 2 * U * (SQRT_ULP + DIV_ULP)
    return y, w.abs() * r * dx + y.abs() * (dr + 2 * U)


def _gelu(x, dx, erf):
    if erf:
        return K1.gelu_erf(x), dx
    ax = x.abs()
    th = torch.tanh(R.KB * (x + R.KK * x ** 3))
    g = 0.5 * x * (1.0 + th)
    d = (K1.GELU_SLOPE * dx + 0.5 * ax * ((1 - th * th) * 8 * U * R.KB * (ax + R.KK * ax ** 3) + 2 * U * TANH_ULP * th.abs() + U * (1 + th))
         + 2 * U * g.abs() + 2.0 ** -52 * ax + R.FLT_MIN)
    return g, d


def block(tok, W, wrong=None, want_tok=True, want_bound=True):
    """The block on tokens [B, G, D] in tok's dtype (float64: the model; float32: an evaluation in torch's own summation order).
    Returns (y [B, G, D] or None, P [B, G, G], dy, dP): the bounds are meaningful in float64; dy is None unless want_bound."""
    dt = tok.dtype
    wq, bq, wv, bv, qw, wp, bp, n2, w1, b1, w2, b2 = (w.to(dt) for w in W)
    G, D = tok.shape[1:]
    q, dq = _linear(tok, torch.zeros_like(tok), wq, bq, D)
    qn, dqn = _rms(q, dq, qw)
    kn, dkn, ktok = qn, dqn, tok
    if wrong == "pad_keys" and G % 64:                                 # all-zero pad tokens up to the next multiple of 64 take part
        pad = torch.zeros((tok.shape[0], 64 - G % 64, D), dtype=dt)
        ktok = torch.cat([tok, pad], 1)
        kq, dkq = _linear(ktok, torch.zeros_like(ktok), wq, bq, D)
        kn, dkn = _rms(kq, dkq, qw)
    scale = D ** -0.5 if wrong == "scale" else 1.0 / D
    l = (qn @ kn.transpose(-2, -1)) * scale
    lmag = (qn.abs() @ kn.abs().transpose(-2, -1)) * scale
    dl = (dqn @ kn.abs().transpose(-2, -1) + qn.abs() @ dkn.transpose(-2, -1)) * scale + (D + 2) * U * lmag + U * l.abs()
    if wrong == "drop_key" and G > 1:
        l = l.clone()
        l[..., G - 1] = -math.inf
    p = torch.softmax(l, dim=-1)
    t = (l - l.max(-1, keepdim=True).values).abs()
    t = torch.where(torch.isinf(t), torch.zeros_like(t), t)
    e_e = dl + U * t + R.exp_rel_bound(t)
    e_p = e_e + (p * e_e).sum(-1, keepdim=True) + (G + 1) * U + 2 * U * DIV_ULP
    dp = p * (e_p / (1.0 - e_p).clamp_min(0.5)) + R.FLT_MIN
    pmap, dpmap = p[..., :G], dp[..., :G]
    if not want_tok:
        return None, pmap, None, dpmap
    Kn = ktok.shape[1]
    pt = p @ ktok
    dpt = dp @ ktok.abs() + (Kn + 2) * U * (p @ ktok.abs())
    y, dy = _tail(pt, dpt, (wv, bv, wp, bp, n2, w1, b1, w2, b2), wrong, want_bound)
    return y, pmap, dy, dpmap


def _tail(pt, dpt, Wt, wrong, want_bound, rows_per_chunk=16):
    """The row-local tail pt -> ov -> op -> h -> y1 -> g -> y of the block and its bound (module docstring, "The tail")."""
    wv, bv, wp, bp, n2, w1, b1, w2, b2 = Wt
    D = pt.shape[-1]
    if wrong == "no_bv":
        bv = torch.zeros_like(bv)
    if wrong == "no_norm2_w":
        n2 = torch.ones_like(n2)
    lin = lambda x, w, b, Kn: (x @ w.T + b, (Kn + 2) * U * (x.abs() @ w.abs().T + b.abs()))
    ov, m_ov = lin(pt, wv, bv, D)
    op, m_op = lin(ov, wp, bp, D)
    r = torch.rsqrt(op.pow(2).mean(-1, keepdim=True) + EPS)
    xh = op * r
    h = n2 * xh
    m_h = h.abs() * ((D + 3) * U / 2 + 2 * U * (SQRT_ULP + DIV_ULP) + 2 * U)
    y1, m_y1 = lin(h, w1, b1, D)
    g, m_g = _gelu(y1, m_y1, wrong == "erf_gelu")                      # m_g: the GELU's own roundings + GELU_SLOPE m_y1
    y, m_y = lin(g, w2, b2, 4 * D)
    if not want_bound:
        return y, None
    dy = m_y + m_g @ w2.abs().T
    gp = R.gelu_tanh_grad(y1)
    shp = y.shape
    f = lambda t: t.reshape(-1, t.shape[-1])
    gp, xh, nr, m_h, m_op, m_ov, dpt, dy = f(gp), f(xh), f(n2 * r), f(m_h), f(m_op), f(m_ov), f(dpt), f(dy).clone()
    for i in range(0, dy.shape[0], rows_per_chunk):
        s = slice(i, i + rows_per_chunk)
        C = (w2 * gp[s, None, :]) @ w1                                   # [n, D, D]: dy / dh of each row
        Jo = C * nr[s, None, :]
        Jo = Jo - (Jo @ xh[s, :, None]) * xh[s, None, :] / D             # dy / d op
        Jv = Jo @ wp                                                     # dy / d ov
        Jp = Jv @ wv                                                     # dy / d pt
        for J, m in ((C, m_h), (Jo, m_op), (Jv, m_ov), (Jp, dpt)):
            dy[s] += (J.abs() @ m[s, :, None])[..., 0]
    return y, dy.reshape(shp)


def forward(c, data=None, wrong=None, dtype=torch.float64, mask=None, want_tok=True, want_bound=None, chunk=32):
    """The hook's two outputs for a case: dict(tok [B, G, D], map [B, G, G], dtok, dmap) (tok / dtok None unless want_tok).
    wrong: one of WRONG.  Evaluated in chunks of `chunk` patches."""
    assert wrong is None or wrong in WRONG
    data = data or make(c)
    zlo, zhi = mask or (c.zlo, c.zhi)
    if want_bound is None:
        want_bound = wrong is None and dtype == torch.float64
    outs = []
    for n0 in range(0, c.B, chunk):
        tok = tokens(data["rna"][n0:n0 + chunk], c, data["gidx"], zlo, zhi, wrong, dtype)
        outs.append(block(tok, data["W"], wrong, want_tok, want_bound))
    y, p, dy, dp = (torch.cat(t) if t[0] is not None else None for t in zip(*outs))
    if y is not None and wrong == "swap_cb8" and c.G >= 2:
        y = y.clone()
        y[:, [0, 1]] = y[:, [1, 0]]
    if wrong == "share_unwritten":
        f = c.run_form
        rows = share_rows(f, c.G, shares_of(f, c.B), 1)
        p = p.clone()
        p[:, rows] = 0.0
        if y is not None:
            y = y.clone()
            y[:, rows] = 0.0
    return dict(tok=y, map=p, dtok=dy, dmap=dp)


def applies(wrong, c):
    """Where a wrong variant can be seen (and by which output).  scale: not under 'sharp' (a one-hot softmax stays one-hot) and
    not at G = 1; drop_key, swap_cb8: the last / second gene must exist and differ (G >= 3: genes 0 and G - 1 are identical);
    pad_keys: G no multiple of 64; the mask errors: always (an emptied mask gives all-zero tokens); feat_order: gn > 1 and
    zs > 1, else both orders coincide; share_unwritten: more than one workgroup per patch and a row in share 1; no_gidx: a
    table; no_bv, no_norm2_w, erf_gelu, swap_cb8: the token output only; erf_gelu: D = 4 only (module docstring: about 1e-3,
    inside ten times the bound from D = 16 on)."""
    if wrong == "erf_gelu" and c.D > 4:
        return False
    tok_only = wrong in ("no_bv", "no_norm2_w", "erf_gelu", "swap_cb8")
    if tok_only and c.outs == "map":
        return False
    if wrong == "scale":
        return c.kind != "sharp" and c.G > 1
    if wrong in ("drop_key", "swap_cb8"):
        return c.G >= 3
    if wrong == "pad_keys":
        return c.G % 64 != 0
    if wrong == "feat_order":
        return c.gn > 1 and c.zs > 1
    if wrong == "share_unwritten":
        f = c.run_form
        return shares_of(f, c.B) > 1 and len(share_rows(f, c.G, shares_of(f, c.B), 1)) > 0
    if wrong == "no_gidx":
        return c.table is not None
    return True


def to_cb8(y, fill=float("nan")):
    """Tokens [B, G, D] -> the CB8 image [B][ceil(G/8)][D][8] (= [B][Gb][zs][gn][gn][8]); the pad slots hold `fill`."""
    B, G, D = y.shape
    Gb = (G + 7) // 8
    o = torch.full((B, Gb * 8, D), fill, dtype=y.dtype)
    o[:, :G] = y
    return o.reshape(B, Gb, 8, D).permute(0, 1, 3, 2).contiguous()


def rna_mid(rna, c):
    """rna_h[:, :, 1:-1]: [B, G, zs - 2, gn, gn] (no table: the first G slots)."""
    B = rna.shape[0]
    r = rna.reshape(B, c.gn, c.gn, c.zs, SLOTS)[..., 1:c.zs - 1, :c.G]
    return r.permute(0, 4, 3, 1, 2).contiguous()


# ----------------------------------------------------------------------------------------------------------------- read-out
def readout(c, glst, data=None, wrong=None, dtype=torch.float64):
    """dict(out [B, 4K, 2 gn^2], sub [4, B, K, K], dout, dsub): rows (map 0 | map 1) x middle slice 0 and (map 1 | map 2) x middle
    slice 1 side by side, then map 3 x both middle slices, then the raw counts.  wrong: one of RO_WRONG, or of WRONG (passed on
    to the maps)."""
    assert c.zs == 4 and (wrong is None or wrong in RO_WRONG + WRONG)
    data = data or make(c)
    gl = sorted(glst) if wrong == "glst_sorted" else list(glst)
    Kn, gg, B = len(gl), c.gn * c.gn, c.B
    masks = [(0, 2), (1, 3), (2, 4), (0, 2) if wrong == "map3_pair" else (0, 4)]
    fw = [forward(c, data, wrong if wrong in WRONG else None, dtype, mask=m, want_tok=False) for m in masks]
    pick = lambda a: a[:, gl][..., gl]
    sub, dsub = torch.stack([pick(f["map"]) for f in fw]), torch.stack([pick(f["dmap"]) for f in fw])
    slots = data["gidx"].long()[gl] if data["gidx"] is not None else torch.tensor(gl)
    cnt = data["rna"].to(dtype).reshape(B, gg, 4, SLOTS)[:, :, 1:3][..., slots].permute(0, 3, 2, 1)     # [B, K, 2, hw]
    if wrong == "mid_swap":
        cnt = cnt.flip(2)

    def prod(m, s):                                                   # [B, K, hw] or [B, K, 2 hw]
        cs = cnt[:, :, s] if s is not None else cnt.reshape(B, Kn, 2 * gg)
        return sub[m] @ cs, dsub[m] @ cs.abs() + (Kn + 2) * U * (sub[m] @ cs.abs())
    rows, drows = [], []
    for m0 in (0, 1):
        (a, da), (b, db) = prod(m0, 0), prod(m0 + 1, 1)
        rows.append(torch.cat([a, b], -1))
        drows.append(torch.cat([da, db], -1))
    a, da = prod(3, None)
    raw = cnt.reshape(B, Kn, 2 * gg)
    out = torch.cat(rows + [a, raw], 1)
    dout = torch.cat(drows + [da, torch.zeros_like(raw)], 1)
    return dict(out=out, sub=sub, dout=dout, dsub=dsub)


def ro_applies(wrong, c, glst):
    if wrong == "glst_sorted":
        return list(glst) != sorted(glst)
    return True
