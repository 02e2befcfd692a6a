"""The fp32 1x1x1 conv / Linear (conv1_mfma, tera-mind_amd/csrc/tm_kernels.hip) in every form the model launches: the float64
model of  y = res + gate_up * act(W x + b),  its deliberately wrong variants, the fp32 error bounds and the case tables of
tests/test_gpu_conv1_f32.py.  No GPU is needed here; tests/test_conv1_cases_host.py checks the model against torch, the tables
against the wrong variants, the bounds in both directions and the launcher's tile rule.

Tensors are NCDHW float64.  A "wide" tensor carries more channel blocks than the conv reads (the executor hands the kernel
channel-block slices of the conditioning tensor: kv reads chunk 3, the gates are chunks 2 and 6 of 7 chunks); `make` builds the
wide tensors and the slices the model sees, `to_cb8` / `from_cb8` are the CB8 layout [N][C/8][Z][H][W][8] in torch.

The bounds (U = 2^-24, first order, never fitted to a kernel's output)
----------------------------------------------------------------------
Linear part.  An output sums Kp = 8 * ceil(Cin / 8) products (the pad channels multiply zeros) in a fixed order on the fp32
matrix pipe, two products per v_mfma_f32_32x32x2_f32, then adds the bias: every product passes through at most Kp + 1
additions, each of which rounds once, and the product itself rounds at most once:
    d_lin <= (Kp + 2) U (sum |w x| + |b|).
Epilogue.  out = res + gate * lin: the error of lin is scaled by |gate|, the multiply rounds once (U |gate lin|) and the add
once (U |out|): with |gate lin| <= |res| + |out|
    d_out <= |gate| d_lin + 2 U (|res| + |out|).
GELU (gelu_tanh_hw, tm_device.h):  g(x) = x * rcp(1 + exp2(t)),  t = x * fma(x * x, k1, k0),  k0 = -2 sqrt(2/pi) log2(e),
k1 = 0.044715 k0, so that exp2(t) = exp(-2u), u = sqrt(2/pi) (x + 0.044715 x^3), and g = x / (1 + exp(-2u)) = tanh-GELU.
The roundings, one by one:
  * k0 is the fp32 product of three fp32 literals: two rounded literals (2 is exact) and two products, of which the one by 2
    is exact: 3 U relative.  k1 = k0 * fl(0.044715): 3 U + U + U = 5 U.
  * p = fl(x * x): U.  q = fma(p, k1, k0) rounds once: |dq| <= U |q| + (U + 5 U) |k1| x^2 + 3 U |k0|.
  * t = fl(x * q): |dt| <= U |t| + |x| |dq| <= U |x| (5 |k0| + 8 |k1| x^2)   (|q| = |k0| + |k1| x^2: both are negative).
  * e = v_exp_f32(t), 1 ulp = 2 U relative at worst; dt moves e by ln 2 * |dt| relative.
  * s = fl(1 + e): U, and passes e's relative error on scaled by e / (1 + e).
  * r = v_rcp_f32(s): 1 ulp, 2 U.  g = fl(x * r): U.
    rel(g) <= (ln 2 * |dt| + 2 U) * e / (1 + e) + U + 2 U + U,      abs <= rel * |g| + FLT_MIN + 2^-52 |x|.
    The last term is the float64 reference's own error, not the kernel's: R.gelu_tanh forms 1 + tanh(u), which cancels for
    x << 0 (tanh(u) -> -1 carries an absolute error of about 2^-53), so 0.5 x (1 + tanh u) is off by up to 2^-52 |x| / 2 + its
    own roundings; at x = -7 the true value is 1e-14 and that term is 1.5e-15, everywhere else it is far below the rest.
With GELU the pre-activation must be exact for this to be the whole error (dyadic data, below); where it is not (the float
family) its error d_lin passes through g with |g'| <= 1.13 (the maximum of the tanh-GELU derivative, 1.1289 at x = 1.46)."""
import functools
import math

import torch

import train_op_ref as R

U = R.U
K0 = -2.0 * R.KB * math.log2(math.e)
K1 = K0 * R.KK
GELU_SLOPE = 1.13

# integer operand ranges (those of tests/test_gpu_ops.py): |x| <= 3, |w| <= 2, |b| <= 4, |gate| <= 2, |res| <= 100
X_R, W_R, B_R, G_R, RES_R = 3, 2, 4, 2, 100


def worst_abs_sum(Cin):
    """Upper bound of every partial result on the integer operands: all of them must stay below 2^24 to be exact in fp32."""
    return G_R * (Cin * X_R * W_R + B_R) + RES_R


# ---------------------------------------------------------------------------------------------------------------- layout
def to_cb8(t):
    """NCDHW (C a multiple of 8) -> CB8 [N][C/8][Z][H][W][8]."""
    N, Cc, Z, H, W = t.shape
    return t.reshape(N, Cc // 8, 8, Z, H, W).permute(0, 1, 3, 4, 5, 2).contiguous()


def from_cb8(t):
    N, Cb, Z, H, W, _ = t.shape
    return t.permute(0, 1, 5, 2, 3, 4).reshape(N, Cb * 8, Z, H, W)


def cb(C):
    return (C + 7) // 8


def ntile_of(Cout):
    return (Cout + 63) // 64


def vox_of(N, Z, S):
    return N * Z * S * S


def conv1_form(vox, ntile, tile_variant):
    """launch_conv_mfma's rule for taps == 1 (conv1_form in tm_kernels.hip), restated: 1 = conv1_mfma<1, 2> (128 voxels x 64
    couts per workgroup), 2 = <2, 2> (256 x 64), 3 = <2, 4> (256 x 128), 0 = refused."""
    if tile_variant == 3:
        return 3 if ntile % 2 == 0 else 0
    variant = tile_variant if tile_variant else (2 if (vox // 256) * ntile >= 512 else 1)
    if variant == 2 and ntile % 2 == 0 and (vox // 256) * (ntile // 2) >= 512:
        return 3
    return 2 if variant == 2 else 1


def grid_of(vox, ntile, form):
    """Workgroups of the launch (xcd_swizzle remaps their ids: grids below 8 and grids that are no multiple of 8 matter)."""
    mv = 128 if form == 1 else 256
    return (vox + mv - 1) // mv * (ntile // 2 if form == 3 else ntile)


# ------------------------------------------------------------------------------------------------------------- the model
def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh_k(x, kk):
    return 0.5 * x * (1.0 + torch.tanh(R.KB * (x + kk * x ** 3)))


def up2(g):
    return g.repeat_interleave(2, -2).repeat_interleave(2, -1)


# the deliberate errors of `reference`; APPLIES says which case each one can be seen in
WRONG = ("gate_clip", "gate_swap_yx", "gate_z0", "gate_chunk_prev", "gate_chunk_next", "x_block_off", "gelu_after_gate",
         "res_times_gate", "erf_gelu", "no_bias", "swap_g4", "swap_halves128")


def _swap_couts(lin, span):
    """Output channel c takes the linear result of channel c ^ span (zero where that channel does not exist: the packed
    weights and the bias are zero padded)."""
    Cout = lin.shape[1]
    src = torch.arange(Cout) ^ span
    pad = torch.zeros_like(lin[:, :1])
    ext = torch.cat([lin, pad], 1)
    return ext[:, torch.where(src < Cout, src, torch.full_like(src, Cout))]


def reference(x, w, b, res, gate, gate_half, gelu, wrong=None, wide=None):
    """res + gate_up * act(W x + b) in float64.  x [N, Cin, Z, S, S], w [Cout, Cin], b [Cout], res [N, Cout, Z, S, S] or None,
    gate [N, Cout, Z, Sg, Sg] or None with Sg = S / 2 when gate_half (then repeated 2 x 2 in (H, W)), act = tanh-GELU when gelu.
    wrong: one of WRONG.  The slice errors need `wide` = the case dict of `make` (the tensors x and gate are slices of)."""
    assert wrong is None or wrong in WRONG
    x, w, b = x.double(), w.double(), b.double()
    Cin, Cout = w.shape[1], w.shape[0]
    if wrong == "x_block_off":
        c0 = wide["x_c0"] + 8
        x = wide["xw"][:, c0:c0 + Cin].double()
    lin = torch.einsum("oc,nczyx->nozyx", w, x)
    if wrong != "no_bias":
        lin = lin + b.view(1, -1, 1, 1, 1)
    if wrong == "swap_g4":
        lin = _swap_couts(lin, 32)
    if wrong == "swap_halves128":
        lin = _swap_couts(lin, 64)
    g = None
    if gate is not None:
        g = gate.double()
        if wrong in ("gate_chunk_prev", "gate_chunk_next"):
            c0 = wide["g_c0"] + (-8 if wrong == "gate_chunk_prev" else 8) * cb(Cout)
            g = wide["gw"][:, c0:c0 + Cout].double()
        if wrong == "gate_z0":
            g = g[:, :, :1].expand_as(g)
        if gate_half:
            if wrong == "gate_clip":
                S = x.shape[-1]
                idx = torch.arange(S).clamp_max(S // 2 - 1)
                g = g[..., idx, :][..., idx]
            else:
                g = up2(g)
        if wrong == "gate_swap_yx":
            g = g.transpose(-1, -2)
    act = (gelu_erf if wrong == "erf_gelu" else R.gelu_tanh) if gelu else (lambda t: t)
    if wrong == "gelu_after_gate":
        out = act(lin * g)
    else:
        out = act(lin)
        if g is not None:
            out = out * g
    if res is not None:
        out = (res.double() + out) * g if wrong == "res_times_gate" else res.double() + out
    return out


def preact(c):
    """The exact pre-activation W x + b of a case, float64."""
    return torch.einsum("oc,nczyx->nozyx", c["w"].double(), c["x"].double()) + c["b"].double().view(1, -1, 1, 1, 1)


def gelu_hw_bound(x):
    """|gelu_tanh_hw(x) - tanh-GELU(x)| for an exact fp32 x, float64 (the derivation is in the module docstring)."""
    x = x.double()
    ax = x.abs()
    dt = U * ax * (5 * abs(K0) + 8 * abs(K1) * x * x)
    e = torch.exp2(x * (K0 + K1 * x * x))
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (1.0 + e))
    rel = (math.log(2.0) * dt + 2 * U) * frac + 4 * U
    return rel * R.gelu_tanh(x).abs() + R.FLT_MIN + 2.0 ** -52 * ax


def gelu_hw_f32(x):
    """gelu_tanh_hw step by step in float32 (the fma as one rounding of the float64 value)."""
    x = x.float()
    k0 = torch.tensor(-2.0, dtype=torch.float32) * torch.tensor(R.KB, dtype=torch.float32) * torch.tensor(math.log2(math.e), dtype=torch.float32)
    k1 = k0 * torch.tensor(R.KK, dtype=torch.float32)
    p = x * x
    q = (p.double() * k1.double() + k0.double()).float()
    e = torch.exp2(x * q)
    return x * (1.0 / (1.0 + e))


def bound(c, exact_pre):
    """The fp32 error bound of a case's output, float64, same shape as the output.  exact_pre: the data make W x + b exact in
    fp32 (integer and dyadic cases): d_lin = 0."""
    x, w, b = c["x"].double(), c["w"].double(), c["b"].double()
    Kp = 8 * cb(w.shape[1])
    if exact_pre:
        d = torch.zeros_like(preact(c))
    else:
        mag = torch.einsum("oc,nczyx->nozyx", w.abs(), x.abs()) + b.abs().view(1, -1, 1, 1, 1)
        d = (Kp + 2) * U * mag
    if c["gelu"]:
        d = GELU_SLOPE * d + gelu_hw_bound(preact(c))
    if c["gate"] is None and c["res"] is None:
        return d
    out = reference(c["x"], c["w"], c["b"], c["res"], c["gate"], c["gate_half"], c["gelu"])
    g = torch.ones_like(out)
    if c["gate"] is not None:
        g = up2(c["gate"].double()) if c["gate_half"] else c["gate"].double()
    r = c["res"].double().abs() if c["res"] is not None else torch.zeros_like(out)
    return g.abs() * d + 2 * U * (r + out.abs())


def emulate_f32(c):
    """The same formula evaluated in float32 by torch (its own summation order): must lie inside `bound`."""
    lin = torch.einsum("oc,nczyx->nozyx", c["w"].float(), c["x"].float()) + c["b"].float().view(1, -1, 1, 1, 1)
    out = gelu_hw_f32(lin) if c["gelu"] else lin
    if c["gate"] is not None:
        out = out * (up2(c["gate"].float()) if c["gate_half"] else c["gate"].float())
    if c["res"] is not None:
        out = c["res"].float() + out
    return out


# ----------------------------------------------------------------------------------------------------------- case tables
# epilogue -> (gelu, gate, res, in_place, gate_half, x sliced, gate chunk of 7 (or None: a tensor of its own))
EPILOGUES = {
    "plain":                (0, 0, 0, 0, 0, 0, None),        # adaLN, kv, q
    "gelu":                 (1, 0, 0, 0, 0, 0, None),        # fc1
    "gate_res":             (0, 1, 1, 0, 0, 0, None),
    "gate_res_inplace":     (0, 1, 1, 1, 0, 0, None),        # proj, fc2: x <- x + gate * Linear(.)
    "gatehalf_res_inplace": (0, 1, 1, 1, 1, 0, None),
    "x_slice":              (0, 0, 0, 0, 0, 1, None),        # kv: x is a chunk of the conditioning tensor
    "gate_chunk2":          (0, 1, 1, 1, 0, 0, 2),           # the gates as the executor hands them over
    "gate_chunk6":          (0, 1, 1, 1, 0, 0, 6),
    "gatehalf_chunk2":      (0, 1, 1, 1, 1, 0, 2),
    "gatehalf_chunk6":      (0, 1, 1, 1, 1, 0, 6),
    "gelu_gate_res":        (1, 1, 1, 0, 0, 0, None),        # not launched by the model; the kernel takes it (order: GELU, then gate)
}
X_SLICE_CB0, X_SLICE_TAIL = 3, 2           # x slice: 3 blocks in front, 2 behind


def applies(wrong, epi, shape, form):
    """Can `wrong` be told from the right model in this case?  The host test requires a difference for every True."""
    gelu, gate, res, _, half, xs, chunk = EPILOGUES[epi]
    N, Cin, Cout, Z, S = shape
    Sg = S // 2 if half else S
    return {
        "gate_clip": bool(half) and S >= 4,             # at S = 2 both rules read the one gate voxel
        "gate_swap_yx": bool(gate) and Sg >= 2,
        "gate_z0": bool(gate) and Z > 1,
        "gate_chunk_prev": chunk is not None,
        "gate_chunk_next": chunk is not None and chunk < 6,
        "x_block_off": bool(xs),
        "gelu_after_gate": bool(gelu and gate),
        "res_times_gate": bool(gate and res),
        "erf_gelu": bool(gelu),
        "no_bias": True,
        "swap_g4": Cout > 32,
        "swap_halves128": form == 3,
    }[wrong]


# (N, Cin, Cout, Z, S)
#   voxels: 75 and 125 (N = 3 / 5, Z = 1, S = 5: a ragged tile of 128 AND of 256), 384 (ragged 256-voxel tile, three full 128s),
#           96 and 64 (less than one tile), 128 / 256 / 512 / 768 / 1536 (full tiles)
#   Cin:    13 and 229 (Cbi 2 and 29: no multiple of KC = 4), 40 (Cbi 5), 8 (one block), 32 (exactly one stage)
#   Cout:   72 (ntile 2, Cob 9: the second 64-tile and the one 128-tile ragged), 200 (ntile 4, Cob 25: ragged 64- and 128-tile),
#           128, 1792 (ntile 28), 37 and 100 (3 and 4 pad slots in the last block; 37: ntile 1, no 128-cout form)
#   grids:  from 1 workgroup (75 voxels, form 3 at Cout 72) to 28; 12 and 28 are no multiple of 8
SHAPES = [
    (3, 13, 72, 1, 5), (5, 13, 200, 1, 5), (3, 229, 200, 2, 8), (2, 40, 128, 4, 4), (2, 8, 37, 8, 4), (1, 32, 1792, 1, 8),
    (3, 13, 100, 2, 16), (3, 40, 72, 8, 2), (2, 13, 128, 1, 16), (3, 229, 72, 4, 8),
]
GELU_GATE_SHAPES = [(3, 13, 72, 1, 5), (3, 229, 200, 2, 8)]
FLOAT_SHAPES = [(3, 229, 200, 2, 8), (3, 13, 100, 2, 16), (3, 40, 72, 8, 2)]
# the automatic choice, N = 1, Z = 2, S = 64 (8192 voxels = 32 tiles of 256), Cin = 8: Cout -> form
#   2048: ntile 32, 32 * 16 = 512 exactly -> 3;   1984: ntile 31 (odd) -> 2;   1920: ntile 30, 32 * 15 = 480 -> 2;
#   1024: ntile 16, 32 * 16 = 512 exactly -> 256-voxel tiles, 32 * 8 = 256 -> 2;   960: ntile 15, 32 * 15 = 480 < 512 -> 1
AUTO_CASES = [((1, 8, 2048, 2, 64), 3), ((1, 8, 1984, 2, 64), 2), ((1, 8, 1920, 2, 64), 2), ((1, 8, 1024, 2, 64), 2),
              ((1, 8, 960, 2, 64), 1)]


def half_ok(S):
    return S >= 2 and S & (S - 1) == 0


def variants_of(shape):
    return (1, 2, 3) if ntile_of(shape[2]) % 2 == 0 else (1, 2)


def epilogues_of(shape):
    out = []
    for e, (gelu, gate, res, inpl, half, xs, chunk) in EPILOGUES.items():
        if half and not half_ok(shape[4]):
            continue
        if e == "gelu_gate_res" and shape not in GELU_GATE_SHAPES:
            continue
        out.append(e)
    return out


def int_cases():
    """(shape, epilogue, tile_variant) of every case held bit for bit (no GELU)."""
    return [(s, e, v) for s in SHAPES for e in epilogues_of(s) if not EPILOGUES[e][0] for v in variants_of(s)]


def gelu_cases():
    """(shape, epilogue, tile_variant): dyadic data, exact pre-activation, held to the GELU bound."""
    return [(s, e, v) for s in SHAPES for e in epilogues_of(s) if EPILOGUES[e][0] for v in variants_of(s)]


def float_cases():
    return [(s, e, v) for s in FLOAT_SHAPES for e in epilogues_of(s) for v in variants_of(s)]


def case_id(c):
    s, e, v = c
    return "-".join(map(str, s)) + f"-{e}-v{v}"


def _ints(shape, r, g):
    return torch.randint(-r, r + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=8)
def make(shape, epi, kind):
    """The data of one case (shared by its tile variants; treat as read-only): dict with the model's tensors x, w, b, res, gate
    (float64 NCDHW; res / gate None where the epilogue has none), the wide tensors xw / gw they are slices of with their first
    channel x_c0 / g_c0, and the switches.  kind: "int" (integers; GELU epilogues: x in multiples of 1/8 and one nonzero
    input channel, so that W x + b is an exact dyadic in [-7, 7]) or "float" (randn)."""
    gelu, gate, res, inpl, half, xs, chunk = EPILOGUES[epi]
    N, Cin, Cout, Z, S = shape
    g = torch.Generator().manual_seed(1000 * Cin + Cout + 7 * Z + S + len(epi))
    Cbi, Cob = cb(Cin), cb(Cout)
    x_cb0 = X_SLICE_CB0 if xs else 0
    x_cbtot = x_cb0 + Cbi + (X_SLICE_TAIL if xs else 0)
    Sg = S // 2 if half else S
    g_cb0 = chunk * Cob if chunk is not None else 0
    g_cbtot = 7 * Cob if chunk is not None else Cob
    if kind == "int":
        assert worst_abs_sum(Cin) < 2 ** 24
        xw = _ints((N, x_cbtot * 8, Z, S, S), X_R, g)
        w, b = _ints((Cout, Cin), W_R, g), _ints((Cout,), B_R, g)
        gw = _ints((N, g_cbtot * 8, Z, Sg, Sg), G_R, g) if gate else None
        r = _ints((N, Cout, Z, S, S), RES_R, g) if res else None
        if gelu:
            xw = _ints((N, x_cbtot * 8, Z, S, S), 8 * X_R, g) / 8
            w[:, 1:] = 0
            w[:, 0] = torch.where(w[:, 0] >= 0, 1.0, -1.0).double()
    else:
        rn = lambda shp: torch.randn(shp, generator=g).double().float().double()      # fp32 values
        xw = rn((N, x_cbtot * 8, Z, S, S))
        w, b = (rn((Cout, Cin)) / math.sqrt(Cin)).float().double(), rn((Cout,))
        gw = rn((N, g_cbtot * 8, Z, Sg, Sg)) if gate else None
        r = rn((N, Cout, Z, S, S)) if res else None
    # pad channels of the slices' last blocks are zero (CB8 keeps pad slots at exactly 0)
    x_c0 = x_cb0 * 8
    xw[:, x_c0 + Cin:x_c0 + Cbi * 8] = 0
    if gate:
        gw[:, g_cb0 * 8 + Cout:(g_cb0 + Cob) * 8] = 0
    return {"shape": shape, "epi": epi, "x": xw[:, x_c0:x_c0 + Cin], "w": w, "b": b, "res": r,
            "gate": gw[:, g_cb0 * 8:g_cb0 * 8 + Cout] if gate else None, "gate_half": bool(half), "gelu": bool(gelu),
            "in_place": bool(inpl), "xw": xw, "x_c0": x_c0, "x_cb0": x_cb0, "x_cbtot": x_cbtot,
            "gw": gw, "g_c0": g_cb0 * 8, "g_cb0": g_cb0, "g_cbtot": g_cbtot}


def ref_of(c):
    return reference(c["x"], c["w"], c["b"], c["res"], c["gate"], c["gate_half"], c["gelu"])


# ---- 16-bit 1x1 conv with the gate at half resolution, as chunk 2 of 7: (N, Cin, Cout, Z, S) ----
H16_GATE_CASES = [(3, 13, 40, 1, 4), (2, 229, 200, 2, 8), (1, 96, 64, 4, 16), (3, 40, 72, 2, 4), (2, 24, 128, 4, 8)]
