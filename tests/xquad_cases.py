"""Cases, float64 model and error bound of the x-quad form of the fp32 3x3x3 pad-1 conv at Z = 2 (conv3d_xquad, hook
tm_op_conv_xquad_f32): the pair form in z composed with the 1-D Winograd identity F(4,3) along x.  Shared by
tests/test_xquad_host.py (no GPU) and tests/test_gpu_xquad.py.

THE IDENTITY.  W0, W1, W2 the kz slices, X0, X1 the two input planes.  Products p = 1, 2, 3 use the filters V(1) = W1,
V(2) = W2 - W1, V(3) = W0 - W1 on the planes Xs(1) = X0 + X1, Xs(2) = X1, Xs(3) = X0.  For a filter row ky with taps g0, g1, g2
    U0 = g0 / 4    U1 = -((g0 + g1) + g2) / 6    U2 = -((g0 - g1) + g2) / 6
    U3 = (g0 / 24 + g1 / 12) + g2 / 6    U4 = (g0 / 24 - g1 / 12) + g2 / 6    U5 = g2                       (pack time)
and for group j (output columns 4j .. 4j + 3) with d0 .. d5 the columns 4j - 1 .. 4j + 4 of a row of Xs(p) (zero outside)
    T0 = (4 d0 - 5 d2) + d4    T1 = (d3 + d4) - 4 (d1 + d2)    T2 = 4 (d1 - d2) - (d3 - d4)
    T3 = 2 (d3 - d1) + (d4 - d2)    T4 = 2 (d1 - d3) + (d4 - d2)    T5 = (4 d1 - 5 d3) + d5                 (staging)
    A_q(p)[y][j] = sum over cin, ky of U_q(p)[ky] T_q(p)[y + ky - 1][j]                                     (the accumulators)
    s = A1 + A2    d = A1 - A2    s' = A3 + A4    d' = A3 - A4
    P(p)[y][4j .. 4j + 3] = (A0 + s) + s',  d + 2 d',  s + 4 s',  (d + 8 d') + A5
    Y0 = P(1) + P(2)    Y1 = P(1) + P(3)    (+ bias, + residual)

BOUND on |y - float64 reference| per output element, first order in U = 2^-24, times SECOND for the (1 + U)^n tails:
    (L + c) U mag
  L = 8 ceil(Cin / 8) * 3   the fp32 accumulation chain of one accumulator A_q(p): padded cin x three filter rows, one rounding
                            per term (every partial sum is bounded by the sum of absolute values, which mag holds);
  c = 15 (+ 1 with a residual), the most roundings outside the chain that one term passes through:
        4  pack time: the z difference V (1); the filter transform, at most three per tap (U1 / U2: two adds and the division
           by 6; U3 / U4: a division, two adds; the other divisions of a sum belong to other taps);
        4  staging: the plane add X0 + X1 (1); the input transform, at most three per column (T0 / T5: the product by 5, the
           difference, the add; multiplications by 2 and 4 are exact);
        1  the product U T, should the matrix unit round it before it is added;
        3  the output transform: A1 passes s (or d), A0 + s (or d + 8 d'), and the last add; 2, 4 and 8 are exact;
        1  the plane sum P(1) + P(2 | 3);   1  the bias add;   1  the second-order terms;
  mag   the whole expression on absolute values in float64, every coefficient by its absolute value (the input transform's
        rows sum to at most 10, the output transform's to at most 18): |V(1)| = |W1|, |V(2)| = |W2| + |W1|, |V(3)| = |W0| +
        |W1|; |U_q| and |T_q| from them; the four column sums of |A_q|; both products of the plane; plus |b| (+ |res|).
No measured tolerance enters: tests print the worst error / bound.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SECOND = 1.001

# (Cin, Cout, S, N, res): Z = 2, always with a bias.  res: 0 none, 1 the output's geometry, 2 half resolution (res_half).
#  S = 8 has only edge groups (two per row) and several patches per workgroup, S = 16 interior groups, S = 32 tile borders in x
#  and y; N = 1 and 3 leave missing patches behind the patch guard; Cin 5: pad channels in the only block; Cin 37: five blocks, an
#  odd count of products in the two-slot ring; Cout 37: a partial second 32-cout tile; Cout 128: four tiles.
SHAPES = [(ci, co, S, N) for S in (8, 16, 32) for N in (1, 3) for (ci, co) in ((5, 37), (37, 128))]
CASES = [s + (r,) for s in SHAPES for r in (0, 1, 2)]
WRONG = ["t0_5_to_4", "y3_8_to_4"]


def case_id(c):
    return "Cin%d-Cout%d-S%d-N%d-r%d" % c


def make(case, kind):
    Cin, Cout, S, N, res = case
    g = torch.Generator().manual_seed(4300 + Cin * 5 + Cout * 3 + S * 13 + N * 7 + 2 * res)
    Sr = S // 2 if res == 2 else S
    if kind == "int":                                # weights 24 x small integers: the filter transform is exact
        x = torch.randint(-3, 4, (N, Cin, 2, S, S), generator=g).float()
        w = 24.0 * torch.randint(-1, 2, (Cout, Cin, 3, 3, 3), generator=g).float()
        b = torch.randint(-4, 5, (Cout,), generator=g).float()
        r = torch.randint(-9, 10, (N, Cout, 2, Sr, Sr), generator=g).float()
    else:
        x = torch.randn((N, Cin, 2, S, S), generator=g)
        w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5
        b = torch.randn((Cout,), generator=g)
        r = torch.randn((N, Cout, 2, Sr, Sr), generator=g)
    return {"case": case, "x": x, "w": w, "b": b, "res": r if res else None, "res_half": res == 2}


def up2(x):
    return x.repeat_interleave(2, dim=-1).repeat_interleave(2, dim=-2)


def residual(c, dtype=torch.float64):
    if c["res"] is None:
        return None
    r = c["res"].to(dtype)
    return up2(r) if c["res_half"] else r


def reference(c, dtype=torch.float64):
    y = F.conv3d(c["x"].to(dtype), c["w"].to(dtype), c["b"].to(dtype), padding=1)
    r = residual(c, dtype)
    return y if r is None else r + y


def filters(w, absolute=False):
    """U[p][q]: [Cout, Cin, 3 (ky)] for the three products, in w's dtype, in the pack's association."""
    w0, w1, w2 = w[:, :, 0], w[:, :, 1], w[:, :, 2]
    V = [w1, w2 + w1, w0 + w1] if absolute else [w1, w2 - w1, w0 - w1]
    out = []
    for g in V:
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
        if absolute:
            u1 = ((g0 + g1) + g2) / 6
            u3 = (g0 / 24 + g1 / 12) + g2 / 6
            out.append([g0 / 4, u1, u1, u3, u3, g2])
        else:
            out.append([g0 / 4, -((g0 + g1) + g2) / 6, -((g0 - g1) + g2) / 6,
                        (g0 / 24 + g1 / 12) + g2 / 6, (g0 / 24 - g1 / 12) + g2 / 6, g2])
    return out


def transforms(xs, wrong=None, absolute=False):
    """T[q]: [N, Cin, S + 2 (zero halo rows), S / 4] of one plane xs [N, Cin, S, S]."""
    S = xs.shape[-1]
    xp = F.pad(xs, (1, 1, 1, 1))
    d = [xp[..., k:k + S:4] for k in range(6)]       # columns 4j - 1 .. 4j + 4
    if absolute:
        return [4 * d[0] + 5 * d[2] + d[4], 4 * (d[1] + d[2]) + (d[3] + d[4]), 4 * (d[1] + d[2]) + (d[3] + d[4]),
                2 * (d[3] + d[1]) + (d[4] + d[2]), 2 * (d[1] + d[3]) + (d[4] + d[2]), 4 * d[1] + 5 * d[3] + d[5]]
    five = 4 if wrong == "t0_5_to_4" else 5
    return [(4 * d[0] - five * d[2]) + d[4], (d[3] + d[4]) - 4 * (d[1] + d[2]), 4 * (d[1] - d[2]) - (d[3] - d[4]),
            2 * (d[3] - d[1]) + (d[4] - d[2]), 2 * (d[1] - d[3]) + (d[4] - d[2]), (4 * d[1] - 5 * d[3]) + d[5]]


def _a(u, t):
    """sum over cin, ky of u[ky] t[y + ky - 1]: [N, Cout, S, S / 4]"""
    return F.conv2d(t, u.unsqueeze(-1))


def _columns(A, wrong=None, absolute=False):
    if absolute:
        s, sp = A[1] + A[2], A[3] + A[4]
        return [A[0] + s + sp, s + 2 * sp, s + 4 * sp, s + 8 * sp + A[5]]
    s, d, sp, dp = A[1] + A[2], A[1] - A[2], A[3] + A[4], A[3] - A[4]
    eight = 4 if wrong == "y3_8_to_4" else 8
    return [(A[0] + s) + sp, d + 2 * dp, s + 4 * sp, (d + eight * dp) + A[5]]


def _planes(c, dtype, wrong, absolute):
    x, w = c["x"].to(dtype), c["w"].to(dtype)
    if absolute:
        x, w = x.abs(), w.abs()
    N, _, _, S, _ = x.shape
    Cout = w.shape[0]
    Uf = filters(w, absolute)
    planes = [x[:, :, 0] + x[:, :, 1], x[:, :, 1], x[:, :, 0]]
    P = []
    for p in range(3):
        T = transforms(planes[p], wrong, absolute)
        A = [_a(Uf[p][q], T[q]) for q in range(6)]
        P.append(torch.stack(_columns(A, wrong, absolute), dim=-1).reshape(N, Cout, S, S))
    return torch.stack([P[0] + P[1], P[0] + P[2]], dim=2)


def model(c, dtype=torch.float64, wrong=None):
    """The identity of the module docstring in `dtype`, term for term (torch's own order inside each A_q)."""
    y = _planes(c, dtype, wrong, False) + c["b"].to(dtype).view(1, -1, 1, 1, 1)
    r = residual(c, dtype)
    return y if r is None else r + y


def magnitude(c):
    """mag of the module docstring: no intermediate of the computation exceeds it in absolute value"""
    mag = _planes(c, torch.float64, None, True) + c["b"].double().abs().view(1, -1, 1, 1, 1)
    r = residual(c)
    return mag if r is None else mag + r.abs()


def bound(c):
    Cin = c["x"].shape[1]
    L = (Cin + 7) // 8 * 8 * 3
    return SECOND * (L + 15 + (1 if c["res"] is not None else 0)) * U * magnitude(c)


def worst(d, bnd):
    return float((d / bnd).max())
