"""Cases, float64 model and error bound of the x-pair form of the fp32 3x3x3 pad-1 conv at Z = 2: the pair form in z composed
with the 1-D Winograd identity F(2,3) along x.  The kernel that ran it (conv3d_xpair) is retired (profiles/conv_xpair_retired.txt);
tests/test_xpair_host.py (no GPU, no library) checks the model, and tests/test_gpu_conv_frag_layout.py takes its operands from make.

THE IDENTITY.  W0, W1, W2 the kz slices, X0, X1 the two input planes.  Products p = 1, 2, 3 use the filters V(1) = W1,
V(2) = W2 - W1, V(3) = W0 - W1 on the planes Xs(1) = X0 + X1, Xs(2) = X1, Xs(3) = X0.  For a filter row ky with taps g0, g1, g2
    U0 = g0    U1 = (g0 + g1 + g2) / 2    U2 = (g0 - g1 + g2) / 2    U3 = g2                      (pack time)
and for x-pair j (output columns 2j, 2j + 1) with d0 .. d3 the columns 2j - 1 .. 2j + 2 of a row of Xs(p) (zero outside the plane)
    T0 = d0 - d2    T1 = d1 + d2    T2 = d2 - d1    T3 = d1 - d3                                  (staging)
    A_q(p)[y][j] = sum over cin, ky of U_q(p)[ky] T_q(p)[y + ky - 1][j]                             (the MFMA accumulators)
    P(p)[y][2j] = (A0 + A1) + A2    P(p)[y][2j + 1] = (A1 - A2) - A3    Y0 = P(1) + P(2)    Y1 = P(1) + P(3)    (+ bias, + residual)

BOUND on |y - float64 reference| per output element, first order in U = 2^-24, times SECOND for the (1 + U)^n tails:
    (L + c) U mag
  L = 8 ceil(Cin / 8) * 3   the fp32 accumulation chain of one accumulator A_q(p): padded cin x three filter rows, one rounding
                            per term (every partial sum is bounded by the sum of absolute values, mag);
  c = 11 (+ 1 with a residual), the roundings outside the chain that a term passes through:
        3  the pack-time sums: the z difference V (1), the two adds of U1 / U2 (the halving is exact);
        2  staging: the plane add X0 + X1 (1) and the difference / sum T (1);
        1  the product U T, should the matrix unit round it before it is added;
        2  the output transform (A0 + A1) + A2 or (A1 - A2) - A3;
        1  the plane sum P(1) + P(2 | 3);   1  the bias add;   1  the second-order terms;
  mag   the whole expression on absolute values in float64: |V(1)| = |W1|, |V(2)| = |W2| + |W1|, |V(3)| = |W0| + |W1|;
        |U0| = |g0|, |U1| = |U2| = (|g0| + |g1| + |g2|) / 2, |U3| = |g2|; |Xs(1)| = |X0| + |X1|; |T_q| = the sum of its two
        |d|; the three (even column) or three (odd column) |U_q| * |T_q| sums of both products of the plane, plus |b| (+ |res|).
No measured tolerance enters: tests print the worst error / bound.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SECOND = 1.001

# (Cin, Cout, S, N, bias, res): Z = 2.  res: 0 none, 1 the output's geometry, 2 half resolution (res_half).
#  S = 8: two patches per 128-voxel workgroup, N = 1 and 3 leave a missing patch; S = 16: one 128-voxel tile per plane (two
#  64-voxel ones); S = 32: tile borders in x and y.  Cin 8 / 16 / 24 / 37 / 96: 1, 2, 3, 5, 12 cin blocks (the last-block
#  instantiation alone, both ring parities of the product slots, pad channels).  Cout 32 / 37 / 64 / 128: output pad slots, two
#  cout tiles.
CASES = [(8, 32, 8, 1, 1, 0), (16, 37, 8, 3, 1, 1), (96, 128, 8, 3, 0, 2), (24, 64, 16, 1, 1, 2), (37, 128, 16, 2, 0, 0),
         (16, 32, 16, 1, 1, 1), (96, 64, 32, 1, 1, 1), (37, 37, 32, 1, 0, 2), (8, 64, 32, 2, 1, 0)]
# the cases a float32 evaluation on the CPU in the kernel's order runs (every mechanism of the arithmetic; small enough for numpy)
HOST_CASES = [(8, 32, 8, 1, 1, 0), (16, 37, 8, 3, 1, 1), (24, 64, 16, 1, 1, 2), (37, 37, 32, 1, 0, 2)]
WRONG = ["swap_u1_u2", "no_half", "t3_from_d2_d3", "odd_plus_a3", "planes_swapped", "halo_not_zeroed"]


def case_id(c):
    return "Cin%d-Cout%d-S%d-N%d-b%d-r%d" % c


def make(case, kind):
    Cin, Cout, S, N, bias, res = case
    g = torch.Generator().manual_seed(3000 + Cin * 5 + Cout * 3 + S * 13 + N * 7 + bias + 2 * res)
    Sr = S // 2 if res == 2 else S
    if kind == "int":
        x = torch.randint(-8, 9, (N, Cin, 2, S, S), generator=g).float()
        w = torch.randint(-4, 5, (Cout, Cin, 3, 3, 3), generator=g).float()
        b = torch.randint(-4, 5, (Cout,), generator=g).float()
        r = torch.randint(-9, 10, (N, Cout, 2, Sr, Sr), generator=g).float()
    else:
        x = torch.randn((N, Cin, 2, S, S), generator=g)
        w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5
        b = torch.randn((Cout,), generator=g)
        r = torch.randn((N, Cout, 2, Sr, Sr), generator=g)
    if not bias:
        b = torch.zeros(Cout)
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


def filters(w, wrong=None, absolute=False):
    """U[p][q]: [Cout, Cin, 3 (ky)] for the three products, in w's dtype, rounded as the pack does (differences, then sums)."""
    w0, w1, w2 = w[:, :, 0], w[:, :, 1], w[:, :, 2]
    V = [w1, w2 + w1, w0 + w1] if absolute else [w1, w2 - w1, w0 - w1]
    out = []
    for g in V:
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
        half = 1.0 if wrong == "no_half" else 0.5
        u1 = ((g0 + g1) + g2) * half
        u2 = u1 if absolute else ((g0 - g1) + g2) * half
        if wrong == "swap_u1_u2":
            u1, u2 = u2, u1
        out.append([g0, u1, u2, g2])
    return out


def transforms(xs, wrong=None, absolute=False):
    """T[q]: [N, Cin, S + 2 (zero halo rows), S / 2] of one plane xs [N, Cin, S, S]."""
    S = xs.shape[-1]
    xp = F.pad(xs, (1, 1, 1, 1))
    if wrong == "halo_not_zeroed":                   # the columns -1 and S repeat their neighbours
        xp[..., 0] = xp[..., 1]
        xp[..., S + 1] = xp[..., S]
    d = [xp[..., k:k + S:2] for k in range(4)]       # columns 2j - 1 .. 2j + 2
    if absolute:
        return [d[0] + d[2], d[1] + d[2], d[2] + d[1], d[1] + d[3]]
    t3 = d[2] - d[3] if wrong == "t3_from_d2_d3" else d[1] - d[3]
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], t3]


def _a(u, t):
    """sum over cin, ky of u[ky] t[y + ky - 1]: [N, Cout, S, S / 2]"""
    return F.conv2d(t, u.unsqueeze(-1))


def model(c, dtype=torch.float64, wrong=None):
    """The identity of the module docstring in `dtype`, term for term (torch's own order inside each A_q)."""
    x, w, b = c["x"].to(dtype), c["w"].to(dtype), c["b"].to(dtype)
    N, _, _, S, _ = x.shape
    Cout = w.shape[0]
    Uf = filters(w, wrong)
    planes = [x[:, :, 0] + x[:, :, 1], x[:, :, 1], x[:, :, 0]]
    P = []
    for p in range(3):
        T = transforms(planes[p], wrong)
        A = [_a(Uf[p][q], T[q]) for q in range(4)]
        even = (A[0] + A[1]) + A[2]
        odd = (A[1] - A[2]) + A[3] if wrong == "odd_plus_a3" else (A[1] - A[2]) - A[3]
        P.append(torch.stack([even, odd], dim=-1).reshape(N, Cout, S, S))
    y0, y1 = P[0] + P[1], P[0] + P[2]
    if wrong == "planes_swapped":
        y0, y1 = y1, y0
    y = torch.stack([y0, y1], dim=2) + b.view(1, -1, 1, 1, 1)
    r = residual(c, dtype)
    return y if r is None else r + y


def bound(c):
    xa, wa = c["x"].double().abs(), c["w"].double().abs()
    N, Cin, _, S, _ = xa.shape
    Cout = wa.shape[0]
    Uf = filters(wa, absolute=True)
    planes = [xa[:, :, 0] + xa[:, :, 1], xa[:, :, 1], xa[:, :, 0]]
    M = []
    for p in range(3):
        T = transforms(planes[p], absolute=True)
        A = [_a(Uf[p][q], T[q]) for q in range(4)]
        M.append(torch.stack([A[0] + A[1] + A[2], A[1] + A[2] + A[3]], dim=-1).reshape(N, Cout, S, S))
    mag = torch.stack([M[0] + M[1], M[0] + M[2]], dim=2) + c["b"].double().abs().view(1, -1, 1, 1, 1)
    r = residual(c)
    if r is not None:
        mag = mag + r.abs()
    L = (Cin + 7) // 8 * 8 * 3
    return SECOND * (L + 11 + (1 if r is not None else 0)) * U * mag


def kernel_order_f32(c):
    """float32 numpy evaluation in the kernel's order: per accumulator A_q(p) the chain runs cin block, ky, k with k pairing
    the channels (k, 4 + k) of a block as one MFMA does; products and sums rounded to float32 one by one."""
    f = np.float32
    x, w, b = c["x"].numpy().astype(f), c["w"].numpy().astype(f), c["b"].numpy().astype(f)
    N, Cin, _, S, _ = x.shape
    Cout = w.shape[0]
    Cp = (Cin + 7) // 8 * 8
    xpad = np.zeros((N, Cp, 2, S, S), f); xpad[:, :Cin] = x
    wpad = np.zeros((Cout, Cp, 3, 3, 3), f); wpad[:, :Cin] = w
    Uf = [[u.numpy() for u in pu] for pu in filters(torch.from_numpy(wpad))]
    planes = [xpad[:, :, 0] + xpad[:, :, 1], xpad[:, :, 1], xpad[:, :, 0]]
    P = []
    for p in range(3):
        T = [t.numpy() for t in transforms(torch.from_numpy(planes[p]))]
        A = []
        for q in range(4):
            acc = np.zeros((N, Cout, S, S // 2), f)
            for cb in range(Cp // 8):
                for ky in range(3):
                    for k in range(4):
                        for ch in (cb * 8 + k, cb * 8 + 4 + k):
                            acc = acc + Uf[p][q][None, :, ch, ky, None, None] * T[q][:, None, ch, ky:ky + S, :]
            A.append(acc)
        even = (A[0] + A[1]) + A[2]
        odd = (A[1] - A[2]) - A[3]
        P.append(np.stack([even, odd], axis=-1).reshape(N, Cout, S, S))
    y = np.stack([P[0] + P[1], P[0] + P[2]], axis=2) + b.reshape(1, -1, 1, 1, 1)
    r = residual(c, torch.float32)
    y = torch.from_numpy(y.astype(f))
    return y if r is None else r + y


def worst(d, bnd):
    return float((d / bnd).max())
