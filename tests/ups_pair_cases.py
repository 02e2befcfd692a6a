"""Cases, reference and error bound of the pair form of the fp32 upsampled-input conv (conv3d_zpair_ups, hook
tm_op_conv_ups_pair_f32): y = conv3d(nearest-x2 upsampled x, w, pad 1) + b at Z = 2, computed on the low-resolution x.

Per output phase (py, px) the 3 x 3 in-plane taps collapse onto a 2 x 2 window of x; the window weights V_kz are SUMS of up to
four taps (formed in fp32 at pack time), the pair form then differences them in z (V2 - V1, V0 - V1) and the kernel runs
P1 = V1 * (X0 + X1), P2 = (V2 - V1) * X1, P3 = (V0 - V1) * X0, Y0 = P1 + P2, Y1 = P1 + P3.

BOUND (the pair-form bound of tests/test_gpu_conv_zpair.py with the window in place of the 3 x 3 taps): (L + c) U mag with
  L = 8 ceil(Cin / 8) * 4 + 1   the fixed fp32 accumulation chain of one product over the padded Cin x 4 window taps, plus the
                                final add of two products;
  c = 7                         roundings outside the chain: the phase sum of up to four taps (3), the z difference (1), the plane
                                add X0 + X1 (1), the bias add (1), and 1 for the second-order terms;
  mag                           the three-product expression on absolute values in float64, which in terms of the ORIGINAL taps
                                is bounded by |W1| * (|X0| + |X1|) + (|W2| + |W1|) * |X1| + |b| on the upsampled |x| (plane 0;
                                plane 1 with W0, X0): sums of absolute values only grow when the window sums are split up.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24

# (Cin, Cout, S_in, N): Z = 2.  Cin 8 is one cin block (the last-block instantiation alone), 37 leaves pad channels, 128 runs
# 16 blocks through both weight slots; Cout 128 has two cout tiles; S_in 4 / 8 / 16 take the 4-, 8- and 16-wide tiles
CASES = [(8, 64, 4, 1), (37, 64, 4, 1), (128, 128, 4, 2), (8, 64, 8, 1), (37, 64, 8, 1), (128, 128, 8, 2),
         (8, 64, 16, 1), (37, 64, 16, 1), (128, 128, 16, 2)]


def case_id(c):
    return "Cin%d-Cout%d-S%d-N%d" % c


def up2(x):
    return x.repeat_interleave(2, dim=-1).repeat_interleave(2, dim=-2)


def make(case, kind):
    Cin, Cout, S, N = case
    g = torch.Generator().manual_seed(2000 + Cin * 5 + Cout + S * 13 + N)
    if kind == "int":
        x = torch.randint(-3, 4, (N, Cin, 2, S, S), generator=g).float()
        w = torch.randint(-2, 3, (Cout, Cin, 3, 3, 3), generator=g).float()
        b = torch.randint(-4, 5, (Cout,), generator=g).float()
    else:
        x = torch.randn((N, Cin, 2, S, S), generator=g)
        w = torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5
        b = torch.randn((Cout,), generator=g)
    return {"case": case, "x": x, "w": w, "b": b}


def reference(c, dtype=torch.float64):
    return F.conv3d(up2(c["x"]).to(dtype), c["w"].to(dtype), c["b"].to(dtype), padding=1)


def bound(c):
    x, w, b = up2(c["x"]), c["w"], c["b"]
    Cin = x.shape[1]
    L = (Cin + 7) // 8 * 8 * 4 + 1
    xa, wa = x.double().abs(), w.double().abs()
    x0, x1 = xa[:, :, 0], xa[:, :, 1]
    w0, w1, w2 = wa[:, :, 0], wa[:, :, 1], wa[:, :, 2]
    p1 = F.conv2d(x0 + x1, w1, padding=1)
    m0 = p1 + F.conv2d(x1, w2 + w1, padding=1)
    m1 = p1 + F.conv2d(x0, w0 + w1, padding=1)
    mag = torch.stack([m0, m1], dim=2) + b.double().abs().view(1, -1, 1, 1, 1)
    return (L + 7) * U * mag


def pair_f32(c):
    """The kernel's arithmetic in float32 on the CPU: phase sums, z differences, three 2 x 2 products per phase."""
    x, w, b = c["x"], c["w"], c["b"]
    N, Cin, _, S, _ = x.shape
    Cout = w.shape[0]
    G0 = (((0, 0), (1, 2)), ((0, 1), (2, 2)))
    y = torch.zeros((N, Cout, 2, 2 * S, 2 * S))
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            v = torch.zeros((3, Cout, Cin, 2, 2))
            for wy in range(2):
                for wx in range(2):
                    for ky in range(G0[py][wy][0], G0[py][wy][1] + 1):
                        for kx in range(G0[px][wx][0], G0[px][wx][1] + 1):
                            v[:, :, :, wy, wx] += w[:, :, :, ky, kx].permute(2, 0, 1)
            win = xp[:, :, :, py:py + S + 1, px:px + S + 1]
            x0, x1 = win[:, :, 0], win[:, :, 1]
            p1 = F.conv2d(x0 + x1, v[1])
            p2 = F.conv2d(x1, v[2] - v[1])
            p3 = F.conv2d(x0, v[0] - v[1])
            y[:, :, 0, py::2, px::2] = p1 + p2
            y[:, :, 1, py::2, px::2] = p1 + p3
    return y + b.view(1, -1, 1, 1, 1)
