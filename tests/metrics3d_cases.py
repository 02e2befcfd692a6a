"""Shared by tests/test_metrics3d_cases_host.py and tests/test_gpu_metrics3d.py: the 5-D measures of the reference's
utils/metrics.py:236-439 (the 3-D window of `_ssim`, `avg_pool3d`, 5-D `ms_ssim` with its skipped-depth levels) restated in
float64 numpy (held to the reference itself through tests/golden/metrics3d_ref.npz, minted by tools/make_metrics3d_golden.py),
the seeded cases, a float32 walk in the order of operations of ssim_volumes_kernel (tm_metrics.hip), and the error bound of
that order.  The plane route and everything it shares are metrics_cases.py's.

THE BOUND (first order in U = 2^-24), per output voxel, as the docstring of metrics_cases.py derives it for two passes.  With
the tile's shifts cx, cy (x and y at the tile's first voxel of plane 0), a = x - cx, b = y - cy, F the exact separable filter
with the float32 taps along columns, rows and depth:
  * each of m1 = F a, m2 = F b, q11 = F a^2, q22 = F b^2, q12 = F ab is THREE dot products of n terms (one FMA, one rounding,
    per tap; the zero taps behind a shorter window add exactly nothing), every term a product that carries up to 3 roundings:
    |err| <= G F|.|,  G = (3 n + 3) U;
  * mu1 = m1 + cx S and the shift corrections of s1, s2, s12 exactly as in two dimensions, with S = (sum of the taps)^3, the
    weight of the n^3 window, and d = 1 - S, both from double and rounded once;
  * cs, lum, ssim: as in two dimensions;
then the mean of the per-voxel bounds.  A lane owns ONE output per plane, so its float32 partial sum has a single term and
adds no rounding (LANE_ADDS = 0); everything above is float64 (2^-50 relative), and U |mean| for the float32 result.
A level of 5-D MS-SSIM that is shallower than the window goes through the plane kernel: its bound is metrics_cases.bound per
plane, averaged.  MS-SSIM: the interval of the product of the weighted powers over the per-level bounds, plus 32 U.
Nothing here was tuned on what the kernel returns.
"""
import zlib

import numpy as np

import metrics_cases as mc

TW, TH = 16, 16                    # tm_kernels.h SSIM3_TW, SSIM3_TH
LANE_ADDS = 0                      # float32 additions a lane makes over its own outputs: it owns one per plane
MAX_TAPS = 11                      # SSIM3_TAPS
U, f32 = mc.U, np.float32
N, C = 2, 2
WIN, SIGMA, K = mc.WIN, mc.SIGMA, mc.K
KINDS = mc.KINDS
TILE_PLUS_ONE = (13, TH + WIN, TW + WIN)      # the valid output exceeds one 16 x 16 tile by one row and one column; 3 planes deep
SHAPES = ((11, 11, 11), (12, 12, 37), TILE_PLUS_ONE)          # the depth is not chunked: one workgroup marches over every plane
CASES = [(k, s) for k in KINDS for s in SHAPES]
# 5-D MS-SSIM, N = 1, C = 2.  (50, 176, 163): depths 50, 25, 13, 7, 4 (3-D window at levels 0-2, planes at 3-4, 25 and 13 and
# 7 odd: padded).  (11, 161, 161): depths 11, 6, 3, 2, 1 (3-D at level 0 only, the depth reaches 1).
MS_CASES = [("noise", (50, 176, 163)), ("near", (11, 161, 161))]      # noise: the levels differ, so the pooling shows


def case_id(kind, shape):
    return f"{kind}-{shape[0]}x{shape[1]}x{shape[2]}"


taps = mc.taps


def pair(kind, shape, n=N, c=C):
    """uint8 X, Y [n, c, D, H, W], seeded by kind and shape."""
    D, H, W = shape
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{D}x{H}x{W}/{n}x{c}".encode()))
    full = (n, c, D, H, W)
    if kind == "noise":
        X, Y = rng.integers(0, 256, full), rng.integers(0, 256, full)
    elif kind == "near":
        X = rng.integers(6, 250, full)
        Y = X + 6 * (2 * rng.integers(0, 2, full) - 1)
    elif kind == "smooth":
        zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        ph = rng.uniform(0, 6.28, (n, c, 1, 1, 1))
        base = 127.5 + 100.0 * np.sin(xx / 9.0 + ph) * np.cos(yy / 7.0 + 0.5 * ph) * np.cos(zz / 5.0 - ph)
        X, Y = np.rint(base + rng.uniform(-3, 3, full)), np.rint(base + rng.uniform(-3, 3, full))
    elif kind == "flat":
        X, Y = 255 - (rng.random(full) < 0.02), 255 - (rng.random(full) < 0.02)
    elif kind == "anti":
        X = rng.integers(0, 256, full)
        Y = 255 - X
    elif kind == "const":
        X, Y = np.full(full, 17), np.full(full, 200)
    elif kind == "equal":
        X = rng.integers(0, 256, full)
        Y = X.copy()
    else:
        raise KeyError(kind)
    X, Y = np.clip(X, 0, 255).astype(np.uint8), np.clip(Y, 0, 255).astype(np.uint8)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


# ---- float64 restatement -------------------------------------------------------------------------------------------------
def _filt_axis(a, w, axis):
    n, L = len(w), a.shape[axis]
    sl = [slice(None)] * a.ndim

    def cut(k):
        sl[axis] = slice(k, L - n + 1 + k)
        return a[tuple(sl)]
    return sum(w[k] * cut(k) for k in range(n))


def gauss64(a, w, skip_depth=False):
    """`gaussian_filter` on [N, C, D, H, W]: along D, H, W in that order, a dimension below the window left unsmoothed (the
    reference warns and skips).  skip_depth=True: the WRONG variant that never smooths along D."""
    for i, axis in enumerate((2, 3, 4)):
        if a.shape[axis] >= len(w) and not (skip_depth and i == 0):
            a = _filt_axis(a, w, axis)
    return a


def ssim_maps64(x, y, w32, data_range=255.0, Kc=K, skip_depth=False):
    x, y, w = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(w32, np.float64)
    C1, C2 = (Kc[0] * data_range) ** 2, (Kc[1] * data_range) ** 2

    def g(a):
        return gauss64(a, w, skip_depth)
    mu1, mu2 = g(x), g(y)
    s1, s2, s12 = g(x * x) - mu1 * mu1, g(y * y) - mu2 * mu2, g(x * y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs, cs


def ssim64(x, y, w32, data_range=255.0, Kc=K, skip_depth=False):
    """(ssim_per_channel, cs) [N, C] of 5-D x, y: the two returns of `_ssim`."""
    s, cs = ssim_maps64(x, y, w32, data_range, Kc, skip_depth)
    return s.reshape(*s.shape[:2], -1).mean(-1), cs.reshape(*cs.shape[:2], -1).mean(-1)


def pool64(a, divisor=8.0, depth_pad=True, count_pad=True):
    """F.avg_pool3d(a, kernel_size=2, padding=(D % 2, H % 2, W % 2)): the zero pad in front of every odd dimension, counted;
    divisor 8.  The keywords are the WRONG variants: another divisor, no pad along the depth (the last plane of an odd depth
    is dropped, as a pool with padding 0 does), the pad left out of the count."""
    a = np.asarray(a, np.float64)
    D, H, W = a.shape[-3:]
    pd = D % 2 if depth_pad else 0
    ones = np.pad(np.ones((D, H, W)), [(pd, 0), (H % 2, 0), (W % 2, 0)])
    a = np.pad(a, [(0, 0)] * (a.ndim - 3) + [(pd, 0), (H % 2, 0), (W % 2, 0)])
    if not depth_pad and D % 2:
        a, ones = a[..., :D - 1, :, :], ones[:D - 1]

    def sum8(t):
        return sum(t[..., i::2, j::2, k::2] for i in (0, 1) for j in (0, 1) for k in (0, 1))
    return sum8(a) / (divisor if count_pad else sum8(ones))


def ms_levels64(x, y, w32, data_range=255.0, Kc=K, levels=len(mc.MS_WEIGHTS), **pool_kw):
    """[(ssim_per_channel, cs, x, y)] per level (x, y: that level's float64 inputs)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = []
    for i in range(levels):
        out.append(ssim64(x, y, w32, data_range, Kc) + (x, y))
        if i < levels - 1:
            x, y = pool64(x, **pool_kw), pool64(y, **pool_kw)
    return out


def ms_ssim64(x, y, w32, data_range=255.0, Kc=K, weights=mc.MS_WEIGHTS, **pool_kw):
    """[N, C]: ms_ssim_val before the channel mean."""
    lv = ms_levels64(x, y, w32, data_range, Kc, len(weights), **pool_kw)
    return mc.ms_combine64([l[1] for l in lv[:-1]], lv[-1][0], weights)


def sqerr64(x, y):
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return (d * d).reshape(*d.shape[:2], -1).sum(-1)


def psnr64(x, y, mval=255.0):
    """Per volume [N, C]: 20 log10(mval / sqrt(mse)) over D, H, W."""
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    with np.errstate(divide="ignore"):
        return 20 * np.log10(mval / np.sqrt((d * d).reshape(*d.shape[:2], -1).mean(-1)))


def interleave(vols):
    """[(s c), H, W] from the per-stain volumes [c][D, H, W]: slice-major, stain-minor, as the stitcher orders a mosaic."""
    return np.ascontiguousarray(np.stack(vols, axis=1).reshape(-1, *vols[0].shape[1:]))


# ---- the kernel's tiles ----------------------------------------------------------------------------------------------------
def tiles(x, y, n):
    """All workgroups of one volume pair [D, H, W] at once: (valid [T, TH, TW], cx [T], cy [T], a, b [T, D, TH + n - 1,
    TW + n - 1]); a = x - cx, b = y - cy, zero outside the plane, in the dtype of x."""
    D, H, W = x.shape
    Ho, Wo = H - n + 1, W - n + 1
    RA, CA = TH + n - 1, TW + n - 1
    va, cxs, cys, aa, bb = [], [], [], [], []
    for oy in range(0, Ho, TH):
        for ox in range(0, Wo, TW):
            rows, cols = min(RA, H - oy), min(CA, W - ox)
            cx, cy = x[0, oy, ox], y[0, oy, ox]
            a, b = np.zeros((D, RA, CA), x.dtype), np.zeros((D, RA, CA), x.dtype)
            a[:, :rows, :cols] = x[:, oy:oy + rows, ox:ox + cols] - cx
            b[:, :rows, :cols] = y[:, oy:oy + rows, ox:ox + cols] - cy
            va.append((np.arange(TH)[:, None] + oy < Ho) & (np.arange(TW)[None, :] + ox < Wo))
            cxs.append(cx), cys.append(cy), aa.append(a), bb.append(b)
    sh = (-1, 1, 1, 1)
    return np.stack(va), np.array(cxs, x.dtype).reshape(sh), np.array(cys, x.dtype).reshape(sh), np.stack(aa), np.stack(bb)


def _fma(acc, wt, p):
    """acc + wt * p with one rounding to the dtype of acc: the product of two float32 is exact in float64."""
    if acc.dtype == np.float64:
        return acc + wt * p
    return (acc.astype(np.float64) + np.float64(wt) * p.astype(np.float64)).astype(f32)


def _filt_tiles(p, w, n):
    """The kernel's three passes over [T, D, RA, CA]: along x into [.., TW], along y into [.., TH, TW], along z into
    [T, D - n + 1, TH, TW]; every pass takes the taps in order from a zero accumulator, one FMA per tap."""
    T, D = p.shape[:2]
    h = np.zeros(p.shape[:3] + (TW,), p.dtype)
    for t in range(n):
        h = _fma(h, w[t], p[..., t:t + TW])
    v = np.zeros((T, D, TH, TW), p.dtype)
    for t in range(n):
        v = _fma(v, w[t], h[:, :, t:t + TH, :])
    o = np.zeros((T, D - n + 1, TH, TW), p.dtype)
    for t in range(n):
        o = _fma(o, w[t], v[:, t:t + D - n + 1])
    return o


def walk32(x, y, w32, C1, C2, s_power=3):
    """(sum of ssim, sum of cs) of one volume pair, float32 arithmetic in the order of ssim_volumes_kernel; a lane's outputs
    go to float64 one by one.  s_power=2 is the WRONG variant that corrects with the weight of an n x n window."""
    x, y, w = np.asarray(x, f32), np.asarray(y, f32), np.asarray(w32, f32)
    n = len(w)
    s64 = w.astype(np.float64).sum() ** s_power
    S, d, C1, C2, two = f32(s64), f32(1.0 - s64), f32(C1), f32(C2), f32(2)
    valid, cx, cy, a, b = tiles(x, y, n)
    m1, m2, q11, q22, q12 = (_filt_tiles(p, w, n) for p in (a, b, a * a, b * b, a * b))
    cxS, cyS = cx * S, cy * S
    mu1, mu2 = m1 + cxS, m2 + cyS
    s1 = (q11 - m1 * m1) + d * (two * cx * m1 + cx * cxS)
    s2 = (q22 - m2 * m2) + d * (two * cy * m2 + cy * cyS)
    s12 = (q12 - m1 * m2) + d * ((cy * m1 + cx * m2) + cx * cyS)
    cs = (two * s12 + C2) / (s1 + s2 + C2)
    ss = ((two * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    assert ss.dtype == f32 and cs.dtype == f32
    m = valid[:, None]
    return float(np.where(m, ss, 0).astype(np.float64).sum()), float(np.where(m, cs, 0).astype(np.float64).sum())


def bound(x, y, w32, C1, C2):
    """(bound on mean ssim, bound on mean cs) of one volume pair [D, H, W]: the docstring's derivation in float64."""
    x, y, w = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(w32, np.float64)
    n = len(w)
    G = (3 * n + 3) * U
    S = float(f32(w.sum() ** 3))
    d = float(f32(1.0 - w.sum() ** 3))
    aw = np.abs(w)
    valid, cx, cy, a, b = tiles(x, y, n)
    m1, m2, q11, q22, q12 = (_filt_tiles(p, w, n) for p in (a, b, a * a, b * b, a * b))
    E1, E2, E11, E22, E12 = (G * _filt_tiles(np.abs(p), aw, n) for p in (a, b, a * a, b * b, a * b))
    ax, ay, aS, ad = np.abs(cx), np.abs(cy), abs(S), abs(d)
    mu1, mu2 = m1 + cx * S, m2 + cy * S
    dmu1, dmu2 = E1 + 3 * U * ax + U * np.abs(mu1), E2 + 3 * U * ay + U * np.abs(mu2)
    s1 = q11 - m1 * m1 + d * (2 * cx * m1 + cx * cx * S)
    s2 = q22 - m2 * m2 + d * (2 * cy * m2 + cy * cy * S)
    s12 = q12 - m1 * m2 + d * (cy * m1 + cx * m2 + cx * cy * S)
    ds1 = E11 + 2 * np.abs(m1) * E1 + 2 * ad * ax * E1 + 6 * U * (q11 + m1 * m1 + ad * (2 * ax * np.abs(m1) + ax * ax * aS))
    ds2 = E22 + 2 * np.abs(m2) * E2 + 2 * ad * ay * E2 + 6 * U * (q22 + m2 * m2 + ad * (2 * ay * np.abs(m2) + ay * ay * aS))
    ds12 = (E12 + np.abs(m1) * E2 + np.abs(m2) * E1 + ad * (ay * E1 + ax * E2)
            + 6 * U * (np.abs(q12) + np.abs(m1 * m2) + ad * (ay * np.abs(m1) + ax * np.abs(m2) + ax * ay * aS)))
    N2, D2 = 2 * s12 + C2, s1 + s2 + C2
    dN2, dD2 = 2 * ds12 + 2 * U * (2 * np.abs(s12) + C2), ds1 + ds2 + 3 * U * (np.abs(s1) + np.abs(s2) + C2)
    m = np.broadcast_to(valid[:, None], D2.shape)
    assert (D2 > 2 * dD2)[m].all(), "the bound needs a denominator well above its own error"
    cs = N2 / D2
    dcs = (dN2 + np.abs(cs) * dD2) / (D2 - dD2) + U * np.abs(cs)
    N1, D1 = 2 * mu1 * mu2 + C1, mu1 * mu1 + mu2 * mu2 + C1
    dN1 = 2 * (np.abs(mu1) * dmu2 + np.abs(mu2) * dmu1) + 3 * U * (2 * np.abs(mu1 * mu2) + C1)
    dD1 = 2 * (np.abs(mu1) * dmu1 + np.abs(mu2) * dmu2) + 4 * U * D1
    lum = N1 / D1
    dlum = (dN1 + np.abs(lum) * dD1) / (D1 - dD1) + U * np.abs(lum)
    ss = lum * cs
    dss = np.abs(lum) * dcs + np.abs(cs) * dlum + dlum * dcs + U * np.abs(ss)
    count = int(m.sum())
    tail = LANE_ADDS * U + 2.0 ** -50
    abs_s, abs_c = np.abs(ss[m]).sum(), np.abs(cs[m]).sum()
    return ((dss[m].sum() + tail * abs_s + U * abs(ss[m].sum())) / count, (dcs[m].sum() + tail * abs_c + U * abs_c) / count)


def volume_bounds(X, Y, w32, data_range=255.0, Kc=K):
    """(ssim bounds, cs bounds) [N, C] of [N, C, D, H, W] in whichever route the depth takes: bound() per volume when the depth
    reaches the window, else the mean of metrics_cases.bound over the D planes."""
    C1, C2 = (Kc[0] * data_range) ** 2, (Kc[1] * data_range) ** 2
    n = len(w32)
    if X.shape[2] >= n:
        b = np.array([[bound(X[i, j], Y[i, j], w32, C1, C2) for j in range(X.shape[1])] for i in range(X.shape[0])])
    else:
        b = np.array([[np.mean([mc.bound(X[i, j, k], Y[i, j, k], w32, C1, C2) for k in range(X.shape[2])], axis=0)
                       for j in range(X.shape[1])] for i in range(X.shape[0])])
    return b[..., 0], b[..., 1]


def ms_bound(lv, w32, data_range=255.0, Kc=K, weights=mc.MS_WEIGHTS):
    """Bound on ms_ssim_val [N, C] from the levels of ms_levels64 (whose inputs are exact in float32 for 8-bit data)."""
    wts = np.asarray(weights, np.float64).reshape(-1, 1, 1)
    vals, bnds = [], []
    for i, (s, cs, x, y) in enumerate(lv):
        bs, bc = volume_bounds(x, y, w32, data_range, Kc)
        last = i == len(lv) - 1
        vals.append(np.maximum(s if last else cs, 0))
        bnds.append(bs if last else bc)
    v, b = np.stack(vals), np.stack(bnds)
    f = np.prod(v ** wts, axis=0)
    hi, lo = np.prod((v + b) ** wts, axis=0), np.prod(np.maximum(v - b, 0) ** wts, axis=0)
    return np.maximum(hi - f, f - lo) + 32 * U * hi


psnr_tol = mc.psnr_tol

# ---- the wrong variants the bound must tell apart --------------------------------------------------------------------------
WRONG_SSIM = ("depth smoothing skipped", "depth stride of one plane")      # on the small cases, against ssim64
WRONG_POOL = {"pool divisor 4": dict(divisor=4.0), "pool without the depth pad": dict(depth_pad=False),
              "pad not counted": dict(count_pad=False)}                      # on the MS cases, against ms_ssim64
WRONG_WALK = "S = (sum of the taps)^2"                                       # on the walk, with a window that is not normalised


def wrong_ssim(name, X, Y, w32):
    """ssim_per_channel [N, C] of a wrong reading of the case X, Y [N, C, D, H, W]."""
    if name == "depth smoothing skipped":
        return ssim64(X, Y, w32, skip_depth=True)[0]
    if name == "depth stride of one plane":            # the C stains of image i interleaved; a stain read as D consecutive planes
        D = X.shape[2]
        out = []
        for i in range(X.shape[0]):
            mx, my = interleave(list(X[i])), interleave(list(Y[i]))
            out.append([ssim64(mx[None, None, c:c + D], my[None, None, c:c + D], w32)[0][0, 0] for c in range(X.shape[1])])
        return np.array(out)
    raise KeyError(name)
