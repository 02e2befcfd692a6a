"""Shared by tests/test_metrics_cases_host.py and tests/test_gpu_metrics.py: the measures of the reference's
utils/metrics.py:201-439 restated in float64 numpy (held to the reference itself through tests/golden/metrics_ref.npz, minted by
tools/make_metrics_golden.py), the seeded cases, a float32 walk in the order of operations of tm_metrics.hip, and the error
bound of that order.

THE BOUND (first order in U = 2^-24; the second-order terms are below 1e-6 of it).  Per output pixel, with the tile's shifts
cx, cy (x and y at the tile's first pixel), a = x - cx, b = y - cy, and F the exact separable filter with the float32 taps:
  * each of the five filtered quantities m1 = F a, m2 = F b, q11 = F a^2, q22 = F b^2, q12 = F ab is a dot product of n terms
    along x followed by one of n terms along y, every term a product that carries up to 3 roundings (two subtractions, one
    multiply):  |err| <= G F|.|,  G = (2 n + 3) U;
  * mu1 = m1 + cx S (S = the squared sum of the taps, the weight of the n x n window, rounded to float32): err(m1) + 3 U |cx| + U |mu1|;
  * s1 = q11 - m1^2 + d (2 cx m1 + cx^2 S), s12 = q12 - m1 m2 + d (cy m1 + cx m2 + cx cy S), d = 1 - S: the filter errors
    pushed through, plus 6 roundings on the magnitude of every term;
  * cs = N2 / D2, lum = N1 / D1, ssim = lum cs: (dN + |ratio| dD) / (D - dD) + U |ratio| each, with this pixel's own
    denominators in float64, C1 and C2 rounded to float32 (one U each);
then the mean of the per-pixel bounds, 7 U mean|v| for the lane's float32 sum of its 8 outputs (the tree above it is float64:
2^-50 relative), and U |mean| for the float32 result.  MS-SSIM: the interval of the product of the weighted powers over the
per-level bounds (the map is monotone in every level), plus 32 U for float32 pow and prod (5 powers at <= 4 U, 4 products, the
conversion).  PSNR: the squared-error sum is exact (uint8) or float64, so 8 U max(1, |psnr|) for sqrt, log10 and the result.
Nothing here was tuned on what the kernel returns.
"""
import zlib

import numpy as np
import torch

TW, TH, OPV = 64, 32, 8            # tm_kernels.h SSIM_TW, SSIM_TH; tm_metrics.hip SSIM_OPV (output rows a lane adds in float32)
U = 2.0 ** -24
N, C = 2, 2
WIN, SIGMA = 11, 1.5
K = (0.01, 0.03)
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
KINDS = ("noise", "near", "smooth", "flat", "anti", "const", "equal")
TILE_PLUS_ONE = (TH + WIN, TW + WIN)          # the valid output exceeds one 32 x 64 tile by one row and one column
MS_SHAPE = (176, 163)                         # levels 88 x 82, 44 x 41, 22 x 21, 11 x 11
SHAPES = ((11, 11), (12, 37), TILE_PLUS_ONE, MS_SHAPE)
CASES = [(k, s) for k in KINDS for s in SHAPES]
f32 = np.float32


def case_id(kind, shape):
    return f"{kind}-{shape[0]}x{shape[1]}"


def taps(n=WIN, sigma=SIGMA):
    """utils/metrics.py:218-233 (`_fspecial_gauss_1d`) in float32 torch -> float32 [n]."""
    coords = torch.arange(n, dtype=torch.float)
    coords -= n // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.numpy()


def pair(kind, shape):
    """uint8 X, Y [N, C, H, W], seeded by kind and shape."""
    H, W = shape
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{H}x{W}".encode()))
    full = (N, C, H, W)
    if kind == "noise":
        X, Y = rng.integers(0, 256, full), rng.integers(0, 256, full)
    elif kind == "near":
        X = rng.integers(6, 250, full)
        Y = X + 6 * (2 * rng.integers(0, 2, full) - 1)
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ph = rng.uniform(0, 6.28, (N, C, 1, 1))
        base = 127.5 + 100.0 * np.sin(xx / 9.0 + ph) * np.cos(yy / 7.0 + 0.5 * ph)
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


def unit_range(a_u8):
    """The same plane as float32 in [-1, 1] (data_range 2)."""
    return a_u8.astype(f32) / f32(127.5) - f32(1)


# ---- float64 restatement -------------------------------------------------------------------------------------------------
def filt_valid(a, w):
    """Separable valid filter of a [..., H, W] with the taps w, along H then along W (gaussian_filter's order)."""
    n = len(w)
    Hh, Ww = a.shape[-2:]
    t = sum(w[k] * a[..., k:Hh - n + 1 + k, :] for k in range(n))
    return sum(w[k] * t[..., :, k:Ww - n + 1 + k] for k in range(n))


def ssim_maps64(x, y, w32, data_range=255.0, Kc=K, same=False):
    """(ssim_map, cs_map) of utils/metrics.py:266-301 in float64 with the float32-rounded taps.  same=True: the WRONG variant
    with a zero-padded 'same' filter."""
    x, y, w = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(w32, np.float64)
    if same:
        p = len(w) // 2
        pad = [(0, 0)] * (x.ndim - 2) + [(p, p), (p, p)]
        x, y = np.pad(x, pad), np.pad(y, pad)
    C1, C2 = (Kc[0] * data_range) ** 2, (Kc[1] * data_range) ** 2
    mu1, mu2 = filt_valid(x, w), filt_valid(y, w)
    s1, s2, s12 = filt_valid(x * x, w) - mu1 * mu1, filt_valid(y * y, w) - mu2 * mu2, filt_valid(x * y, w) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs, cs


def ssim64(x, y, w32, data_range=255.0, Kc=K, same=False):
    """(ssim_per_channel, cs) [N, C]: the two returns of `_ssim`."""
    s, cs = ssim_maps64(x, y, w32, data_range, Kc, same)
    return s.reshape(*s.shape[:-2], -1).mean(-1), cs.reshape(*cs.shape[:-2], -1).mean(-1)


def pool64(a):
    """F.avg_pool2d(a, kernel_size=2, padding=(H % 2, W % 2)): zero pad on top / left, counted; divisor 4."""
    a = np.asarray(a, np.float64)
    H, W = a.shape[-2:]
    a = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(H % 2, 0), (W % 2, 0)])
    return (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2]) / 4


def ms_levels64(x, y, w32, data_range=255.0, Kc=K, levels=len(MS_WEIGHTS)):
    """[(ssim_per_channel, cs, x, y)] per level (x, y: that level's float64 inputs)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = []
    for i in range(levels):
        out.append(ssim64(x, y, w32, data_range, Kc) + (x, y))
        if i < levels - 1:
            x, y = pool64(x), pool64(y)
    return out


def ms_combine64(cs_levels, ssim_last, weights=MS_WEIGHTS):
    v = np.stack([np.maximum(c, 0) for c in cs_levels] + [np.maximum(ssim_last, 0)])
    return np.prod(v ** np.asarray(weights, np.float64).reshape(-1, *[1] * (v.ndim - 1)), axis=0)


def ms_ssim64(x, y, w32, data_range=255.0, Kc=K, weights=MS_WEIGHTS):
    """[N, C]: ms_ssim_val before the channel mean (utils/metrics.py:421-434)."""
    lv = ms_levels64(x, y, w32, data_range, Kc, len(weights))
    return ms_combine64([l[1] for l in lv[:-1]], lv[-1][0], weights)


def sqerr64(x, y):
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return (d * d).reshape(*d.shape[:-2], -1).sum(-1)


def psnr64(x, y, mval=255.0):
    """PSNR.forward for [N, C, H, W]: per image over C, H, W; inf for equal images."""
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    mse = (d * d).reshape(d.shape[0], -1).mean(-1)
    with np.errstate(divide="ignore"):
        return 20 * np.log10(mval / np.sqrt(mse))


# ---- the kernel's tiles ----------------------------------------------------------------------------------------------------
def tiles(x, y, n):
    """(valid mask [TH, TW], cx, cy, a, b) per workgroup of a plane pair: a = x - cx, b = y - cy over the (TH + n - 1) x (TW + n - 1)
    input of the tile, zero outside the plane, in the dtype of x (float32 or float64)."""
    H, W = x.shape
    Ho, Wo = H - n + 1, W - n + 1
    RA, CA = TH + n - 1, TW + n - 1
    for oy in range(0, Ho, TH):
        for ox in range(0, Wo, TW):
            rows, cols = min(RA, H - oy), min(CA, W - ox)
            cx, cy = x[oy, ox], y[oy, ox]
            a, b = np.zeros((RA, CA), x.dtype), np.zeros((RA, CA), x.dtype)
            a[:rows, :cols] = x[oy:oy + rows, ox:ox + cols] - cx
            b[:rows, :cols] = y[oy:oy + rows, ox:ox + cols] - cy
            valid = (np.arange(TH)[:, None] + oy < Ho) & (np.arange(TW)[None, :] + ox < Wo)
            yield valid, cx, cy, a, b


def _filt_tile(p, w, n):
    """The tile's two passes: along x into [RA, TW], then along y into [TH, TW]; taps in order from a zero accumulator, in
    the dtype of p and w (one rounding per multiply and per add in float32: the kernel's FMAs round once per tap)."""
    h = np.zeros((p.shape[0], TW), p.dtype)
    for t in range(n):
        h = h + w[t] * p[:, t:t + TW]
    v = np.zeros((TH, TW), p.dtype)
    for t in range(n):
        v = v + w[t] * h[t:t + TH, :]
    return v


def walk32(x, y, w32, C1, C2):
    """(sum of ssim, sum of cs) of one plane pair, float32 arithmetic in the order of ssim_planes_kernel; the sums above a
    lane's 8 outputs in float64."""
    x, y, w = np.asarray(x, f32), np.asarray(y, f32), np.asarray(w32, f32)
    n = len(w)
    s64 = w.astype(np.float64).sum() ** 2
    S, d, C1, C2, two = f32(s64), f32(1.0 - s64), f32(C1), f32(C2), f32(2)
    tot_s = tot_c = 0.0
    for valid, cx, cy, a, b in tiles(x, y, n):
        m1, m2, q11, q22, q12 = (_filt_tile(p, w, n) for p in (a, b, a * a, b * b, a * b))
        cxS, cyS = cx * S, cy * S
        mu1, mu2 = m1 + cxS, m2 + cyS
        s1 = (q11 - m1 * m1) + d * (two * cx * m1 + cx * cxS)
        s2 = (q22 - m2 * m2) + d * (two * cy * m2 + cy * cyS)
        s12 = (q12 - m1 * m2) + d * ((cy * m1 + cx * m2) + cx * cyS)
        cs = (two * s12 + C2) / (s1 + s2 + C2)
        ss = ((two * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
        assert ss.dtype == f32 and cs.dtype == f32
        for v, which in ((ss, 0), (cs, 1)):
            v = np.where(valid, v, f32(0)).reshape(TH // OPV, OPV, TW)
            lane = np.zeros((TH // OPV, TW), f32)
            for o in range(OPV):
                lane = lane + v[:, o, :]
            if which == 0:
                tot_s += float(lane.astype(np.float64).sum())
            else:
                tot_c += float(lane.astype(np.float64).sum())
    return tot_s, tot_c


def bound(x, y, w32, C1, C2):
    """(bound on mean ssim, bound on mean cs) of one plane pair: the docstring's derivation, evaluated in float64."""
    x, y, w = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(w32, np.float64)
    n = len(w)
    G = (2 * n + 3) * U
    S = float(f32(w.sum() ** 2))
    d = float(f32(1.0 - w.sum() ** 2))
    aw = np.abs(w)
    sum_s = sum_c = abs_s = abs_c = val_s = 0.0
    count = 0
    for valid, cx, cy, a, b in tiles(x, y, n):
        m1, m2, q11, q22, q12 = (_filt_tile(p, w, n) for p in (a, b, a * a, b * b, a * b))
        E1, E2, E11, E22, E12 = (G * _filt_tile(np.abs(p), aw, n) for p in (a, b, a * a, b * b, a * b))
        ax, ay, aS = abs(cx), abs(cy), abs(S)
        mu1, mu2 = m1 + cx * S, m2 + cy * S
        dmu1, dmu2 = E1 + 3 * U * ax + U * np.abs(mu1), E2 + 3 * U * ay + U * np.abs(mu2)
        s1 = q11 - m1 * m1 + d * (2 * cx * m1 + cx * cx * S)
        s2 = q22 - m2 * m2 + d * (2 * cy * m2 + cy * cy * S)
        s12 = q12 - m1 * m2 + d * (cy * m1 + cx * m2 + cx * cy * S)
        ad = abs(d)
        ds1 = E11 + 2 * np.abs(m1) * E1 + 2 * ad * ax * E1 + 6 * U * (q11 + m1 * m1 + ad * (2 * ax * np.abs(m1) + ax * ax * aS))
        ds2 = E22 + 2 * np.abs(m2) * E2 + 2 * ad * ay * E2 + 6 * U * (q22 + m2 * m2 + ad * (2 * ay * np.abs(m2) + ay * ay * aS))
        ds12 = (E12 + np.abs(m1) * E2 + np.abs(m2) * E1 + ad * (ay * E1 + ax * E2)
                + 6 * U * (np.abs(q12) + np.abs(m1 * m2) + ad * (ay * np.abs(m1) + ax * np.abs(m2) + ax * ay * aS)))
        N2, D2 = 2 * s12 + C2, s1 + s2 + C2
        dN2, dD2 = 2 * ds12 + 2 * U * (2 * np.abs(s12) + C2), ds1 + ds2 + 3 * U * (np.abs(s1) + np.abs(s2) + C2)
        assert (D2 > 2 * dD2)[valid].all(), "the bound needs a denominator well above its own error"
        cs = N2 / D2
        dcs = (dN2 + np.abs(cs) * dD2) / (D2 - dD2) + U * np.abs(cs)
        N1, D1 = 2 * mu1 * mu2 + C1, mu1 * mu1 + mu2 * mu2 + C1
        dN1 = 2 * (np.abs(mu1) * dmu2 + np.abs(mu2) * dmu1) + 3 * U * (2 * np.abs(mu1 * mu2) + C1)
        dD1 = 2 * (np.abs(mu1) * dmu1 + np.abs(mu2) * dmu2) + 4 * U * D1
        lum = N1 / D1
        dlum = (dN1 + np.abs(lum) * dD1) / (D1 - dD1) + U * np.abs(lum)
        ss = lum * cs
        dss = np.abs(lum) * dcs + np.abs(cs) * dlum + dlum * dcs + U * np.abs(ss)
        sum_s += dss[valid].sum()
        sum_c += dcs[valid].sum()
        abs_s += np.abs(ss[valid]).sum()
        abs_c += np.abs(cs[valid]).sum()
        val_s += ss[valid].sum()
        count += int(valid.sum())
    tail = (OPV - 1) * U + 2.0 ** -50
    return ((sum_s + tail * abs_s + U * abs(val_s)) / count, (sum_c + tail * abs_c + U * abs_c) / count)


def plane_bounds(X, Y, w32, data_range=255.0, Kc=K):
    """bound() over every plane of [N, C, H, W]: (ssim bounds, cs bounds), [N, C] each."""
    C1, C2 = (Kc[0] * data_range) ** 2, (Kc[1] * data_range) ** 2
    b = np.array([[bound(X[i, j], Y[i, j], w32, C1, C2) for j in range(X.shape[1])] for i in range(X.shape[0])])
    return b[..., 0], b[..., 1]


def ms_bound(lv, w32, data_range=255.0, Kc=K, weights=MS_WEIGHTS):
    """Bound on ms_ssim_val [N, C] from the levels of ms_levels64 (whose inputs are exact in float32 for 8-bit data)."""
    wts = np.asarray(weights, np.float64).reshape(-1, 1, 1)
    vals, bnds = [], []
    for i, (s, cs, x, y) in enumerate(lv):
        bs, bc = plane_bounds(x, y, w32, data_range, Kc)
        last = i == len(lv) - 1
        vals.append(np.maximum(s if last else cs, 0))
        bnds.append(bs if last else bc)
    v, b = np.stack(vals), np.stack(bnds)
    f = np.prod(v ** wts, axis=0)
    hi, lo = np.prod((v + b) ** wts, axis=0), np.prod(np.maximum(v - b, 0) ** wts, axis=0)
    return np.maximum(hi - f, f - lo) + 32 * U * hi


def psnr_tol(p):
    return 8 * U * np.maximum(1.0, np.abs(p))


# ---- the wrong variants the bound must tell apart (noise and anti at 11 x 11) ---------------------------------------------
def wrong_variants():
    """{name: kwargs of ssim64 (w32, data_range, Kc, same)}; the right one is (taps(), 255, K, False)."""
    w = taps()
    return {
        "sigma 1.0": dict(w32=taps(WIN, 1.0)),
        "9 taps": dict(w32=taps(9, SIGMA)),
        "K2 0.04": dict(w32=w, Kc=(0.01, 0.04)),
        "data_range 1": dict(w32=w, data_range=1.0),
        "K swapped": dict(w32=w, Kc=(0.03, 0.01)),
        "same padding": dict(w32=w, same=True),
        "window x 1.01": dict(w32=(w * f32(1.01)).astype(f32)),
    }
