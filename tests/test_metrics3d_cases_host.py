"""CPU: the float64 restatement of the reference's 5-D SSIM / MS-SSIM (metrics3d_cases.py) against the reference's own float64
results (tests/golden/metrics3d_ref.npz, tools/make_metrics3d_golden.py); the float32 walk in the volume kernel's order against
the derived bound; the bound against six wrong variants; the pooled levels against F.avg_pool3d; the argument checks of the
two entry points (before any device call) and of the 5-D Python surface on host tensors.

Every wrong variant has to move at least one case by more than WELL_OVER = 10 bounds.  Found (printed by
test_bound_tells_the_wrong_variants_apart and test_bound_tells_the_wrong_pools_apart), |wrong - right| / bound at the case
that shows the variant best: depth smoothing skipped 5681, depth stride of one plane 11053, S = (sum of the taps)^2 4276, pool
divisor 4 657, pad not counted 35, pool without the depth pad 12.6 (the smallest: that variant changes the levels from the
third on, whose own bounds, a few 1e-4, dominate the interval of the product)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics3d_cases as m3
import util
from teramind_amd import _lib, metrics

GOLDEN = np.load(os.path.join(util.ROOT, "tests", "golden", "metrics3d_ref.npz"))
IDS = [m3.case_id(k, s) for k, s in m3.CASES]
MS_IDS = [m3.case_id(k, s) for k, s in m3.MS_CASES]
C1, C2 = (m3.K[0] * 255.0) ** 2, (m3.K[1] * 255.0) ** 2
WELL_OVER = 10.0


@functools.lru_cache(maxsize=None)
def ms_model(kind, shape):
    X, Y = m3.pair(kind, shape, n=1)
    lv = m3.ms_levels64(X, Y, m3.taps())
    return X, Y, lv, m3.mc.ms_combine64([l[1] for l in lv[:-1]], lv[-1][0]), m3.ms_bound(lv, m3.taps())


@pytest.mark.parametrize("kind,shape", m3.CASES, ids=IDS)
def test_model_equals_the_reference(kind, shape):
    X, Y = m3.pair(kind, shape)
    key = m3.case_id(kind, shape)
    s, cs = m3.ssim64(X, Y, m3.taps())
    assert s.shape == (m3.N, m3.C)
    assert np.abs(s - GOLDEN[key + "/ssim_pc"]).max() <= 1e-10 and np.abs(cs - GOLDEN[key + "/cs"]).max() <= 1e-10
    assert np.abs(s.mean(1) - GOLDEN[key + "/ssim"]).max() <= 1e-10
    assert abs(s.mean() - GOLDEN[key + "/ssim_module"]) <= 1e-10


@pytest.mark.parametrize("kind,shape", m3.MS_CASES, ids=MS_IDS)
def test_ms_model_equals_the_reference(kind, shape):
    X, Y, lv, ms, _ = ms_model(kind, shape)
    key = m3.case_id(kind, shape)
    want = GOLDEN[key + "/ms_ssim"]
    assert np.isfinite(want).all() and (want > 0).all()
    assert np.abs(ms.mean(1) - want).max() <= 1e-10 and abs(ms.mean() - GOLDEN[key + "/ms_module"]) <= 1e-10
    assert np.abs(lv[0][0].mean(1) - GOLDEN[key + "/ssim"]).max() <= 1e-10
    depths = [l[2].shape[2] for l in lv]
    assert depths == ([50, 25, 13, 7, 4] if shape[0] == 50 else [11, 6, 3, 2, 1])     # 3-D window while the depth is >= 11


def test_pool_model_at_depth_one():
    """D = 1 pools to 1: the pad plane is counted, so the level is the in-plane 2 x 2 sum over 8 (F.avg_pool3d refuses a
    depth below its kernel, and the reference never pools one: the fifth level is the last)."""
    a = np.arange(2 * 3 * 4, dtype=np.float64).reshape(1, 1, 1, 6, 4)
    assert np.array_equal(m3.pool64(a)[0, 0, 0], m3.mc.pool64(a[0, 0])[0] / 2)


@pytest.mark.parametrize("kind,shape", m3.CASES, ids=IDS)
def test_float32_walk_stays_inside_the_bound(kind, shape):
    X, Y = m3.pair(kind, shape)
    w = m3.taps()
    s, cs = m3.ssim64(X, Y, w)
    bs, bc = m3.volume_bounds(X, Y, w)
    count = np.prod([d - m3.WIN + 1 for d in shape])
    for i in range(m3.N):
        for j in range(m3.C):
            ws, wc = m3.walk32(X[i, j], Y[i, j], w, C1, C2)
            print(f"{kind} {shape} volume {i},{j}: |d ssim| {abs(ws / count - s[i, j]):.3e} / {bs[i, j]:.3e}   "
                  f"|d cs| {abs(wc / count - cs[i, j]):.3e} / {bc[i, j]:.3e}")
            assert abs(ws / count - s[i, j]) <= bs[i, j] and abs(wc / count - cs[i, j]) <= bc[i, j]


@pytest.mark.parametrize("kind,shape", m3.MS_CASES, ids=MS_IDS)
def test_float32_walk_stays_inside_the_bound_on_the_ms_levels(kind, shape):
    """Every level of the MS cases that is as deep as the window (the others are the plane kernel's, metrics_cases.py)."""
    X, Y, lv, _, _ = ms_model(kind, shape)
    w = m3.taps()
    deep = [l for l in lv if l[2].shape[2] >= m3.WIN]
    assert len(deep) == (3 if shape[0] == 50 else 1)
    for s, cs, x, y in deep:
        bs, bc = m3.volume_bounds(x, y, w)
        count = np.prod([d - m3.WIN + 1 for d in x.shape[2:]])
        for j in range(m3.C):
            ws, wc = m3.walk32(x[0, j], y[0, j], w, C1, C2)
            print(f"{kind} level {x.shape[2:]} channel {j}: |d ssim| {abs(ws / count - s[0, j]):.3e} / {bs[0, j]:.3e}   "
                  f"|d cs| {abs(wc / count - cs[0, j]):.3e} / {bc[0, j]:.3e}")
            assert abs(ws / count - s[0, j]) <= bs[0, j] and abs(wc / count - cs[0, j]) <= bc[0, j]


def test_float32_walk_on_the_unit_range_and_short_windows():
    """float32 volumes in [-1, 1], data_range 2, and windows of 3, 5 and 9 taps on 8-bit data."""
    w = m3.taps()
    c1, c2 = (m3.K[0] * 2.0) ** 2, (m3.K[1] * 2.0) ** 2
    for kind in m3.KINDS:
        Xu, Yu = m3.pair(kind, (12, 12, 37))
        X, Y = m3.mc.unit_range(Xu), m3.mc.unit_range(Yu)
        s, cs = m3.ssim64(X, Y, w, data_range=2.0)
        bs, bc = m3.volume_bounds(X, Y, w, data_range=2.0)
        ws, wc = m3.walk32(X[0, 0], Y[0, 0], w, c1, c2)
        assert abs(ws / 108 - s[0, 0]) <= bs[0, 0] and abs(wc / 108 - cs[0, 0]) <= bc[0, 0], kind
    X, Y = m3.pair("smooth", m3.TILE_PLUS_ONE)
    for n in (3, 5, 9):
        wn = m3.taps(n, 0.3 * ((n - 1) * 0.5 - 1) + 0.8)
        s, cs = m3.ssim64(X, Y, wn)
        bs, bc = m3.volume_bounds(X, Y, wn)
        count = np.prod([d - n + 1 for d in m3.TILE_PLUS_ONE])
        ws, wc = m3.walk32(X[1, 0], Y[1, 0], wn, C1, C2)
        assert abs(ws / count - s[1, 0]) <= bs[1, 0] and abs(wc / count - cs[1, 0]) <= bc[1, 0], n


def test_bound_tells_the_wrong_variants_apart():
    """Depth smoothing skipped and the stains mixed, on the small cases; S of an n x n window, on the walk with a window
    that is not normalised (for a normalised one S is 1 either way and the correction vanishes)."""
    w = m3.taps()
    best = {name: 0.0 for name in m3.WRONG_SSIM + (m3.WRONG_WALK,)}
    for kind, shape in m3.CASES:
        X, Y = m3.pair(kind, shape)
        right, bnd = m3.ssim64(X, Y, w)[0], m3.volume_bounds(X, Y, w)[0]
        for name in m3.WRONG_SSIM:
            best[name] = max(best[name], float((np.abs(m3.wrong_ssim(name, X, Y, w) - right) / bnd).max()))
    w101 = (w * np.float32(1.01)).astype(np.float32)
    for kind in ("noise", "near", "anti"):               # kinds whose variances stay positive under a window that weighs 1.03
        X, Y = m3.pair(kind, (12, 12, 37))
        right, bnd = m3.ssim64(X, Y, w101)[0][0, 0], m3.volume_bounds(X, Y, w101)[0][0, 0]
        ok = m3.walk32(X[0, 0], Y[0, 0], w101, C1, C2)[0] / 108
        bad = m3.walk32(X[0, 0], Y[0, 0], w101, C1, C2, s_power=2)[0] / 108
        assert abs(ok - right) <= bnd, kind                        # the walk alone passes
        best[m3.WRONG_WALK] = max(best[m3.WRONG_WALK], abs(bad - right) / bnd)
    print("largest |wrong - right| / bound per variant:", best)
    assert all(v > WELL_OVER for v in best.values()), best


def test_bound_tells_the_wrong_pools_apart():
    best = {name: 0.0 for name in m3.WRONG_POOL}
    for kind, shape in m3.MS_CASES:
        X, Y, _, right, bnd = ms_model(kind, shape)
        for name, kw in m3.WRONG_POOL.items():
            if name == "pool without the depth pad" and shape[0] == 11:
                continue                                   # 11 -> 5 -> 2 -> 1 -> 0 planes: that variant has no last level there
            wrong = m3.ms_ssim64(X, Y, m3.taps(), **kw)
            best[name] = max(best[name], float((np.abs(wrong - right) / bnd).max()))
    print("largest |wrong - right| / bound per pool variant:", best)
    assert all(v > WELL_OVER for v in best.values()), best


def test_pooled_levels_equal_avg_pool3d_bit_for_bit():
    X, _ = m3.pair("noise", (50, 176, 163), n=1)
    a, t = X.astype(np.float64), torch.from_numpy(X.astype(np.float32))
    sizes = []
    for _ in range(4):
        a = m3.pool64(a)
        t = F.avg_pool3d(t, kernel_size=2, padding=[s % 2 for s in t.shape[2:]])
        sizes.append(tuple(t.shape[2:]))
        assert a.shape == t.shape and np.array_equal(a.astype(np.float32), t.numpy()) and np.array_equal(a, t.numpy().astype(np.float64))
    assert sizes == [(25, 88, 82), (13, 44, 41), (7, 22, 21), (4, 11, 11)]


def test_five_d_argument_checks_without_device():
    a = torch.zeros(1, 2, 11, 32, 32)
    for call in (metrics.ssim, metrics.ms_ssim):
        with pytest.raises(ValueError, match="same dimensions"):
            call(a, torch.zeros(1, 2, 11, 32, 31))
        with pytest.raises(ValueError, match="same dtype"):
            call(a, a.to(torch.uint8))
        with pytest.raises(ValueError, match="odd"):
            call(a, a, win_size=10)
    with pytest.raises(AssertionError, match="larger than 160"):
        metrics.ms_ssim(torch.zeros(1, 1, 50, 160, 400), torch.zeros(1, 1, 50, 160, 400))
    big = torch.zeros(1, 1, 11, 161, 161)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # NotImplementedError is one
        metrics.ssim(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.ms_ssim(big, big)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.SSIM(channel=2, spatial_dims=3)(a, a)
    with pytest.raises(TypeError, match="uint8 or float32"):
        metrics.ssim(a.double(), a.double())
    with pytest.raises(ValueError, match="whole number of slices"):
        metrics.compare_volumes(np.zeros((5, 32, 32), np.uint8), np.zeros((5, 32, 32), np.uint8))
    with pytest.raises(ValueError, match="below the 3-D window"):
        metrics.compare_volumes(np.zeros((20, 32, 32), np.uint8), np.zeros((20, 32, 32), np.uint8))
    with pytest.raises(TypeError, match="uint8"):
        metrics.compare_volumes(np.zeros((22, 32, 32), np.float32), np.zeros((22, 32, 32), np.float32))
    assert metrics.MAX_TAPS_3D == m3.MAX_TAPS == 11
    assert metrics.SSIM(channel=3, spatial_dims=3).win.shape == (3, 1, 1, 1, 11)


def test_entry_points_refuse_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 1)
    w = (C.c_float * 16)(*([1.0 / 11] * 16))
    ARG = -1
    f = L.tm_ssim_volumes

    def vol(x=p, y=p, dtype=0, V=1, D=16, H=16, W=16, xp=16, xd=256, xv=4096, yp=16, yd=256, yv=4096, win=w, n=11, out=p):
        rc = f(x, y, dtype, V, D, H, W, xp, xd, xv, yp, yd, yv, win, n, 1.0, 1.0, out, None)
        return rc, L.tm_last_error()

    for kw, text in ((dict(x=None), b"null"), (dict(y=None), b"null"), (dict(win=None), b"null"), (dict(out=None), b"null"),
                     (dict(dtype=2), b"dtype"), (dict(n=10), b"taps"), (dict(n=1), b"taps"), (dict(n=13), b"registers"),
                     (dict(n=33), b"taps"), (dict(D=10), b"below the window"), (dict(H=10), b"below the window"),
                     (dict(W=10), b"below the window"), (dict(V=0), b"V ="), (dict(V=65536), b"V ="), (dict(xp=15), b"pitch"),
                     (dict(yp=15), b"pitch"), (dict(xd=255), b"depth stride"), (dict(yd=16 * 15 + 15), b"depth stride"),
                     (dict(dtype=1, xp=64, yp=64, xd=1024, yd=1024, x=odd), b"multiples of 4"),
                     (dict(dtype=1, xp=64, yp=64, xd=1026, yd=1024), b"multiple of 4"),
                     (dict(dtype=1, xp=60, yp=64, xd=1024, yd=1024), b"pitch"), (dict(xp=(1 << 26) + 1, xd=1 << 40), b"2^26")):
        rc, msg = vol(**kw)
        assert rc == ARG and text in msg, (kw, rc, msg)
    # the depth stride of an interleaved mosaic and a zero volume stride (V = 1) are geometry, not errors: they reach the device
    # call, so they are not tried here
    g = L.tm_avgpool2_pad3
    ok = (p, 0, 1, 8, 8, 8, 8, 64, 512, p, 16, 64, 256)
    for i, val, text in ((0, None, b"null"), (9, None, b"null"), (1, 3, b"dtype"), (2, 0, b"V ="), (3, 0, b"positive"),
                         (6, 7, b"pitch"), (7, 63, b"depth stride"), (10, 12, b"pitch"), (11, 60, b"depth stride")):
        args = list(ok)
        args[i] = val
        assert g(*args, None) == ARG and text in L.tm_last_error(), (i, val, L.tm_last_error())
