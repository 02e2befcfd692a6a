"""CPU: the float64 restatement of the reference's SSIM / MS-SSIM / PSNR (metrics_cases.py) against the reference's own
float64 results (tests/golden/metrics_ref.npz, tools/make_metrics_golden.py); the float32 walk in the kernel's order against
the derived bound; the bound against seven wrong variants; the pooled levels against F.avg_pool2d; the real-tile stitcher;
the argument checks of teramind_amd.metrics and of the two entry points (before any device call)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_cases as mc
import util
from teramind_amd import _lib, formats, metrics, stitch

GOLDEN = np.load(os.path.join(util.ROOT, "tests", "golden", "metrics_ref.npz"))
IDS = [mc.case_id(k, s) for k, s in mc.CASES]


@pytest.mark.parametrize("kind,shape", mc.CASES, ids=IDS)
def test_model_equals_the_reference(kind, shape):
    X, Y = mc.pair(kind, shape)
    key = mc.case_id(kind, shape)
    s, cs = mc.ssim64(X, Y, mc.taps())
    assert np.abs(s - GOLDEN[key + "/ssim_pc"]).max() <= 1e-10 and np.abs(cs - GOLDEN[key + "/cs"]).max() <= 1e-10
    assert np.abs(s.mean(1) - GOLDEN[key + "/ssim"]).max() <= 1e-10
    p, want = mc.psnr64(X, Y), GOLDEN[key + "/psnr"]
    if kind == "equal":
        assert np.isposinf(p).all() and np.isposinf(want).all()
    else:
        assert np.isfinite(want).all() and np.abs(p - want).max() <= 1e-10
    if shape == mc.MS_SHAPE:
        want = GOLDEN[key + "/ms_ssim"]
        assert np.isfinite(want).all() and np.abs(mc.ms_ssim64(X, Y, mc.taps()).mean(1) - want).max() <= 1e-10
        if kind == "anti":
            assert (want == 0).all()                      # cs < 0 at every level: relu


@pytest.mark.parametrize("kind,shape", mc.CASES, ids=IDS)
def test_float32_walk_stays_inside_the_bound(kind, shape):
    X, Y = mc.pair(kind, shape)
    w = mc.taps()
    C1, C2 = (mc.K[0] * 255.0) ** 2, (mc.K[1] * 255.0) ** 2
    s, cs = mc.ssim64(X, Y, w)
    bs, bc = mc.plane_bounds(X, Y, w)
    count = (shape[0] - mc.WIN + 1) * (shape[1] - mc.WIN + 1)
    for i in range(mc.N):
        for j in range(mc.C):
            ws, wc = mc.walk32(X[i, j], Y[i, j], w, C1, C2)
            print(f"{kind} {shape} plane {i},{j}: |d ssim| {abs(ws / count - s[i, j]):.3e} / {bs[i, j]:.3e}   "
                  f"|d cs| {abs(wc / count - cs[i, j]):.3e} / {bc[i, j]:.3e}")
            assert abs(ws / count - s[i, j]) <= bs[i, j] and abs(wc / count - cs[i, j]) <= bc[i, j]


def test_float32_walk_on_the_unit_range_stays_inside_the_bound():
    """float32 planes in [-1, 1], data_range 2: the inputs carry their own rounding; the model reads the same float32 values."""
    w = mc.taps()
    C1, C2 = (mc.K[0] * 2.0) ** 2, (mc.K[1] * 2.0) ** 2
    for kind in mc.KINDS:
        Xu, Yu = mc.pair(kind, (12, 37))
        X, Y = mc.unit_range(Xu), mc.unit_range(Yu)
        s, cs = mc.ssim64(X, Y, w, data_range=2.0)
        bs, bc = mc.plane_bounds(X, Y, w, data_range=2.0)
        ws, wc = mc.walk32(X[0, 0], Y[0, 0], w, C1, C2)
        assert abs(ws / 54 - s[0, 0]) <= bs[0, 0] and abs(wc / 54 - cs[0, 0]) <= bc[0, 0], kind


@pytest.mark.parametrize("kind", ["noise", "anti"])
def test_bound_tells_the_wrong_variants_apart(kind):
    X, Y = mc.pair(kind, (11, 11))
    right = mc.ssim64(X, Y, mc.taps())[0].mean(1)                  # what `ssim(size_average=False)` returns, [N]
    bnd = mc.plane_bounds(X, Y, mc.taps())[0].mean(1)
    assert (bnd < 4.6e-4).all()                                    # the reference moves by >= 4.6e-3 for every variant
    for name, kw in mc.wrong_variants().items():
        wrong = mc.ssim64(X, Y, **kw)[0].mean(1)
        print(f"{kind} / {name}: moves {np.abs(wrong - right).min():.3e}, bound {bnd.max():.3e}")
        assert (np.abs(wrong - right) > bnd).all(), name


def test_pooled_levels_equal_avg_pool2d_bit_for_bit():
    X, _ = mc.pair("noise", mc.MS_SHAPE)
    a, t = X.astype(np.float64), torch.from_numpy(X.astype(np.float32))
    sizes = []
    for _ in range(4):
        a = mc.pool64(a)
        t = F.avg_pool2d(t, kernel_size=2, padding=[s % 2 for s in t.shape[2:]])
        sizes.append(tuple(t.shape[2:]))
        assert a.shape == t.shape and np.array_equal(a.astype(np.float32), t.numpy()) and np.array_equal(a, t.numpy().astype(np.float64))
    assert sizes == [(88, 82), (44, 41), (22, 21), (11, 11)]


def test_stitch_real_dir(tmp_path):
    """2 x 2 real tiles with eight-number names and the 128-px frame, [(c s), 512, 512]: the centres in '(s c)' order."""
    rng = np.random.default_rng(5)
    hst, wst, slc, cst = 20480, 40960, 3, 2
    want = np.zeros((slc * cst, 512, 512), np.uint8)
    for ph in range(2):
        for pw in range(2):
            r0, c0 = hst + 256 * ph, wst + 256 * pw
            a = rng.integers(0, 256, (cst * slc, 512, 512)).astype(np.float16)
            formats.write_zarr_zip(tmp_path / f"{r0}_{r0 + 256}_{c0}_{c0 + 256}_{r0 - 128}_{r0 + 384}_{c0 - 128}_{c0 + 384}.zip", a)
            for c in range(cst):
                for s in range(slc):
                    want[s * cst + c, 256 * ph:256 * ph + 256, 256 * pw:256 * pw + 256] = a[c * slc + s, 128:384, 128:384].astype(np.uint8)
    got = stitch.stitch_real_dir(tmp_path, hst, wst, 2, 2, slc=slc)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(stitch.stitch_real_dir(tmp_path, hst, wst, 2, 2, slc=slc, slices=[4, 1]), want[[4, 1]])
    with pytest.raises(FileNotFoundError):
        stitch.stitch_real_dir(tmp_path, hst, wst, 3, 2, slc=slc)


def test_metrics_argument_checks_without_device():
    """The reference's checks with its exception types, raised on host tensors before anything is launched."""
    a = torch.zeros(1, 2, 32, 32)
    with pytest.raises(ValueError, match="same dimensions"):
        metrics.ssim(a, torch.zeros(1, 2, 32, 31))
    with pytest.raises(ValueError, match="same dimensions"):
        metrics.ms_ssim(a, torch.zeros(1, 2, 32, 31))
    with pytest.raises(ValueError, match="4-d or 5-d"):
        metrics.ssim(torch.zeros(4, 32, 32), torch.zeros(4, 32, 32))
    with pytest.raises(ValueError, match="same dtype"):
        metrics.ssim(a, a.to(torch.uint8))
    with pytest.raises(ValueError, match="same dtype"):
        metrics.ms_ssim(a, a.to(torch.uint8))
    with pytest.raises(ValueError, match="odd"):
        metrics.ssim(a, a, win_size=10)
    with pytest.raises(ValueError, match="odd"):
        metrics.ms_ssim(a, a, win_size=10)
    with pytest.raises(ValueError, match="odd"):
        metrics.ssim(a, a, win=torch.ones(2, 1, 1, 4) / 4)
    with pytest.raises(AssertionError, match="larger than 160"):
        metrics.ms_ssim(torch.zeros(1, 1, 160, 400), torch.zeros(1, 1, 160, 400))
    with pytest.raises(AssertionError):
        metrics.SSIM(unsqueeze=True)(a, a)
    with pytest.raises(NotImplementedError, match="3-D window"):
        metrics.ssim(torch.zeros(1, 1, 11, 32, 32), torch.zeros(1, 1, 11, 32, 32))
    with pytest.raises(NotImplementedError, match="depth"):
        metrics.ms_ssim(torch.zeros(1, 1, 4, 200, 200), torch.zeros(1, 1, 4, 200, 200))
    win = torch.ones(2, 1, 1, 3) / 3
    win[1, 0, 0, 0] = 0.5
    with pytest.raises(NotImplementedError, match="differs between channels"):
        metrics.ssim(a, a, win=win)
    # trailing singleton dimensions are squeezed first, as the reference does: [1, 2, 32, 32, 1] is 4-D
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.ssim(a[..., None], a[..., None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.PSNR()(a, a)
    with pytest.raises(TypeError, match="uint8 or float32"):
        metrics.ssim(a.double(), a.double())
    assert np.array_equal(metrics._fspecial_gauss_1d(11, 1.5).reshape(-1).numpy(), mc.taps())
    assert metrics.MAX_TAPS == 33 and tuple(metrics.MS_WEIGHTS) == mc.MS_WEIGHTS


def test_entry_points_refuse_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 1)
    w = (C.c_float * 34)(*([1.0 / 11] * 34))
    ARG = -1
    # tm_ssim_planes(x, y, dtype, P, H, W, x_pitch, x_plane, y_pitch, y_plane, win_host, n, C1, C2, out, stream)
    f = L.tm_ssim_planes
    assert f(None, p, 0, 1, 16, 16, 16, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG and b"null" in L.tm_last_error()
    assert f(p, None, 0, 1, 16, 16, 16, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG
    assert f(p, p, 0, 1, 16, 16, 16, 256, 16, 256, None, 11, 1.0, 1.0, p, None) == ARG
    assert f(p, p, 0, 1, 16, 16, 16, 256, 16, 256, w, 11, 1.0, 1.0, None, None) == ARG
    assert f(p, p, 2, 1, 16, 16, 16, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG and b"dtype" in L.tm_last_error()
    for n in (10, 1, 35, 34, -3):
        assert f(p, p, 0, 1, 64, 64, 64, 4096, 64, 4096, w, n, 1.0, 1.0, p, None) == ARG and b"taps" in L.tm_last_error()
    assert f(p, p, 0, 1, 10, 16, 16, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG and b"below the window" in L.tm_last_error()
    assert f(p, p, 0, 1, 16, 10, 16, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG and b"below the window" in L.tm_last_error()
    assert f(p, p, 0, 0, 16, 16, 16, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG
    assert f(p, p, 0, 1, 16, 16, 15, 256, 16, 256, w, 11, 1.0, 1.0, p, None) == ARG and b"pitch" in L.tm_last_error()
    assert f(p, p, 0, 1, 16, 16, 16, 256, 15, 256, w, 11, 1.0, 1.0, p, None) == ARG and b"pitch" in L.tm_last_error()
    assert f(p, p, 1, 1, 16, 16, 60, 1024, 64, 1024, w, 11, 1.0, 1.0, p, None) == ARG and b"pitch" in L.tm_last_error()
    assert f(odd, p, 1, 1, 16, 16, 64, 1024, 64, 1024, w, 11, 1.0, 1.0, p, None) == ARG and b"multiples of 4" in L.tm_last_error()
    # tm_avgpool2_pad(src, dtype, P, H, W, src_pitch, src_plane, dst, dst_pitch, dst_plane, stream)
    g = L.tm_avgpool2_pad
    assert g(None, 0, 1, 8, 8, 8, 64, p, 16, 64, None) == ARG and b"null" in L.tm_last_error()
    assert g(p, 0, 1, 8, 8, 8, 64, None, 16, 64, None) == ARG
    assert g(p, 3, 1, 8, 8, 8, 64, p, 16, 64, None) == ARG and b"dtype" in L.tm_last_error()
    assert g(p, 0, 1, 0, 8, 8, 64, p, 16, 64, None) == ARG
    assert g(p, 0, 1, 8, 9, 8, 64, p, 20, 80, None) == ARG and b"pitch" in L.tm_last_error()
    assert g(p, 0, 1, 8, 9, 9, 72, p, 16, 80, None) == ARG and b"pitch" in L.tm_last_error()
