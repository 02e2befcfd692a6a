"""ROI evaluation: PSNR, SSIM and MS-SSIM of a generated / real pair ("evaluation").

The call surface of the reference's utils/metrics.py:201-541 (`PSNR`, `ssim`, `ms_ssim`, `SSIM`, `MS_SSIM`) with its checks
and exception types.  The arithmetic runs in tm_metrics.hip: `tm_ssim_planes` reads each pixel of X and Y once and returns,
per plane, the fp64 sums of the ssim map, of the cs map and of (x - y)^2; `tm_avgpool2_pad` is one MS-SSIM level.  What is
left to torch are the means, relu, and the product of the weighted powers, on [N, C] tensors.

5-D inputs [N, C, D, H, W] are volumes, as in the reference: a depth that reaches the window is smoothed along D, H and W
(`tm_ssim_volumes`, the 3-D window; any pitch, depth stride and volume stride is read in place, so one stain of an '(s c)'
mosaic needs no copy), a shallower one in-plane only (its planes averaged, which is what the reference computes when it skips
the depth smoothing).  5-D `ms_ssim` pools every level along the depth too (`tm_avgpool2_pad3`) and takes either route per
level.  `compare_volumes` reports PSNR, SSIM and MS-SSIM per stain of two mosaics over the slice stack.

Extension over the reference: inputs are device tensors of float32 or uint8 (the reference takes float only); uint8 needs
no float copy of a mosaic.  Results are float32 device tensors of the reference's shapes.  Not covered (NotImplementedError
with the reason): 3-D windows of more than 11 taps, planes smaller than the window (the reference skips the smoothing
there), windows that differ between channels or have more than 33 taps.  No CPU fallback (a 5-D host tensor is refused with
a NotImplementedError, which is a RuntimeError, as it was before the 3-D window existed).
"""
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_TAPS = 33
MAX_TAPS_3D = 11
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _fspecial_gauss_1d(size, sigma):
    """utils/metrics.py:218-233: the 1-D Gaussian in float32 torch, [1, 1, size]."""
    coords = torch.arange(size, dtype=torch.float)
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.unsqueeze(0).unsqueeze(0)


def _squeeze_pair(X, Y):
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    for d in range(len(X.shape) - 1, 1, -1):
        X = X.squeeze(dim=d)
        Y = Y.squeeze(dim=d)
    return X, Y


def _taps(win, win_size, win_sigma, channels):
    """The window as n float32 taps on the host.  A given `win` ([C, 1, ..., n]) must have equal rows."""
    if win is None:
        return _fspecial_gauss_1d(win_size, win_sigma).reshape(-1).numpy()
    if not all(ws == 1 for ws in win.shape[1:-1]):
        raise AssertionError(win.shape)
    rows = win.detach().to("cpu", torch.float32).reshape(-1, win.shape[-1])
    if rows.shape[0] != channels:
        raise RuntimeError(f"win has {rows.shape[0]} rows for {channels} channels")
    if not bool((rows == rows[:1]).all()):
        raise NotImplementedError("a window that differs between channels: the kernel takes one set of taps")
    return rows[0].contiguous().numpy()


def _check_device(X):
    if X.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"metrics take uint8 or float32 tensors, got {X.dtype}")
    if not X.is_cuda:
        raise RuntimeError("teramind_amd.metrics has no CPU fallback: inputs must be device tensors")


def _rows_ok(t):
    return t.stride(-1) == 1 and t.stride(-2) >= t.shape[-1]


def _plane_calls(ts):
    """[(first image, planes per call, plane stride in elements per tensor)] covering [N, C, H, W] tensors `ts`: one call when
    the N x C planes of every tensor are evenly strided, else one call per image."""
    N, Cn = ts[0].shape[:2]
    if all(N == 1 or Cn == 1 or t.stride(0) == Cn * t.stride(1) for t in ts):
        return [(0, N * Cn, [t.stride(1) if Cn > 1 else t.stride(0) for t in ts])]
    return [(i, Cn, [t.stride(1) for t in ts]) for i in range(N)]


def _pix(t):
    return 1 if t.dtype == torch.float32 else 0            # TM_PIX_F32 / TM_PIX_U8


def ssim_sums(X, Y, taps, C1, C2):
    """float64 [N, C, 3] on the device: sum of the ssim map, of the cs map (valid region) and of (x - y)^2 (whole plane) for
    every plane of X, Y [N, C, H, W].  Any row pitch and plane stride is read in place; only a tensor whose last dimension
    is not dense is copied."""
    if not _rows_ok(X):
        X = X.contiguous()
    if not _rows_ok(Y):
        Y = Y.contiguous()
    N, Cn, H, W = X.shape
    n = int(taps.shape[0])
    if n > MAX_TAPS:
        raise NotImplementedError(f"a window of {n} taps: the kernel takes at most {MAX_TAPS}")
    if H < n or W < n:
        raise NotImplementedError(f"a {H} x {W} plane below the window of {n} taps (the reference skips the smoothing there)")
    esz = X.element_size()
    out = torch.empty((N, Cn, 3), dtype=torch.float64, device=X.device)
    w = np.ascontiguousarray(taps, dtype=np.float32)
    L = _lib.lib()
    with torch.cuda.device(X.device):
        for i0, P, (xs, ys) in _plane_calls((X, Y)):
            _lib.check(L.tm_ssim_planes(C.c_void_p(X[i0].data_ptr()), C.c_void_p(Y[i0].data_ptr()), _pix(X), P, H, W,
                                        X.stride(-2) * esz, xs * esz, Y.stride(-2) * esz, ys * esz,
                                        w.ctypes.data_as(C.POINTER(C.c_float)), n, float(C1), float(C2),
                                        C.c_void_p(out[i0].data_ptr()), _lib.current_stream_ptr()), "tm_ssim_planes")
    return out


def avgpool2_pad(X):
    """One MS-SSIM level of X [N, C, H, W]: F.avg_pool2d(X, kernel_size=2, padding=(H % 2, W % 2)) as float32."""
    if not _rows_ok(X):
        X = X.contiguous()
    N, Cn, H, W = X.shape
    esz = X.element_size()
    out = torch.empty((N, Cn, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=X.device)
    L = _lib.lib()
    with torch.cuda.device(X.device):
        for i0, P, (xs,) in _plane_calls((X,)):
            _lib.check(L.tm_avgpool2_pad(C.c_void_p(X[i0].data_ptr()), _pix(X), P, H, W, X.stride(-2) * esz, xs * esz,
                                         C.c_void_p(out[i0].data_ptr()), out.stride(-2) * 4, out.stride(1) * 4,
                                         _lib.current_stream_ptr()), "tm_avgpool2_pad")
    return out


def _vols_ok(t):
    H, W = t.shape[-2:]
    return _rows_ok(t) and t.stride(-3) >= (H - 1) * t.stride(-2) + W


def ssim_sums3(X, Y, taps, C1, C2):
    """float64 [N, C, 3] on the device: sum of the ssim map, of the cs map (the (D - n + 1)(H - n + 1)(W - n + 1) valid
    region of the 3-D window) and of (x - y)^2 (whole volume) for every volume of X, Y [N, C, D, H, W].  Any row pitch, depth
    stride and volume stride is read in place; only a tensor whose last dimension is not dense (or whose planes overlap) is
    copied."""
    if not _vols_ok(X):
        X = X.contiguous()
    if not _vols_ok(Y):
        Y = Y.contiguous()
    N, Cn, D, H, W = X.shape
    n = int(taps.shape[0])
    if n > MAX_TAPS_3D:
        raise NotImplementedError(f"a 3-D window of {n} taps: the kernel keeps the depth window in registers and takes at most "
                                  f"{MAX_TAPS_3D}")
    if H < n or W < n:
        raise NotImplementedError(f"a {H} x {W} plane below the window of {n} taps (the reference skips the smoothing there)")
    if D < n:
        raise NotImplementedError(f"a depth of {D} below the window of {n} taps: the plane route serves it")
    esz = X.element_size()
    out = torch.empty((N, Cn, 3), dtype=torch.float64, device=X.device)
    w = np.ascontiguousarray(taps, dtype=np.float32)
    L = _lib.lib()
    with torch.cuda.device(X.device):
        for i0, V, (xs, ys) in _plane_calls((X, Y)):
            _lib.check(L.tm_ssim_volumes(C.c_void_p(X[i0].data_ptr()), C.c_void_p(Y[i0].data_ptr()), _pix(X), V, D, H, W,
                                         X.stride(-2) * esz, X.stride(-3) * esz, xs * esz,
                                         Y.stride(-2) * esz, Y.stride(-3) * esz, ys * esz,
                                         w.ctypes.data_as(C.POINTER(C.c_float)), n, float(C1), float(C2),
                                         C.c_void_p(out[i0].data_ptr()), _lib.current_stream_ptr()), "tm_ssim_volumes")
    return out


def avgpool2_pad3(X):
    """One 5-D MS-SSIM level of X [N, C, D, H, W]: F.avg_pool3d(X, kernel_size=2, padding=(D % 2, H % 2, W % 2)) as float32."""
    if not _vols_ok(X):
        X = X.contiguous()
    N, Cn, D, H, W = X.shape
    esz = X.element_size()
    out = torch.empty((N, Cn, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=X.device)
    L = _lib.lib()
    with torch.cuda.device(X.device):
        for i0, V, (xs,) in _plane_calls((X,)):
            _lib.check(L.tm_avgpool2_pad3(C.c_void_p(X[i0].data_ptr()), _pix(X), V, D, H, W, X.stride(-2) * esz,
                                          X.stride(-3) * esz, xs * esz, C.c_void_p(out[i0].data_ptr()), out.stride(-2) * 4,
                                          out.stride(-3) * 4, out.stride(1) * 4, _lib.current_stream_ptr()), "tm_avgpool2_pad3")
    return out


def _ssim(X, Y, data_range, taps, K=(0.01, 0.03)):
    """(ssim_per_channel, cs, squared-error sums), float64 [N, C] each, of 4-D or 5-D X, Y (utils/metrics.py:266-305).  A 5-D
    input as deep as the window takes the 3-D window; a shallower one is smoothed in-plane only, as the reference does: its
    planes join the channels and are averaged afterwards (the means of equally many outputs)."""
    K1, K2 = K
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    n = int(taps.shape[0])
    if len(X.shape) == 5:
        N, Cn, D, H, W = X.shape
        if D >= n:
            s = ssim_sums3(X, Y, taps, C1, C2)
            count = (D - n + 1) * (H - n + 1) * (W - n + 1)
            return s[..., 0] / count, s[..., 1] / count, s[..., 2]
        s = ssim_sums(X.reshape(N, Cn * D, H, W), Y.reshape(N, Cn * D, H, W), taps, C1, C2).reshape(N, Cn, D, 3)
        count = (H - n + 1) * (W - n + 1)
        return s[..., 0].mean(-1) / count, s[..., 1].mean(-1) / count, s[..., 2].sum(-1)
    s = ssim_sums(X, Y, taps, C1, C2)
    count = (X.shape[-2] - n + 1) * (X.shape[-1] - n + 1)
    return s[..., 0] / count, s[..., 1] / count, s[..., 2]


def _as_planes(X, Y, win_size):
    """4-D as it is; 5-D with a depth below the window is smoothed in-plane only by the reference: its planes join the
    channels here and `groups` of them are averaged afterwards.  A deeper 5-D input is a volume (groups = 0)."""
    if len(X.shape) == 4:
        return X, Y, 1
    N, Cn, D, H, W = X.shape
    if D >= win_size:
        return X, Y, 0
    return X.reshape(N, Cn * D, H, W), Y.reshape(N, Cn * D, H, W), D


def _check_volume_device(X, text):
    """A 5-D host tensor is refused with NotImplementedError, the type such input was refused with while the package had no
    3-D window; it is a RuntimeError like every other 'no CPU fallback' refusal, so callers that catch that see no change."""
    if X.dtype in (torch.uint8, torch.float32) and not X.is_cuda:
        raise NotImplementedError(f"{text} on the device only: teramind_amd.metrics has no CPU fallback")


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
         nonnegative_ssim=False):
    """utils/metrics.py:308-364.  X, Y: device tensors [N, C, H, W] or [N, C, D, H, W] (the 3-D window when D reaches the
    window, else the planes averaged), float32 or uint8 (the extension)."""
    X, Y = _squeeze_pair(X, Y)
    if len(X.shape) not in (4, 5):
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {X.shape}")
    if not X.type() == Y.type():
        raise ValueError(f"Input images should have the same dtype, but got {X.type()} and {Y.type()}.")
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    taps = _taps(win, win_size, win_sigma, X.shape[1])
    N, Cn = X.shape[:2]
    Xp, Yp, groups = _as_planes(X, Y, win_size)
    if groups == 0:
        _check_volume_device(X, f"a 5-D input of depth {X.shape[2]} takes the 3-D window of {win_size} taps, which runs")
    _check_device(X)
    ssim_per_channel = _ssim(Xp, Yp, data_range, taps, K)[0].reshape(N, Cn, max(groups, 1)).mean(-1).float()
    if nonnegative_ssim:
        ssim_per_channel = torch.relu(ssim_per_channel)
    return ssim_per_channel.mean() if size_average else ssim_per_channel.mean(1)


def _ms_combine(mcs, ssim_last, weights):
    """utils/metrics.py:432-434 on float32 [N, C] tensors: relu, then the product of the weighted powers."""
    stack = torch.stack([torch.relu(c) for c in mcs] + [torch.relu(ssim_last)], dim=0)
    return torch.prod(stack ** weights.view(-1, 1, 1), dim=0)


def _ms_levels(X, Y, data_range, taps, K, levels):
    """[(ssim, cs, squared error)] of level 0 .. levels - 1, each pooled from the one before (5-D: along the depth too)."""
    pool = avgpool2_pad3 if len(X.shape) == 5 else avgpool2_pad
    out = []
    for i in range(levels):
        out.append(_ssim(X, Y, data_range, taps, K))
        if i < levels - 1:
            X, Y = pool(X), pool(Y)
    return out


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """utils/metrics.py:367-439 for 4-D or 5-D device tensors, float32 or uint8 (the extension).  5-D: every level is pooled
    along D, H and W; a level as deep as the window takes the 3-D window, a shallower one its planes averaged."""
    X, Y = _squeeze_pair(X, Y)
    if not X.type() == Y.type():
        raise ValueError(f"Input images should have the same dtype, but got {X.type()} and {Y.type()}.")
    if len(X.shape) not in (4, 5):
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {X.shape}")
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** 4), \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((win_size - 1) * (2 ** 4))
    if weights is None:
        weights = list(MS_WEIGHTS)
    taps = _taps(win, win_size, win_sigma, X.shape[1])
    if len(X.shape) == 5:
        _check_volume_device(X, "5-D ms_ssim pools and smooths along the depth, which runs")
        if win_size > MAX_TAPS_3D and X.shape[2] >= win_size:
            raise NotImplementedError(f"a 3-D window of {win_size} taps: the kernel takes at most {MAX_TAPS_3D}")
    _check_device(X)
    weights = torch.tensor(weights, dtype=torch.float32, device=X.device)
    lv = _ms_levels(X, Y, data_range, taps, K, weights.shape[0])
    val = _ms_combine([l[1].float() for l in lv[:-1]], lv[-1][0].float(), weights)
    return val.mean() if size_average else val.mean(1)


class PSNR(torch.nn.Module):
    """utils/metrics.py:201-215: 20 log10(mval / sqrt(mse)) per image of [N, H, W] or [N, C, H, W]; inf for equal images.
    The squared-error sums are those of `tm_ssim_planes` (exact for uint8), so a plane has at least 3 x 3 pixels."""

    def __init__(self, mval=255.):
        super().__init__()
        self.mval = mval

    def forward(self, img1, img2):
        if img1.shape != img2.shape or img1.dtype != img2.dtype:
            raise ValueError(f"Input images should have the same shape and dtype, but got {img1.shape} {img1.dtype} and "
                             f"{img2.shape} {img2.dtype}.")
        if len(img1.shape) == 3:
            img1, img2 = img1[:, None], img2[:, None]
        elif len(img1.shape) != 4:
            raise ValueError(f"Input images should be 3-d or 4-d tensors, but got {img1.shape}")
        _check_device(img1)
        sq = ssim_sums(img1, img2, np.array([0.0, 1.0, 0.0], dtype=np.float32), 1.0, 1.0)[..., 2].sum(1)
        return psnr_from_sq(sq, img1[0].numel(), self.mval)


def psnr_from_sq(sq, pixels, mval=255.):
    """float32 PSNR from float64 squared-error sums over `pixels` pixels each."""
    return (20 * torch.log10(mval / torch.sqrt(sq / pixels))).float()


class SSIM(torch.nn.Module):
    """utils/metrics.py:442-491."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 K=(0.01, 0.03), nonnegative_ssim=False, unsqueeze=False):
        super().__init__()
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim
        self.unsqueeze = unsqueeze

    def forward(self, X, Y):
        if self.unsqueeze:                                  # [N, H, W] input: add the channel
            assert len(X.shape) == len(Y.shape) == 3
            X = X.unsqueeze(1)
            Y = Y.unsqueeze(1)
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    """utils/metrics.py:494-541; a 3-D input takes the "gray" route (one channel, the one-row window)."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 weights=None, K=(0.01, 0.03), unsqueeze=False):
        super().__init__()
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.win_gray = _fspecial_gauss_1d(win_size, win_sigma).repeat([1, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights
        self.K = K
        self.unsqueeze = unsqueeze

    def forward(self, X, Y):
        is_gray = False
        if len(X.shape) == 3:
            X, Y = X[:, None], Y[:, None]
            is_gray = True
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average,
                       win=self.win_gray if is_gray else self.win, weights=self.weights, K=self.K)


def ms_ssim_fits(H, W, win_size=11):
    """The reference's size rule for the four downsamplings (utils/metrics.py:408-411)."""
    return min(H, W) > (win_size - 1) * (2 ** 4)


def compare_mosaics(gen_u8, real_u8, ms=True, device=None, win_size=11, win_sigma=1.5,
                    weights: Optional[Sequence[float]] = None):
    """Per-plane measures of two uint8 mosaics [K, H, W] (as `stitch.stitch_dir` / `stitch_real_dir` return; host or device),
    data range 255: {"psnr": [K], "ssim": [K], "ms_ssim": [K]} as Python floats.  "ms_ssim" is absent with ms=False or when
    the plane is too small for the four downsamplings.  One plane pair is resident at a time; level 0 is read once for all
    three measures."""
    if tuple(gen_u8.shape) != tuple(real_u8.shape) or len(gen_u8.shape) != 3:
        raise ValueError(f"mosaics should be [K, H, W] of one shape, but got {tuple(gen_u8.shape)} and {tuple(real_u8.shape)}")
    if any(str(a.dtype).split(".")[-1] != "uint8" for a in (gen_u8, real_u8)):
        raise TypeError(f"mosaics should be uint8, got {gen_u8.dtype} and {real_u8.dtype}")
    on_dev = isinstance(gen_u8, torch.Tensor) and gen_u8.is_cuda
    dev = torch.device(device) if device is not None else (gen_u8.device if on_dev else torch.device("cuda"))

    def plane(a, k):                                        # one [1, 1, H, W] plane on the device
        t = torch.from_numpy(np.array(a[k])) if isinstance(a, np.ndarray) else a[k]
        return t.to(dev)[None, None]
    K_, H, W = gen_u8.shape
    taps = _fspecial_gauss_1d(win_size, win_sigma).reshape(-1).numpy()
    do_ms = bool(ms) and ms_ssim_fits(H, W, win_size)
    wts = torch.tensor(list(MS_WEIGHTS) if weights is None else list(weights), dtype=torch.float32, device=dev)
    rows = []
    for k in range(K_):
        g, r = plane(gen_u8, k), plane(real_u8, k)
        lv = _ms_levels(g, r, 255, taps, (0.01, 0.03), wts.shape[0] if do_ms else 1)
        row = [psnr_from_sq(lv[0][2].reshape(1), H * W), lv[0][0].float().reshape(1)]
        if do_ms:
            row.append(_ms_combine([l[1].float() for l in lv[:-1]], lv[-1][0].float(), wts).reshape(1))
        rows.append(torch.cat(row))
    res = torch.stack(rows).cpu().tolist()                  # the one synchronisation
    out = {"psnr": [r[0] for r in res], "ssim": [r[1] for r in res]}
    if do_ms:
        out["ms_ssim"] = [r[2] for r in res]
    return out


def compare_volumes(gen_u8, real_u8, n_stain=2, ms=True, device=None, win_size=11, win_sigma=1.5,
                    weights: Optional[Sequence[float]] = None):
    """Per-stain measures over the slice stack of two uint8 '(s c)' mosaics [K, H, W] (slice-major, stain-minor; host or
    device), data range 255: {"psnr3d": [n_stain], "ssim3d": [n_stain], "ms_ssim3d": [n_stain]} as Python floats.  The volume
    of stain c is every n_stain-th plane from c, [1, 1, K / n_stain, H, W], read in place through its depth stride.
    "ms_ssim3d" is absent with ms=False or when the plane is too small for the four downsamplings (the reference's rule looks
    at H and W only).  Both mosaics are resident; level 0 is read once for all three measures; one synchronisation."""
    if tuple(gen_u8.shape) != tuple(real_u8.shape) or len(gen_u8.shape) != 3:
        raise ValueError(f"mosaics should be [K, H, W] of one shape, but got {tuple(gen_u8.shape)} and {tuple(real_u8.shape)}")
    if any(str(a.dtype).split(".")[-1] != "uint8" for a in (gen_u8, real_u8)):
        raise TypeError(f"mosaics should be uint8, got {gen_u8.dtype} and {real_u8.dtype}")
    K_, H, W = gen_u8.shape
    if n_stain < 1 or K_ % n_stain:
        raise ValueError(f"{K_} planes are no whole number of slices of {n_stain} stains")
    D = K_ // n_stain
    if D < win_size or min(H, W) < win_size:
        raise ValueError(f"a stain's volume of {D} x {H} x {W} is below the 3-D window of {win_size} taps")
    on_dev = isinstance(gen_u8, torch.Tensor) and gen_u8.is_cuda
    dev = torch.device(device) if device is not None else (gen_u8.device if on_dev else torch.device("cuda"))

    def mosaic(a):
        if isinstance(a, np.ndarray):                       # torch refuses to wrap a read-only array quietly
            a = torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else np.array(a))
        return a.to(dev)
    g, r = mosaic(gen_u8), mosaic(real_u8)
    taps = _fspecial_gauss_1d(win_size, win_sigma).reshape(-1).numpy()
    do_ms = bool(ms) and ms_ssim_fits(H, W, win_size)
    wts = torch.tensor(list(MS_WEIGHTS) if weights is None else list(weights), dtype=torch.float32, device=dev)
    rows = []
    for c in range(n_stain):
        lv = _ms_levels(g[c::n_stain][None, None], r[c::n_stain][None, None], 255, taps, (0.01, 0.03),
                        wts.shape[0] if do_ms else 1)
        row = [psnr_from_sq(lv[0][2].reshape(1), D * H * W), lv[0][0].float().reshape(1)]
        if do_ms:
            row.append(_ms_combine([l[1].float() for l in lv[:-1]], lv[-1][0].float(), wts).reshape(1))
        rows.append(torch.cat(row))
    res = torch.stack(rows).cpu().tolist()                  # the one synchronisation
    out = {"psnr3d": [x[0] for x in res], "ssim3d": [x[1] for x in res]}
    if do_ms:
        out["ms_ssim3d"] = [x[2] for x in res]
    return out
