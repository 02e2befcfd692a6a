"""Shared by tests/test_heatmap_cases_host.py, tests/test_gpu_heatmap.py and tests/test_gpu_export_heatmap.py: the attention
heat map (include/teramind_hip.h, tm_heat_field / tm_heat_render) restated in numpy, the seeded cases, the error bound of the
field and the list of wrong variants the bound must tell apart.

THE FIELD is held to a bound against `field_model` in float64 (which is scipy.ndimage.gaussian_filter of the reference's
expression, test_attn.py:204-206; the host test checks that to 1e-12).  THE BOUND, with U = 2^-24 (float32 unit roundoff),
g(k) = k U / (1 - k U) (k roundings compounded), nsum summed channels, n = 2 r + 1 taps t >= 0 (the float32 taps, taken as
given; S = their sum in float64), fmax = max |f| and pmax = max |p| over the case's exact field:
  * float16 -> float32 and max(., 0) are exact; v, v * wei and + 1 are nsum - 1 additions, a multiplication and an addition of
    non-negative terms: the argument of the logarithm carries a relative error d <= g(nsum + 1)
  * log2 of the perturbed argument moves by at most e_log = -log2(1 - d); a log2 admitted at 2 ulp <= 4 U relative adds
    4 U (fmax + e_log):  e_f = e_log + 4 U (fmax + e_log).  The mask is exact, so e_p = e_f on the cells it keeps.
  * a pass of n multiply-adds from zero (fused or not) over values of magnitude <= M carrying errors <= e gives errors
    <= S e + g(n) S (M + e): after axis 0  e1 = S e_f + g(n) S (pmax + e_f)  on values of magnitude <= S pmax, after axis 1
    e2 = S e1 + g(n) S (S pmax + e1).
`field_bound` returns e2; for the cases here it is 2e-6 .. 3e-5, against fields of order 1.  Nothing in it was tuned on what the
kernel returns.

THE RENDER is exact: `render_ref` walks tm_heat_render's pixel rule in numpy float32, every operation rounded once, and the
kernel is held to its bytes.
"""
import functools
import math
import zlib

import numpy as np

U = 2.0 ** -24
f32 = np.float32
TILE_H, TILE_W = 32, 64            # tm_heatmap.hip HF_TH, HF_TW: the output tile of one workgroup
SCALES = (1, 2, 4, 8, 16)


def gamma(k):
    return k * U / (1 - k * U)


# ---- taps --------------------------------------------------------------------------------------------------------------
def gaussian_taps64(sigma, truncate=4.0):
    """scipy.ndimage._filters._gaussian_kernel1d: (r, float64 [2 r + 1])."""
    r = int(truncate * float(sigma) + 0.5)
    if r == 0:
        return 0, np.ones(1)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return r, w / w.sum()


def gaussian_taps(sigma, truncate=4.0):
    """The taps the library is given: the float64 ones cast once."""
    r, w = gaussian_taps64(sigma, truncate)
    return r, w.astype(f32)


# ---- the field ---------------------------------------------------------------------------------------------------------
def reflect_index(n, r, kind="reflect"):
    """Source index of positions -r .. n - 1 + r: 'reflect' = scipy's half-sample reflection R(-j) = j - 1,
    R(n - 1 + j) = n - j; 'mirror' = whole-sample, R(-j) = j, R(n - 1 + j) = n - 1 - j (needs r < n)."""
    i = np.arange(-r, n + r)
    if kind == "reflect":
        i = np.where(i < 0, -i - 1, i)
        i = np.where(i >= n, 2 * n - 1 - i, i)
    else:
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
    assert i.min() >= 0 and i.max() < n, "one reflection must suffice"
    return i


def mode_ranges(K, mode, gene=None):
    """(sum0, nsum, mask0, nmask) in the [4K] channels (test_attn.py:204-206, 228-229, 253-258)."""
    if mode == "expr":
        return 3 * K + gene, 1, 0, 0
    return {"att_up": 0, "att_dn": K, "att_all": 2 * K}[mode], K, 3 * K, K


def pointwise(src, sum0, nsum, wei, mask0, nmask, dtype=np.float64, log=np.log2, plus=1.0, any_gene=False):
    """(f, m): f = log2(v * wei + 1) with v the clamped channel sum in index order, m the mask (bool), in `dtype`."""
    s = src.astype(dtype)
    v = np.zeros(s.shape[1:], dtype=dtype)
    for c in range(sum0, sum0 + nsum):
        v = v + np.maximum(s[c], dtype(0))
    with np.errstate(divide="ignore"):
        f = log(v * dtype(wei) + dtype(plus)).astype(dtype)
    nz = src[mask0:mask0 + nmask] != 0
    m = (nz.any(0) if any_gene else nz.all(0)) if nmask else np.ones(s.shape[1:], dtype=bool)
    return f, m


def separable(p, taps, pad="reflect"):
    """Axis 0 first, then axis 1; per output the taps in order from zero, in p's dtype."""
    dt = p.dtype.type
    r = (len(taps) - 1) // 2
    H, W = p.shape
    if pad == "zero":
        P = np.zeros((H + 2 * r, W + 2 * r), dtype=p.dtype)
        P[r:r + H, r:r + W] = p
    else:
        P = p[reflect_index(H, r, pad)][:, reflect_index(W, r, pad)]
    a = np.zeros((H, W + 2 * r), dtype=p.dtype)
    with np.errstate(invalid="ignore"):
        for j, t in enumerate(taps):
            a = a + dt(t) * P[j:j + H]
        out = np.zeros((H, W), dtype=p.dtype)
        for j, t in enumerate(taps):
            out = out + dt(t) * a[:, j:j + W]
    return out


def field_model(src, sum0, nsum, wei, mask0, nmask, taps, dtype=np.float64):
    """tm_heat_field's definition in `dtype` arithmetic (float64: the reference of the tests; float32: a walk of it)."""
    f, m = pointwise(src, sum0, nsum, f32(wei), mask0, nmask, dtype)
    return separable(np.where(m, f, dtype(0)), taps)


def field_bound(src, sum0, nsum, wei, mask0, nmask, taps):
    """The derivation of the module docstring."""
    f, m = pointwise(src, sum0, nsum, f32(wei), mask0, nmask)
    fmax = float(np.abs(f).max())
    pmax = float(np.abs(np.where(m, f, 0.0)).max())
    n, S = len(taps), float(np.asarray(taps, dtype=np.float64).sum())
    e_log = -math.log2(1 - gamma(nsum + 1))
    e_f = e_log + 4 * U * (fmax + e_log)
    e1 = S * e_f + gamma(n) * S * (pmax + e_f)
    return S * e1 + gamma(n) * S * (S * pmax + e1)


# ---- wrong variants: each a field in float64 that a correct kernel must NOT give ---------------------------------------------
def _v_pad(kind):
    def fn(src, sum0, nsum, wei, mask0, nmask, taps, K):
        f, m = pointwise(src, sum0, nsum, f32(wei), mask0, nmask)
        return separable(np.where(m, f, 0.0), taps, kind)
    return fn


def _v_taps(change):
    def fn(src, sum0, nsum, wei, mask0, nmask, taps, K):
        f, m = pointwise(src, sum0, nsum, f32(wei), mask0, nmask)
        return separable(np.where(m, f, 0.0), change(np.asarray(taps, dtype=np.float64)))
    return fn


def _v_point(**kw):
    def fn(src, sum0, nsum, wei, mask0, nmask, taps, K):
        f, m = pointwise(src, sum0, nsum, f32(wei), mask0, nmask, **kw)
        return separable(np.where(m, f, 0.0), taps)
    return fn


def _v_mask_after(src, sum0, nsum, wei, mask0, nmask, taps, K):
    f, m = pointwise(src, sum0, nsum, f32(wei), mask0, nmask)
    return separable(f, taps) * m


def _v_no_wei(src, sum0, nsum, wei, mask0, nmask, taps, K):
    return field_model(src, sum0, nsum, 1.0, mask0, nmask, taps)


def _v_shift(src, sum0, nsum, wei, mask0, nmask, taps, K):
    return field_model(src, (sum0 + K) % (4 * K), nsum, wei, mask0, nmask, taps)


def _shorter(t):
    t = t[1:-1]
    return t / t.sum()


VARIANTS = {
    "zero_pad": _v_pad("zero"),                                   # zero padding instead of reflection
    "mirror": _v_pad("mirror"),                                   # whole-sample reflection (scipy mode='mirror')
    "radius_minus_1": _v_taps(_shorter),                          # the Gaussian cut at r - 1, normalised again
    "unnormalised": _v_taps(lambda t: t / t.max()),               # exp(-x^2 / 2 sigma^2) as it is
    "mask_after": _v_mask_after,                                  # mask applied after the filter
    "mask_any": _v_point(any_gene=True),                          # any gene expressed instead of all
    "ln": _v_point(log=np.log),                                   # natural logarithm
    "no_wei": _v_no_wei,                                          # wei left out
    "no_plus_1": _v_point(plus=0.0),                              # the + 1 left out
    "sum_shift": _v_shift,                                        # sum range shifted by K
}
_FILTER_V = ("zero_pad", "radius_minus_1", "unnormalised")
_POINT_V = ("ln", "no_plus_1", "sum_shift")
_MASK_V = ("mask_after", "mask_any")


# ---- field cases -------------------------------------------------------------------------------------------------------
#   name: (K, H, W, sigma, mode, gene)
FIELD_CASES = {
    "s4_16x16": (2, 16, 16, 4.0, "att_all", None),                # r = 16 = H = W: both reflections meet in every window
    "s2_16x16": (2, 16, 16, 2.0, "att_all", None),
    "odd_17x33": (2, 17, 33, 2.0, "att_up", None),
    "tiles_70x150": (2, 70, 150, 2.0, "att_all", None),           # two workgroup tiles and a remainder both ways, r = 8
    "tiles_s4_70x150": (1, 70, 150, 4.0, "att_dn", None),         # the same through the run-time radius
    "s05_16x40": (2, 16, 40, 0.5, "att_dn", None),
    "s0_16x16": (2, 16, 16, 0.0, "att_all", None),                # r = 0: the identity
    "k1_17x33": (1, 17, 33, 2.0, "att_all", None),
    "k8_33x70": (8, 33, 70, 2.0, "att_all", None),
    "expr_17x33": (2, 17, 33, 2.0, "expr", 1),
}
WEI = 229


def variants_of(name):
    """The wrong variants that are wrong for this case: filter variants need r >= 1 (mirror also r < H, W), mask variants a
    mask ('any' differs from 'all' from two genes on), 'no_wei' a wei other than 1."""
    K, H, W, sigma, mode, gene = FIELD_CASES[name]
    r = gaussian_taps(sigma)[0]
    out = list(_POINT_V)
    if r >= 1:
        out += list(_FILTER_V) + (["mirror"] if r < min(H, W) else [])
    if mode != "expr":
        out += ["no_wei"] + (["mask_any"] if K >= 2 else []) + (["mask_after"] if r >= 1 else [])
    return out


@functools.lru_cache(maxsize=None)
def mosaic_slice(name):
    """float16 [4K, H, W]: the attention channels [0, 3K) are fp16 values in [0, 0.05] (2 % of them small negatives, which the
    clamp removes), the expression channels [3K, 4K) small integers with about 40 % zeros, placed independently per gene."""
    K, H, W = FIELD_CASES[name][:3]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    att = rng.random((3 * K, H, W)) * 0.05
    att[rng.random(att.shape) < 0.02] = -0.01
    expr = rng.integers(1, 6, (K, H, W)) * (rng.random((K, H, W)) >= 0.4)
    a = np.concatenate([att, expr]).astype(np.float16)
    a.setflags(write=False)
    return a


def field_args(name):
    """(sum0, nsum, wei, mask0, nmask, r, float32 taps) of a case, as the library is called."""
    K, H, W, sigma, mode, gene = FIELD_CASES[name]
    sum0, nsum, mask0, nmask = mode_ranges(K, mode, gene)
    r, taps = gaussian_taps(sigma)
    return sum0, nsum, (1.0 if mode == "expr" else float(WEI)), mask0, nmask, r, taps


@functools.lru_cache(maxsize=None)
def field_reference(name):
    """(float64 model, bound) of a case, computed once per process and shared (not to be changed)."""
    sum0, nsum, wei, mask0, nmask, r, taps = field_args(name)
    src = mosaic_slice(name)
    ref = field_model(src, sum0, nsum, wei, mask0, nmask, taps)
    ref.setflags(write=False)
    return ref, field_bound(src, sum0, nsum, wei, mask0, nmask, taps)


def variant_field(name, variant):
    sum0, nsum, wei, mask0, nmask, r, taps = field_args(name)
    return VARIANTS[variant](mosaic_slice(name), sum0, nsum, wei, mask0, nmask, taps, FIELD_CASES[name][0])


# ---- the render --------------------------------------------------------------------------------------------------------
def two_colour(end, n=100, start=(0, 0, 0)):
    """Row j = trunc((start + (end - start) j / (n - 1)) 255): LinearSegmentedColormap.from_list(N=n) as bytes."""
    st, ed = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    return ((st + (ed - st) * (np.arange(n, dtype=np.float64)[:, None] / (n - 1))) * 255).astype(np.uint8)


def _axis32(n_out, n_in, scale):
    s = (np.arange(n_out).astype(f32) + f32(0.5)) * f32(1.0 / scale) - f32(0.5)
    s = np.minimum(np.maximum(s, f32(0)), f32(n_in - 1))
    i0 = s.astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), (s - i0.astype(f32)).astype(f32)


def resample_ref(field, scale):
    """g of tm_heat_render in float32, one rounding per operation."""
    fld = np.asarray(field, dtype=f32)
    H, W = fld.shape
    y0, y1, wy = _axis32(H * scale, H, scale)
    x0, x1, wx = _axis32(W * scale, W, scale)
    wy, wx = wy[:, None], wx[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        f00, f01, f10, f11 = fld[y0][:, x0], fld[y0][:, x1], fld[y1][:, x0], fld[y1][:, x1]
        top = (f00 + ((f01 - f00) * wx).astype(f32)).astype(f32)
        bot = (f10 + ((f11 - f10) * wx).astype(f32)).astype(f32)
        return (top + ((bot - top).astype(f32) * wy).astype(f32)).astype(f32)


def index_ref(g, vmin, vmax, N):
    """idx = !(i >= 0) ? 0 : min(N - 1, (int)i), i = ((g - vmin) * inv_range) * N in float32."""
    inv_range = f32(1.0 / (float(vmax) - float(vmin)))
    with np.errstate(invalid="ignore", over="ignore"):
        i = (((g.astype(f32) - f32(vmin)).astype(f32) * inv_range).astype(f32) * f32(N)).astype(f32)
        i = np.where(i >= 0, np.minimum(i, f32(N)), f32(0))        # NaN and negatives -> 0, large values capped before the cast
    return np.minimum(N - 1, i.astype(np.int64))


def render_ref(field, lut, vmin=0.0, vmax=1.0, scale=1, floor=0):
    """uint8 [H scale, W scale, 3]: the bytes tm_heat_render writes (interleaved; plane c is [..., c])."""
    lut = np.asarray(lut, dtype=np.uint8)
    idx = index_ref(resample_ref(field, scale), vmin, vmax, len(lut))
    return np.where((idx < floor)[..., None], np.uint8(0), lut[idx]).astype(np.uint8)


def resample64(field, scale):
    """The same geometry in float64 (the host test holds it to F.interpolate(mode='bilinear', align_corners=False))."""
    fld = np.asarray(field, dtype=np.float64)
    H, W = fld.shape

    def axis(n_out, n_in):
        s = np.clip((np.arange(n_out) + 0.5) / scale - 0.5, 0, n_in - 1)
        i0 = s.astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0
    y0, y1, wy = axis(H * scale, H)
    x0, x1, wx = axis(W * scale, W)
    wy, wx = wy[:, None], wx[None, :]
    top = fld[y0][:, x0] + (fld[y0][:, x1] - fld[y0][:, x0]) * wx
    bot = fld[y1][:, x0] + (fld[y1][:, x1] - fld[y1][:, x0]) * wx
    return top + (bot - top) * wy


RENDER_SHAPES = ((7, 5), (33, 17))
VMIN, VMAX = 0.25, 2.0


@functools.lru_cache(maxsize=None)
def render_field(shape):
    """float32 [H, W] spread over [vmin - 0.5, vmax + 0.5] with cells below vmin, equal to vmin and vmax, above vmax, and NaN."""
    H, W = shape
    rng = np.random.default_rng(zlib.crc32(f"render/{H}x{W}".encode()))
    a = (VMIN - 0.5 + rng.random((H, W)) * (VMAX - VMIN + 1.0)).astype(f32)
    a[0, 0], a[0, 1], a[1, 0], a[1, 1] = VMIN - 1, VMAX, VMAX + 3, VMIN
    a[H - 1, W - 1], a[H // 2, W // 2] = VMAX, np.nan
    a[2, 3] = np.inf
    a.setflags(write=False)
    return a


# ---- the export test's mosaic ------------------------------------------------------------------------------------------
EXPORT_SHAPE = (2, 8, 48, 80)      # [S, 4K, H, W], K = 2


@functools.lru_cache(maxsize=None)
def export_mosaic():
    """float16 [2, 8, 48, 80] in the layout of stitch_attn_dir: smooth attention channels (so that the map has structure at
    every pyramid level) times noise, expression as in `mosaic_slice` with one gene silent in the right third, where the masked
    field falls to 0 (table entry 0: below the export's floor, transparent in the blend)."""
    S, C4, H, W = EXPORT_SHAPE
    K = C4 // 4
    rng = np.random.default_rng(zlib.crc32(b"export"))
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    att = np.stack([[0.025 * (1 + np.sin(x / (5.0 + c) + s) * np.cos(y / (7.0 - 0.5 * c))) for c in range(3 * K)] for s in range(S)])
    att = att * (0.5 + 0.5 * rng.random(att.shape))
    expr = rng.integers(1, 6, (S, K, H, W)) * (rng.random((S, K, H, W)) >= 0.4)
    expr[:, 0, :, 52:] = 0                                         # gene 0 silent on the right: the mask empties the field there
    a = np.concatenate([att, expr], 1).astype(np.float16)
    a.setflags(write=False)
    return a
