"""No GPU: the heat-map restatements of heatmap_cases.py are what they claim to be.  The float64 field model is
scipy.ndimage.gaussian_filter of the reference's expression; the tables and the index rule are matplotlib's bytes; the
resampling geometry is F.interpolate's; the derived field bound holds a float32 walk of the model and rejects every wrong
variant; the package's host-side pieces (taps, tables, pathway data) equal the restated ones."""
import numpy as np
import pytest
import torch

import heatmap_cases as hc
from teramind_amd import attn_maps, heatmap

NAMES = list(hc.FIELD_CASES)


@pytest.mark.parametrize("name", NAMES)
def test_field_model_is_scipys_gaussian_filter_of_the_reference_expression(name):
    ndi = pytest.importorskip("scipy.ndimage")
    K, H, W, sigma, mode, gene = hc.FIELD_CASES[name]
    gen = np.maximum(hc.mosaic_slice(name).astype(np.float64), 0)          # gen_img clamps at 0 when it loads (test_attn.py:156)
    sum0, nsum, wei, mask0, nmask, r, taps = hc.field_args(name)
    taps64 = hc.gaussian_taps64(sigma)[1]
    ours = hc.field_model(hc.mosaic_slice(name), sum0, nsum, wei, mask0, nmask, taps64)
    if mode == "expr":                                                       # test_attn.py:228-229
        want = ndi.gaussian_filter(np.log2(gen[3 * K + gene] + 1), sigma=sigma)
    else:                                                                    # test_attn.py:192-206, 253-258
        msk = True
        for gi in range(K):
            msk = msk & (gen[3 * K + gi] != 0)
        want = ndi.gaussian_filter(np.log2(gen[sum0:sum0 + K].sum(0) * wei + 1) * msk, sigma=sigma)
    assert np.abs(ours - want).max() <= 1e-12
    # and the float32 taps the library gets move the field by no more than their own rounding
    assert np.abs(hc.field_reference(name)[0] - want).max() <= 4 * hc.U * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", NAMES)
def test_float32_walk_stays_inside_the_bound_and_every_wrong_variant_leaves_it(name):
    ref, bound = hc.field_reference(name)
    sum0, nsum, wei, mask0, nmask, r, taps = hc.field_args(name)
    walk = hc.field_model(hc.mosaic_slice(name), sum0, nsum, wei, mask0, nmask, taps, dtype=np.float32)
    assert walk.dtype == np.float32
    d = np.abs(walk.astype(np.float64) - ref).max()
    print(f"{name}: bound {bound:.3e}, float32 walk max|d| / bound = {d / bound:.3f}, max|field| = {np.abs(ref).max():.3f}")
    assert 0 < bound < 1e-4 and d <= bound
    for v in hc.variants_of(name):
        with np.errstate(invalid="ignore"):
            dv = np.abs(hc.variant_field(name, v) - ref)
        worst = np.nanmax(dv)
        print(f"    variant {v}: max|d| / bound = {worst / bound:.3g}")
        assert worst > bound, v


def test_every_variant_is_listed_somewhere_and_the_data_is_as_stated():
    listed = set()
    for name in NAMES:
        listed |= set(hc.variants_of(name))
        K, H, W, sigma, mode, gene = hc.FIELD_CASES[name]
        a = hc.mosaic_slice(name).astype(np.float64)
        assert a[:3 * K].max() <= 0.05 and a[:3 * K].min() >= -0.0101
        zeros = (a[3 * K:] == 0).mean()
        assert 0.3 < zeros < 0.5 and np.array_equal(a[3 * K:], np.round(a[3 * K:]))
        r = hc.gaussian_taps(sigma)[0]
        if mode != "expr" and r >= 1:
            m = (a[3 * K:] != 0).all(0)
            assert m.any() and not m.all()
            ys, xs = np.nonzero(m)
            near = np.zeros_like(m)
            for y, x in zip(ys, xs):
                near[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
            assert (near & ~m).any(), "a masked-out cell within r of an unmasked one"
    assert listed == set(hc.VARIANTS)
    assert {c[4] for c in hc.FIELD_CASES.values()} == set(heatmap.MODES)


def test_package_taps_tables_and_ranges_equal_the_restated_ones():
    for sigma in (0.0, 0.5, 2.0, 4.0):
        r, t = heatmap.gaussian_taps(sigma)
        r2, t2 = hc.gaussian_taps(sigma)
        assert r == r2 and t.dtype == np.float32 and np.array_equal(t, t2)
    assert heatmap.gaussian_taps(0) == (0, np.ones(1, dtype=np.float32))
    assert [heatmap.gaussian_taps(s)[0] for s in (2.0, 4.0)] == [8, 16]
    assert heatmap.INFERNO.shape == (256, 3) and heatmap.INFERNO.dtype == np.uint8
    assert tuple(heatmap.INFERNO[0]) == (0, 0, 3) and tuple(heatmap.INFERNO[-1]) == (252, 254, 164)
    for end in ((0, 1, 0.82), (0.89, 0, 1)):
        assert np.array_equal(heatmap.two_colour(end), hc.two_colour(end))
        assert np.array_equal(heatmap.two_colour(end, 17, (0.1, 0.2, 0.3)), hc.two_colour(end, 17, (0.1, 0.2, 0.3)))
    for K in (1, 2, 8):
        for mode in heatmap.MODES:
            assert heatmap.mode_ranges(K, mode, K - 1) == hc.mode_ranges(K, mode, K - 1)
    assert set(heatmap.PATHWAY_COLOURS) == set(heatmap.PATHWAY_VMAX) == set(attn_maps.PATHWAYS)
    for p, genes in attn_maps.PATHWAYS.items():
        assert len(heatmap.PATHWAY_COLOURS[p]) >= len(genes) == len(heatmap.PATHWAY_VMAX[p]["expr"])
    assert heatmap.gene_weight(229) == 229 and heatmap.gene_weight(500) == 500
    with pytest.raises(ValueError, match="gene"):
        heatmap.mode_ranges(2, "expr")
    with pytest.raises(ValueError, match="mode"):
        heatmap.mode_ranges(2, "att_updn")


def _probe_values(N, n=100000):
    """float64 in [0, 1) at least 1e-6 from every bin edge k / N, plus 0, 1, -0.5 and 1.5."""
    rng = np.random.default_rng(N)
    k = rng.integers(0, N, n)
    u = (k + 1e-6 * N + rng.random(n) * (1 - 2e-6 * N)) / N
    return np.concatenate([u, [0.0, 1.0, -0.5, 1.5]])


@pytest.mark.parametrize("which", ["inferno", "two_colour"])
def test_tables_and_index_rule_are_matplotlibs_bytes(which):
    mpl = pytest.importorskip("matplotlib")
    from matplotlib import cm, colors
    if which == "inferno":
        cmap, lut = cm.inferno, heatmap.INFERNO
    else:
        end = heatmap.PATHWAY_COLOURS["GLUT"][0]
        cmap, lut = colors.LinearSegmentedColormap.from_list("Custom", [(0, 0, 0), end], N=100), heatmap.two_colour(end)
    N = len(lut)
    assert np.array_equal(cmap(np.arange(N), bytes=True)[:, :3], lut), mpl.__version__
    u = _probe_values(N)
    want = cmap(colors.Normalize(0.0, 1.0)(u), bytes=True)[:, :3]
    got = hc.render_ref(u.astype(np.float32)[None, :], lut, 0.0, 1.0)[0]
    assert np.array_equal(got, want)
    # another range: Normalize(vmin, vmax) then the same rule
    v = 0.25 + u * 1.75
    want = cmap(colors.Normalize(0.25, 2.0)(v), bytes=True)[:, :3]
    got = hc.render_ref(v.astype(np.float32)[None, :], lut, 0.25, 2.0)[0]
    assert (got != want).any(-1).mean() < 1e-3                    # float32 v: a value within 1e-7 of an edge may change bins
    assert np.array_equal(got[-4:], want[-4:])


def test_every_pathway_palette_is_matplotlibs():
    pytest.importorskip("matplotlib")
    from matplotlib import colors
    for p, ends in heatmap.PATHWAY_COLOURS.items():
        for end in ends:
            cmap = colors.LinearSegmentedColormap.from_list("Custom", [(0, 0, 0), end], N=100)
            assert np.array_equal(cmap(np.arange(100), bytes=True)[:, :3], heatmap.two_colour(end)), (p, end)


@pytest.mark.parametrize("shape", hc.RENDER_SHAPES)
@pytest.mark.parametrize("scale", hc.SCALES)
def test_resampling_geometry_is_bilinear_interpolate(shape, scale):
    rng = np.random.default_rng(3)
    fld = rng.standard_normal(shape)
    want = torch.nn.functional.interpolate(torch.from_numpy(fld)[None, None], scale_factor=scale, mode="bilinear",
                                           align_corners=False)[0, 0].numpy()
    got = hc.resample64(fld, scale)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    g32 = hc.resample_ref(fld.astype(np.float32), scale)
    assert g32.dtype == np.float32 and np.abs(g32 - hc.resample64(fld.astype(np.float32), scale)).max() <= 8 * hc.U * np.abs(fld).max()
    if scale == 1:
        assert np.array_equal(g32, fld.astype(np.float32))


def test_render_restatement_edges():
    lut = hc.two_colour((0, 1, 0.82), 100)
    f = np.array([[-1.0, 0.25, 2.0, 5.0, np.nan, 0.25 + 1.75 * 0.5]], dtype=np.float32)
    idx = hc.index_ref(f, 0.25, 2.0, 100)
    assert idx.tolist() == [[0, 0, 99, 99, 0, 50]]
    out = hc.render_ref(f, lut, 0.25, 2.0, floor=3)
    assert out[0, 0].tolist() == [0, 0, 0] and out[0, 2].tolist() == lut[99].tolist()
    lo = np.array([[0.25 + 1.75 * 0.025]], dtype=np.float32)      # index 2 < floor 3 -> black; floor 0 -> lut[2]
    assert hc.render_ref(lo, lut, 0.25, 2.0, floor=3)[0, 0].tolist() == [0, 0, 0]
    assert hc.render_ref(lo, lut, 0.25, 2.0, floor=0)[0, 0].tolist() == lut[2].tolist()
