"""-m gpu: tm_ssim_volumes / tm_avgpool2_pad3 and the 5-D surface of teramind_amd.metrics against the float64 restatement of the
reference's measures (metrics3d_cases.py, itself held to the reference by test_metrics3d_cases_host.py), within the bound
derived there from the kernel's own accumulation lengths.  Every test that feeds a 5-D input as deep as the window raised
NotImplementedError before the 3-D window existed.  The worst |d| / bound per measure is written to metrics3d_worst_ratio.json
in the session's output directory (profiles/metrics_ssim3d.txt quotes it)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics3d_cases as m3
import util
from teramind_amd import _lib, formats, metrics, stitch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [m3.case_id(k, s) for k, s in m3.CASES]
MS_IDS = [m3.case_id(k, s) for k, s in m3.MS_CASES]
C1, C2 = (m3.K[0] * 255.0) ** 2, (m3.K[1] * 255.0) ** 2
WORST = {"ssim": 0.0, "ms_ssim": 0.0, "psnr": 0.0}


def note(what, d, bound):
    """Every figure is printed before it is asserted; the worst ratio is kept for profiles/metrics_ssim3d.txt."""
    d, bound = np.asarray(d, np.float64), np.asarray(bound, np.float64)
    r = float((np.abs(d) / bound).max())
    WORST[what] = max(WORST[what], r)
    print(f"{what}: max |d| {np.abs(d).max():.3e}, bound {bound.max():.3e}, worst ratio {r:.3f}")
    assert (np.abs(d) <= bound).all(), (what, d, bound)


def frozen(m):
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def model(kind, shape):
    """The float64 results and bounds of one 8-bit case, computed once (not to be changed)."""
    X, Y = m3.pair(kind, shape)
    w = m3.taps()
    s, cs = m3.ssim64(X, Y, w)
    bs, bc = m3.volume_bounds(X, Y, w)
    return frozen({"X": X, "Y": Y, "ssim": s, "cs": cs, "b_ssim": bs, "b_cs": bc, "sq": m3.sqerr64(X, Y)})


@functools.lru_cache(maxsize=None)
def ms_model(kind, shape):
    X, Y = m3.pair(kind, shape, n=1)
    w = m3.taps()
    lv = m3.ms_levels64(X, Y, w)
    return frozen({"X": X, "Y": Y, "ms": m3.mc.ms_combine64([l[1] for l in lv[:-1]], lv[-1][0]), "b_ms": m3.ms_bound(lv, w),
                   "ssim": lv[0][0], "b_ssim": m3.volume_bounds(X, Y, w)[0]})


def dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)


def count_of(shape, n=m3.WIN):
    return int(np.prod([d - n + 1 for d in shape]))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("kind,shape", m3.CASES, ids=IDS)
def test_against_the_model(kind, shape, dtype):
    m = model(kind, shape)
    X, Y = dev(m["X"], dtype), dev(m["Y"], dtype)
    sums = metrics.ssim_sums3(X, Y, m3.taps(), C1, C2).cpu().numpy()
    assert sums.dtype == np.float64 and sums.shape == (m3.N, m3.C, 3)
    note("ssim", sums[..., 0] / count_of(shape) - m["ssim"], m["b_ssim"])
    note("ssim", sums[..., 1] / count_of(shape) - m["cs"], m["b_cs"])
    assert np.array_equal(sums[..., 2], m["sq"])                      # exact integers
    got = metrics.ssim(X, Y, size_average=False)
    assert got.dtype == torch.float32 and got.shape == (m3.N,) and got.is_cuda
    note("ssim", got.cpu().numpy() - m["ssim"].mean(1), m["b_ssim"].mean(1) + m3.U)
    scalar = metrics.SSIM(channel=m3.C, spatial_dims=3)(X, Y)
    assert scalar.shape == () and abs(scalar.item() - m["ssim"].mean()) <= m["b_ssim"].mean() + m3.U


def test_unit_range_float32():
    """One kind as float32 volumes in [-1, 1] with data_range 2; the model reads the same float32 values."""
    shape = (12, 12, 37)
    Xu, Yu = m3.pair("smooth", shape)
    Xf, Yf = m3.mc.unit_range(Xu), m3.mc.unit_range(Yu)
    w = m3.taps()
    s, cs = m3.ssim64(Xf, Yf, w, data_range=2.0)
    bs, bc = m3.volume_bounds(Xf, Yf, w, data_range=2.0)
    X, Y = dev(Xf, torch.float32), dev(Yf, torch.float32)
    sums = metrics.ssim_sums3(X, Y, w, (m3.K[0] * 2.0) ** 2, (m3.K[1] * 2.0) ** 2).cpu().numpy()
    note("ssim", sums[..., 0] / count_of(shape) - s, bs)
    note("ssim", sums[..., 1] / count_of(shape) - cs, bc)
    sq = m3.sqerr64(Xf, Yf)
    assert (np.abs(sums[..., 2] - sq) <= 1e-12 * sq).all()
    note("ssim", metrics.ssim(X, Y, data_range=2, size_average=False).cpu().numpy() - s.mean(1), bs.mean(1) + m3.U)


@pytest.mark.parametrize("n", [3, 5, 9])
def test_shorter_windows(n):
    """The same code over zero-padded taps; the valid region is that of the real n."""
    shape = m3.TILE_PLUS_ONE
    X, Y = m3.pair("smooth", shape)
    w = m3.taps(n, 0.3 * ((n - 1) * 0.5 - 1) + 0.8)
    s, cs = m3.ssim64(X, Y, w)
    bs, bc = m3.volume_bounds(X, Y, w)
    for dtype in (torch.uint8, torch.float32):
        sums = metrics.ssim_sums3(dev(X, dtype), dev(Y, dtype), w, C1, C2).cpu().numpy()
        note("ssim", sums[..., 0] / count_of(shape, n) - s, bs)
        note("ssim", sums[..., 1] / count_of(shape, n) - cs, bc)
        assert np.array_equal(sums[..., 2], m3.sqerr64(X, Y))
    win = torch.from_numpy(w).reshape(1, 1, 1, 1, n).repeat(m3.C, 1, 1, 1, 1)
    got = metrics.ssim(dev(X, torch.uint8), dev(Y, torch.uint8), win=win, size_average=False)
    note("ssim", got.cpu().numpy() - s.mean(1), bs.mean(1) + m3.U)


def test_longer_windows_are_refused():
    X = torch.zeros(1, 1, 13, 16, 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(NotImplementedError, match="at most 11"):
        metrics.ssim(X, X, win_size=13)


def framed(a, fill, dtype):
    """`a` [N, C, D, H, W] inside a larger filled buffer: a channel slice, a depth slice, a pitch above W, an odd offset."""
    n, c, d, h, w = a.shape
    big = torch.empty((n, c + 1, d + 2, h + 3, w + 7), dtype=dtype, device=DEV)
    if dtype == torch.uint8:
        big.fill_(fill)
    else:
        big.fill_(float("nan"))
    view = big[:, 1:1 + c, 1:1 + d, 2:2 + h, 3:3 + w]
    view.copy_(dev(a, dtype))
    assert view.stride(3) > w and view.stride(2) > h * view.stride(3) and view.stride(0) != c * view.stride(1)
    return view


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_addressing_and_determinism(dtype):
    m = model("smooth", m3.TILE_PLUS_ONE)
    w = m3.taps()
    X, Y = dev(m["X"], dtype), dev(m["Y"], dtype)
    a = metrics.ssim_sums3(X, Y, w, C1, C2)
    assert torch.equal(a, metrics.ssim_sums3(X, Y, w, C1, C2))                     # two calls, equal bits
    Xv, Yv = framed(m["X"], 0xA5, dtype), framed(m["Y"], 0xA5, dtype)
    b = metrics.ssim_sums3(Xv, Yv, w, C1, C2)
    assert torch.equal(a, b) and torch.isfinite(b).all()
    assert torch.equal(a, metrics.ssim_sums3(X, Yv, w, C1, C2))                    # operands strided independently
    assert torch.equal(metrics.avgpool2_pad3(X), metrics.avgpool2_pad3(Xv))
    # the '(s c)' mosaic of image 0: stain c is every C-th plane from c, read through its depth stride
    gm, rm = dev(m3.interleave(list(m["X"][0])), dtype), dev(m3.interleave(list(m["Y"][0])), dtype)
    for c in range(m3.C):
        gv, rv = gm[c::m3.C][None, None], rm[c::m3.C][None, None]
        assert gv.stride(2) == m3.C * gv.shape[3] * gv.shape[4] and gv.data_ptr() == gm[c].data_ptr()
        assert torch.equal(metrics.ssim_sums3(gv, rv, w, C1, C2)[0, 0], a[0, c])
        assert torch.equal(metrics.avgpool2_pad3(gv)[0, 0], metrics.avgpool2_pad3(X)[0, c])
    assert torch.equal(metrics.ssim(X, Y, size_average=False), metrics.ssim(Xv, Yv, size_average=False))


@pytest.mark.parametrize("kind,shape", m3.MS_CASES, ids=MS_IDS)
def test_ms_ssim(kind, shape):
    m = ms_model(kind, shape)
    for dtype in (torch.uint8, torch.float32):
        X, Y = dev(m["X"], dtype), dev(m["Y"], dtype)
        got = metrics.ms_ssim(X, Y, size_average=False)
        assert got.dtype == torch.float32 and got.shape == (1,) and got.is_cuda
        note("ms_ssim", got.cpu().numpy() - m["ms"].mean(1), m["b_ms"].mean(1) + m3.U)
        assert torch.equal(got, metrics.ms_ssim(X, Y, size_average=False))
    module = metrics.MS_SSIM(channel=m3.C, spatial_dims=3)(X, Y)
    assert module.shape == () and abs(module.item() - m["ms"].mean()) <= m["b_ms"].mean() + m3.U
    note("ssim", metrics.ssim(X, Y, size_average=False).cpu().numpy() - m["ssim"].mean(1), m["b_ssim"].mean(1) + m3.U)


def test_pooling_levels_equal_torch_on_the_cpu():
    X, _ = m3.pair("noise", (50, 176, 163), n=1)
    t, g, gf = torch.from_numpy(X.astype(np.float32)), dev(X, torch.uint8), dev(X, torch.float32)
    for lvl in range(4):
        t = F.avg_pool3d(t, kernel_size=2, padding=[s % 2 for s in t.shape[2:]])
        g, gf = metrics.avgpool2_pad3(g), metrics.avgpool2_pad3(gf)
        assert g.dtype == torch.float32 and g.shape == t.shape
        assert torch.equal(g.cpu(), t) and torch.equal(gf.cpu(), t), lvl
    assert tuple(t.shape[2:]) == (4, 11, 11)
    one = X[:, :, 7:8, :21]                                           # D = 1 pools to 1 (the pad plane counted): the model's word
    want = torch.from_numpy(m3.pool64(one).astype(np.float32))
    assert torch.equal(metrics.avgpool2_pad3(dev(one, torch.uint8)).cpu(), want) and want.shape[2:] == (1, 11, 82)


def test_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    x = torch.zeros(16, 64, 64, dtype=torch.uint8, device=DEV)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    pooled = torch.full((8, 32, 32), float("nan"), dtype=torch.float32, device=DEV)
    w = (C.c_float * 16)(*([1.0 / 11] * 16))
    p, o, st = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), _lib.current_stream_ptr()

    def rc_of(xp=p, yp=p, dtype=0, V=1, D=16, H=64, W=64, pitch=64, depth=4096, win=w, n=11, outp=o):
        rc = L.tm_ssim_volumes(xp, yp, dtype, V, D, H, W, pitch, depth, 65536, pitch, depth, 65536, win, n, 6.5, 58.5, outp, st)
        return rc, L.tm_last_error()

    for kw, text in ((dict(D=10), b"below the window"), (dict(H=10), b"below the window"), (dict(W=10), b"below the window"),
                     (dict(n=10), b"taps"), (dict(n=13), b"registers"), (dict(n=1), b"taps"), (dict(dtype=2), b"dtype"),
                     (dict(xp=None), b"null"), (dict(yp=None), b"null"), (dict(win=None), b"null"), (dict(pitch=63), b"pitch"),
                     (dict(depth=4095), b"depth stride"), (dict(dtype=1, pitch=64), b"pitch"), (dict(V=0), b"V =")):
        rc, msg = rc_of(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert rc_of(outp=None)[0] == -1
    pp = C.c_void_p(pooled.data_ptr())
    good = [p, 0, 1, 16, 64, 64, 64, 4096, 65536, pp, 128, 4096, 32768]
    for i, val, text in ((0, None, b"null"), (9, None, b"null"), (1, 5, b"dtype"), (6, 63, b"pitch"), (7, 4095, b"depth stride"),
                         (10, 124, b"pitch"), (11, 4092, b"depth stride"), (3, 0, b"positive")):
        args = list(good)
        args[i] = val
        assert L.tm_avgpool2_pad3(*args, st) == -1 and text in L.tm_last_error(), (i, val)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pooled).all()
    with pytest.raises(NotImplementedError, match="below the window"):           # H below the window: still no route
        metrics.ssim(x[None, None, :, :8], x[None, None, :, :8])
    with pytest.raises(NotImplementedError, match="below the window"):
        metrics.ssim(x[None, None, :4, :8], x[None, None, :4, :8])


SLC, CST = 11, 2


@pytest.fixture(scope="module")
def roi(tmp_path_factory):
    """A generated step directory and a real-tile directory of 2 x 2 tiles, 2 stains x 11 slices: 22 planes of 512 x 512, the
    generated slices 4 and 5 of stain 1 swapped (a fault no per-plane measure of the stack's mean shows)."""
    root = tmp_path_factory.mktemp("roi3d")
    gdir, rdir = root / "gen", root / "real"
    gdir.mkdir()
    rdir.mkdir()
    rng = np.random.default_rng(13)
    hst, wst = 20480, 40960
    yy, xx = np.meshgrid(np.arange(768), np.arange(768), indexing="ij")
    field = np.stack([127.5 + 90 * np.sin(xx / (23.0 + 5 * c) + 0.4 * s) * np.cos(yy / (31.0 - 4 * c) - 0.3 * s)
                      for c in range(CST) for s in range(SLC)])                          # [(c s), 768, 768]
    real = np.clip(np.rint(field + rng.normal(0, 4, field.shape)), 0, 255)
    gen = np.clip(real + rng.normal(0, 9, real.shape), 0, 255) / 127.5 - 1
    gen[[SLC + 4, SLC + 5]] = gen[[SLC + 5, SLC + 4]]
    for ph in range(2):
        for pw in range(2):
            r0, c0 = hst + 256 * ph, wst + 256 * pw
            formats.write_zarr_zip(rdir / f"{r0}_{r0 + 256}_{c0}_{c0 + 256}_{r0 - 128}_{r0 + 384}_{c0 - 128}_{c0 + 384}.zip",
                                   real[:, 256 * ph:256 * ph + 512, 256 * pw:256 * pw + 512].astype(np.uint8))
            formats.write_state_tile(gdir / f"{r0}_{r0 + 256}_{c0}_{c0 + 256}.zip",
                                     gen[:, 128 + 256 * ph:384 + 256 * ph, 128 + 256 * pw:384 + 256 * pw])
    g = stitch.stitch_dir(gdir, hst, wst, 2, 2, slc=SLC)
    r = stitch.stitch_real_dir(rdir, hst, wst, 2, 2, slc=SLC)
    assert g.shape == r.shape == (SLC * CST, 512, 512) and r.dtype == np.uint8
    g.setflags(write=False)
    r.setflags(write=False)
    return dict(gdir=gdir, rdir=rdir, gen=g, real=r, args=(hst, wst, 2, 2), root=root)


def volumes_of(mosaic):
    """[1, C, D, H, W] from the '(s c)' mosaic: the stains as channels."""
    return np.ascontiguousarray(mosaic.reshape(SLC, CST, *mosaic.shape[1:]).transpose(1, 0, 2, 3))[None]


def want_rows(gen, real):
    """The model's word on the stains of two mosaics: (psnr, ssim, ssim bound, ms, ms bound), [C] each."""
    w = m3.taps()
    G, R = volumes_of(gen), volumes_of(real)
    lv = m3.ms_levels64(G, R, w)
    return dict(psnr=m3.psnr64(G, R)[0], ssim=lv[0][0][0], b_ssim=m3.volume_bounds(G, R, w)[0][0],
                ms=m3.mc.ms_combine64([l[1] for l in lv[:-1]], lv[-1][0])[0], b_ms=m3.ms_bound(lv, w)[0])


def check_volume_rows(rows, want, ms=True):
    note("ssim", np.array(rows["ssim3d"]) - want["ssim"], want["b_ssim"] + m3.U)
    note("psnr", np.array(rows["psnr3d"]) - want["psnr"], m3.psnr_tol(want["psnr"]))
    if ms:
        note("ms_ssim", np.array(rows["ms_ssim3d"]) - want["ms"], want["b_ms"] + m3.U)


def test_compare_volumes(roi):
    g, r = roi["gen"][:, :176, :163], roi["real"][:, :176, :163]               # the smallest planes that still fit MS-SSIM
    rows = metrics.compare_volumes(g, r)
    assert sorted(rows) == ["ms_ssim3d", "psnr3d", "ssim3d"] and all(len(v) == CST and isinstance(v[0], float) for v in rows.values())
    assert 0 < min(rows["ssim3d"]) and max(rows["ssim3d"]) < 1 and 20 < min(rows["psnr3d"]) < 40      # a meaningful pair
    check_volume_rows(rows, want_rows(g, r))
    assert rows["ssim3d"][1] < rows["ssim3d"][0] - 0.01                         # the swapped slices of stain 1 show
    assert metrics.compare_volumes(torch.from_numpy(np.array(g)).to(DEV), r) == rows
    assert sorted(metrics.compare_volumes(g, r, ms=False)) == ["psnr3d", "ssim3d"]
    assert sorted(metrics.compare_volumes(g[:, :160], r[:, :160])) == ["psnr3d", "ssim3d"]   # too small for the downsamplings
    three = metrics.compare_volumes(np.concatenate([g, g[:11]]), np.concatenate([r, r[:11]]), n_stain=3, ms=False)
    assert len(three["ssim3d"]) == 3


def test_eval_roi_tool_with_volumes(roi):
    hst, wst, hnm, wnm = roi["args"]
    base = [sys.executable, os.path.join(util.ROOT, "tools", "eval_roi.py"), "--gen_dir", str(roi["gdir"]), "--real_dir", str(roi["rdir"]),
            "--hst", str(hst), "--wst", str(wst), "--hnm", str(hnm), "--wnm", str(wnm), "--slc", str(SLC)]
    vol = roi["root"] / "volume.json"
    subprocess.run(base + ["--volume", "--out", str(vol)], check=True, timeout=300)            # MS-SSIM on
    repv = json.load(open(vol))
    # without the flag (whose command line test_gpu_metrics.py runs): the report of before, key for key, and nothing else
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import eval_roi
    rep = eval_roi.evaluate(roi["gdir"], roi["rdir"], hst, wst, hnm, wnm, slc=SLC)
    assert list(rep) == ["gen_dir", "real_dir", "roi", "shape", "measures", "planes", "mean_per_stain"]
    assert list(repv) == list(rep) + ["volumes"]
    assert json.dumps({k: repv[k] for k in rep}, indent=1) == json.dumps(rep, indent=1)
    assert [(v["stain"], v["slices"]) for v in repv["volumes"]] == [(0, SLC), (1, SLC)]
    assert all(list(v) == ["stain", "slices", "psnr3d", "ssim3d", "ms_ssim3d"] for v in repv["volumes"])
    rows = {k: [v[k] for v in repv["volumes"]] for k in ("psnr3d", "ssim3d", "ms_ssim3d")}
    # the tool's three measures are compare_volumes' on the whole mosaics, bit for bit (that function is held to the model
    # with MS-SSIM on the 176 x 163 crop above); PSNR and SSIM of the 512 x 512 stacks are held to the model here as well
    assert rows == metrics.compare_volumes(roi["gen"], roi["real"])
    assert 0 < min(rows["ms_ssim3d"]) and max(rows["ms_ssim3d"]) < 1 and rows["ms_ssim3d"][1] < rows["ms_ssim3d"][0]
    G, R = volumes_of(roi["gen"]), volumes_of(roi["real"])
    w = m3.taps()
    check_volume_rows(rows, dict(psnr=m3.psnr64(G, R)[0], ssim=m3.ssim64(G, R, w)[0][0], b_ssim=m3.volume_bounds(G, R, w)[0][0]),
                      ms=False)
    with pytest.raises(ValueError, match="--slices"):
        eval_roi.evaluate(roi["gdir"], roi["rdir"], hst, wst, hnm, wnm, slc=SLC, slices=[0, 1], volume=True)
    refused = subprocess.run(base + ["--volume", "--slices", "0", "1", "--out", str(vol)], capture_output=True, timeout=300)
    assert refused.returncode == 2 and b"--slices" in refused.stderr


def test_worst_ratio_is_written(out_dir):
    """Runs last in this file: the worst |d| / bound seen above, for profiles/metrics_ssim3d.txt."""
    with open(os.path.join(out_dir, "metrics3d_worst_ratio.json"), "w") as f:
        json.dump(WORST, f)
    print("worst |d| / bound:", WORST)
    assert all(v <= 1.0 for v in WORST.values())
