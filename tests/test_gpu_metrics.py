"""-m gpu: tm_ssim_planes / tm_avgpool2_pad and teramind_amd.metrics against the float64 restatement of the reference's
measures (metrics_cases.py, itself held to the reference by test_metrics_cases_host.py), within the bound derived there from
the kernel's own accumulation lengths.  Measured on one MI355X (profiles/metrics_ssim.txt): worst |d| / bound over this file
0.078 (ssim / cs means), 0.024 (MS-SSIM), 0.108 (PSNR)."""
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

import metrics_cases as mc
import util
from teramind_amd import _lib, formats, metrics, stitch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [mc.case_id(k, s) for k, s in mc.CASES]
WORST = {"ssim": 0.0, "ms_ssim": 0.0, "psnr": 0.0}


def note(what, d, bound):
    """Every figure is printed before it is asserted; the worst ratio is kept for profiles/metrics_ssim.txt."""
    d, bound = np.asarray(d, np.float64), np.asarray(bound, np.float64)
    r = float((np.abs(d) / bound).max())
    WORST[what] = max(WORST[what], r)
    print(f"{what}: max |d| {np.abs(d).max():.3e}, bound {bound.max():.3e}, worst ratio {r:.3f}")
    assert (np.abs(d) <= bound).all(), (what, d, bound)


@functools.lru_cache(maxsize=None)
def model(kind, shape):
    """The float64 results and bounds of one 8-bit case, computed once (not to be changed)."""
    X, Y = mc.pair(kind, shape)
    w = mc.taps()
    s, cs = mc.ssim64(X, Y, w)
    bs, bc = mc.plane_bounds(X, Y, w)
    m = {"X": X, "Y": Y, "ssim": s, "cs": cs, "b_ssim": bs, "b_cs": bc, "sq": mc.sqerr64(X, Y), "psnr": mc.psnr64(X, Y)}
    if shape == mc.MS_SHAPE:
        lv = mc.ms_levels64(X, Y, w)
        m["ms"] = mc.ms_combine64([l[1] for l in lv[:-1]], lv[-1][0])
        m["b_ms"] = mc.ms_bound(lv, w)
    for v in m.values():
        v.setflags(write=False)
    return m


def dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)


def check_psnr(got, want, kind):
    if kind == "equal":
        assert np.isposinf(got).all() and np.isposinf(want).all()
    else:
        note("psnr", got - want, mc.psnr_tol(want))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("kind,shape", mc.CASES, ids=IDS)
def test_against_the_model(kind, shape, dtype):
    m = model(kind, shape)
    X, Y = dev(m["X"], dtype), dev(m["Y"], dtype)
    count = (shape[0] - mc.WIN + 1) * (shape[1] - mc.WIN + 1)
    sums = metrics.ssim_sums(X, Y, mc.taps(), (mc.K[0] * 255.0) ** 2, (mc.K[1] * 255.0) ** 2).cpu().numpy()
    assert sums.dtype == np.float64 and sums.shape == (mc.N, mc.C, 3)
    note("ssim", sums[..., 0] / count - m["ssim"], m["b_ssim"])
    note("ssim", sums[..., 1] / count - m["cs"], m["b_cs"])
    assert np.array_equal(sums[..., 2], m["sq"])                      # exact integers
    got = metrics.ssim(X, Y, size_average=False)
    assert got.dtype == torch.float32 and got.shape == (mc.N,) and got.is_cuda
    note("ssim", got.cpu().numpy() - m["ssim"].mean(1), m["b_ssim"].mean(1) + mc.U)
    scalar = metrics.SSIM(channel=mc.C)(X, Y)
    assert scalar.shape == () and abs(scalar.item() - m["ssim"].mean()) <= m["b_ssim"].mean() + mc.U
    p = metrics.PSNR()(X, Y)
    assert p.dtype == torch.float32 and p.shape == (mc.N,)
    check_psnr(p.cpu().numpy().astype(np.float64), m["psnr"], kind)
    if shape == mc.MS_SHAPE:
        got = metrics.ms_ssim(X, Y, size_average=False)
        assert got.dtype == torch.float32 and got.shape == (mc.N,)
        note("ms_ssim", got.cpu().numpy() - m["ms"].mean(1), m["b_ms"].mean(1) + mc.U)
        if kind == "anti":
            assert (got == 0).all()
        gray = metrics.MS_SSIM(channel=mc.C)(X[:, 0], Y[:, 0])       # 3-D input: the one-channel window
        assert abs(gray.item() - m["ms"][:, 0].mean()) <= m["b_ms"][:, 0].mean() + mc.U


@pytest.mark.parametrize("shape", [(12, 37), mc.TILE_PLUS_ONE], ids=["12x37", "tile+1"])
@pytest.mark.parametrize("kind", mc.KINDS)
def test_unit_range_float32(kind, shape):
    """float32 planes in [-1, 1] with data_range 2; the model reads the same float32 values."""
    Xu, Yu = mc.pair(kind, shape)
    Xf, Yf = mc.unit_range(Xu), mc.unit_range(Yu)
    w = mc.taps()
    s, cs = mc.ssim64(Xf, Yf, w, data_range=2.0)
    bs, bc = mc.plane_bounds(Xf, Yf, w, data_range=2.0)
    X, Y = dev(Xf, torch.float32), dev(Yf, torch.float32)
    count = (shape[0] - mc.WIN + 1) * (shape[1] - mc.WIN + 1)
    sums = metrics.ssim_sums(X, Y, w, (mc.K[0] * 2.0) ** 2, (mc.K[1] * 2.0) ** 2).cpu().numpy()
    note("ssim", sums[..., 0] / count - s, bs)
    note("ssim", sums[..., 1] / count - cs, bc)
    sq = mc.sqerr64(Xf, Yf)
    assert (np.abs(sums[..., 2] - sq) <= 1e-12 * sq).all()
    note("ssim", metrics.ssim(X, Y, data_range=2, size_average=False).cpu().numpy() - s.mean(1), bs.mean(1) + mc.U)
    check_psnr(metrics.PSNR(mval=2.0)(X, Y).cpu().numpy().astype(np.float64), mc.psnr64(Xf, Yf, 2.0), kind)


@pytest.mark.parametrize("n", [3, 9, 13, 33])
def test_other_window_lengths(n):
    """Every window but the 11-tap one takes the loops with run-time trip counts; 33 taps is the largest LDS plan."""
    shape = (mc.TH + 33, mc.TW + 33)
    X, Y = mc.pair("smooth", shape)
    w = mc.taps(n, 0.3 * ((n - 1) * 0.5 - 1) + 0.8)
    C1, C2 = (mc.K[0] * 255.0) ** 2, (mc.K[1] * 255.0) ** 2
    s, cs = mc.ssim64(X, Y, w)
    b = np.array([[mc.bound(X[i, j], Y[i, j], w, C1, C2) for j in range(mc.C)] for i in range(mc.N)])
    count = (shape[0] - n + 1) * (shape[1] - n + 1)
    for dtype in (torch.uint8, torch.float32):
        sums = metrics.ssim_sums(dev(X, dtype), dev(Y, dtype), w, C1, C2).cpu().numpy()
        note("ssim", sums[..., 0] / count - s, b[..., 0])
        note("ssim", sums[..., 1] / count - cs, b[..., 1])
        assert np.array_equal(sums[..., 2], mc.sqerr64(X, Y))
    win = torch.from_numpy(w).reshape(1, 1, 1, n).repeat(mc.C, 1, 1, 1)
    got = metrics.ssim(dev(X, torch.uint8), dev(Y, torch.uint8), win=win, size_average=False)
    note("ssim", got.cpu().numpy() - s.mean(1), b[..., 0].mean(1) + mc.U)


def framed(a, fill, dtype):
    """`a` [N, C, H, W] inside a larger filled buffer: a channel slice, a pitch above W, an odd element offset."""
    n, c, h, w = a.shape
    big = torch.empty((n, c + 2, h + 5, w + 14), dtype=dtype, device=DEV)
    if dtype == torch.uint8:
        big.fill_(fill)
    else:
        big.fill_(float("nan"))
    col = 3 if ((h + 5) * (w + 14) + 2 * (w + 14)) % 2 == 0 else 2
    view = big[:, 1:1 + c, 2:2 + h, col:col + w]
    view.copy_(dev(a, dtype))
    assert view.storage_offset() % 2 == 1 and view.stride(2) > w and view.stride(0) != c * view.stride(1)
    return view


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_addressing_and_determinism(dtype):
    m = model("smooth", mc.MS_SHAPE)
    w, C1, C2 = mc.taps(), 6.5025, 58.5225
    X, Y = dev(m["X"], dtype), dev(m["Y"], dtype)
    Xv, Yv = framed(m["X"], 0xA5, dtype), framed(m["Y"], 0xA5, dtype)
    a, b = metrics.ssim_sums(X, Y, w, C1, C2), metrics.ssim_sums(Xv, Yv, w, C1, C2)
    assert torch.equal(a, b) and torch.isfinite(b).all()
    assert torch.equal(a, metrics.ssim_sums(X, Y, w, C1, C2))                     # two calls, equal bits
    assert torch.equal(a, metrics.ssim_sums(X, Yv, w, C1, C2))                    # operands pitched independently
    assert torch.equal(metrics.avgpool2_pad(X), metrics.avgpool2_pad(Xv))
    assert torch.equal(metrics.ms_ssim(X, Y, size_average=False), metrics.ms_ssim(Xv, Yv, size_average=False))
    assert torch.equal(metrics.ms_ssim(X, Y, size_average=False), metrics.ms_ssim(X, Y, size_average=False))
    # one image, one channel of the frame: a single call with its own plane stride
    assert torch.equal(metrics.ssim_sums(Xv[1:, :1], Yv[1:, :1], w, C1, C2), a[1:, :1])


def test_five_d_input_below_the_window_depth():
    m = model("near", mc.TILE_PLUS_ONE)
    X, Y = dev(m["X"], torch.uint8), dev(m["Y"], torch.uint8)          # [N, C, H, W] read as [1, N, C, H, W]: depth C
    got = metrics.ssim(X[None], Y[None], size_average=False)
    assert got.shape == (1,)
    note("ssim", got.cpu().numpy() - m["ssim"].mean(), m["b_ssim"].mean() + mc.U)


def test_pooling_levels_equal_torch_on_the_cpu():
    X, _ = mc.pair("noise", mc.MS_SHAPE)
    t, g = torch.from_numpy(X.astype(np.float32)), dev(X, torch.uint8)
    gf = dev(X, torch.float32)
    for lvl in range(4):
        t = F.avg_pool2d(t, kernel_size=2, padding=[s % 2 for s in t.shape[2:]])
        g, gf = metrics.avgpool2_pad(g), metrics.avgpool2_pad(gf)
        assert g.dtype == torch.float32 and g.shape == t.shape
        assert torch.equal(g.cpu(), t) and torch.equal(gf.cpu(), t), lvl
    assert tuple(t.shape[2:]) == (11, 11)


def test_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    x = torch.zeros(64, 64, dtype=torch.uint8, device=DEV)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    pooled = torch.full((32, 32), float("nan"), dtype=torch.float32, device=DEV)
    w = (C.c_float * 34)(*([1.0 / 11] * 34))
    p, o, st = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), _lib.current_stream_ptr()

    def ssim_rc(xp=p, yp=p, dtype=0, P=1, H=64, W=64, pitch=64, win=w, n=11, outp=o):
        rc = L.tm_ssim_planes(xp, yp, dtype, P, H, W, pitch, 4096, pitch, 4096, win, n, 6.5, 58.5, outp, st)
        return rc, L.tm_last_error()

    for kw, text in ((dict(H=10), b"below the window"), (dict(W=10), b"below the window"), (dict(n=10), b"taps"),
                     (dict(n=35), b"taps"), (dict(n=1), b"taps"), (dict(dtype=2), b"dtype"), (dict(xp=None), b"null"),
                     (dict(yp=None), b"null"), (dict(win=None), b"null"), (dict(pitch=63), b"pitch"),
                     (dict(dtype=1, pitch=64), b"pitch"), (dict(P=0), b"P =")):
        rc, msg = ssim_rc(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert ssim_rc(outp=None)[0] == -1
    pp = C.c_void_p(pooled.data_ptr())
    for args, text in (((None, 0, 1, 64, 64, 64, 4096, pp, 128, 4096), b"null"), ((p, 5, 1, 64, 64, 64, 4096, pp, 128, 4096), b"dtype"),
                       ((p, 0, 1, 64, 64, 63, 4096, pp, 128, 4096), b"pitch"), ((p, 0, 1, 64, 64, 64, 4096, pp, 124, 4096), b"pitch"),
                       ((p, 0, 1, 0, 64, 64, 4096, pp, 128, 4096), b"positive")):
        assert L.tm_avgpool2_pad(*args, st) == -1 and text in L.tm_last_error(), args
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(pooled).all()
    with pytest.raises(NotImplementedError, match="below the window"):
        metrics.ssim(x[None, None, :8], x[None, None, :8])


@pytest.fixture(scope="module")
def roi(tmp_path_factory):
    """A generated step directory and a real-tile directory of 2 x 2 tiles, 2 stains x 2 slices: 4 planes of 512 x 512."""
    root = tmp_path_factory.mktemp("roi")
    gdir, rdir = root / "gen", root / "real"
    gdir.mkdir()
    rdir.mkdir()
    rng = np.random.default_rng(11)
    hst, wst, slc, cst = 20480, 40960, 2, 2
    yy, xx = np.meshgrid(np.arange(768), np.arange(768), indexing="ij")
    field = np.stack([127.5 + 90 * np.sin(xx / (23.0 + 5 * k)) * np.cos(yy / (31.0 - 4 * k)) for k in range(cst * slc)])
    real = np.clip(np.rint(field + rng.normal(0, 4, field.shape)), 0, 255)              # [(c s), 768, 768], origin (hst-128, wst-128)
    gen = np.clip(real + rng.normal(0, 9, real.shape), 0, 255) / 127.5 - 1
    for ph in range(2):
        for pw in range(2):
            r0, c0 = hst + 256 * ph, wst + 256 * pw
            formats.write_zarr_zip(rdir / f"{r0}_{r0 + 256}_{c0}_{c0 + 256}_{r0 - 128}_{r0 + 384}_{c0 - 128}_{c0 + 384}.zip",
                                   real[:, 256 * ph:256 * ph + 512, 256 * pw:256 * pw + 512].astype(np.uint8))
            formats.write_state_tile(gdir / f"{r0}_{r0 + 256}_{c0}_{c0 + 256}.zip",
                                     gen[:, 128 + 256 * ph:384 + 256 * ph, 128 + 256 * pw:384 + 256 * pw])
    g = stitch.stitch_dir(gdir, hst, wst, 2, 2, slc=slc)
    r = stitch.stitch_real_dir(rdir, hst, wst, 2, 2, slc=slc)
    assert g.shape == r.shape == (4, 512, 512) and r.dtype == np.uint8
    assert np.array_equal(r[1], real[1 * slc + 0, 128:640, 128:640].astype(np.uint8))   # '(s c)' plane 1 = stain 1 of slice 0
    g.setflags(write=False)
    r.setflags(write=False)
    w = mc.taps()
    want = {"psnr": mc.psnr64(g[:, None], r[:, None]), "ssim": mc.ssim64(g[:, None], r[:, None], w)[0][:, 0],
            "b_ssim": mc.plane_bounds(g[:, None], r[:, None], w)[0][:, 0]}
    lv = mc.ms_levels64(g[:, None], r[:, None], w)
    want["ms_ssim"], want["b_ms"] = mc.ms_combine64([l[1] for l in lv[:-1]], lv[-1][0])[:, 0], mc.ms_bound(lv, w)[:, 0]
    return dict(gdir=gdir, rdir=rdir, gen=g, real=r, want=want, args=(hst, wst, 2, 2), slc=slc, root=root)


def check_rows(rows, want):
    note("ssim", np.array(rows["ssim"]) - want["ssim"], want["b_ssim"] + mc.U)
    note("ms_ssim", np.array(rows["ms_ssim"]) - want["ms_ssim"], want["b_ms"] + mc.U)
    note("psnr", np.array(rows["psnr"]) - want["psnr"], mc.psnr_tol(want["psnr"]))


def test_compare_mosaics(roi):
    rows = metrics.compare_mosaics(roi["gen"], roi["real"])
    assert sorted(rows) == ["ms_ssim", "psnr", "ssim"] and all(len(v) == 4 for v in rows.values())
    assert 0 < min(rows["ssim"]) and max(rows["ssim"]) < 1 and 20 < min(rows["psnr"]) < 40              # a meaningful pair
    check_rows(rows, roi["want"])
    assert metrics.compare_mosaics(torch.from_numpy(np.array(roi["gen"])).to(DEV), roi["real"]) == rows
    assert sorted(metrics.compare_mosaics(roi["gen"], roi["real"], ms=False)) == ["psnr", "ssim"]
    small = metrics.compare_mosaics(roi["gen"][:, :160, :160], roi["real"][:, :160, :160])
    assert sorted(small) == ["psnr", "ssim"]                         # too small for the four downsamplings


def test_eval_roi_tool(roi):
    hst, wst, hnm, wnm = roi["args"]
    out = roi["root"] / "report.json"
    cmd = [sys.executable, os.path.join(util.ROOT, "tools", "eval_roi.py"), "--gen_dir", str(roi["gdir"]), "--real_dir", str(roi["rdir"]),
           "--hst", str(hst), "--wst", str(wst), "--hnm", str(hnm), "--wnm", str(wnm), "--slc", str(roi["slc"]), "--out", str(out)]
    subprocess.run(cmd, check=True, timeout=300)
    rep = json.load(open(out))
    assert [(r["plane"], r["slice"], r["stain"]) for r in rep["planes"]] == [(0, 0, 0), (1, 0, 1), (2, 1, 0), (3, 1, 1)]
    rows = {k: [r[k] for r in rep["planes"]] for k in ("psnr", "ssim", "ms_ssim")}
    check_rows(rows, roi["want"])
    assert rows == metrics.compare_mosaics(roi["gen"], roi["real"])
    for c, m in enumerate(rep["mean_per_stain"]):
        assert m["stain"] == c and m["planes"] == 2
        for k in rows:
            assert m[k] == pytest.approx(np.mean([rows[k][c], rows[k][2 + c]]), rel=1e-12)
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import eval_roi
    one = eval_roi.evaluate(roi["gdir"], roi["rdir"], hst, wst, hnm, wnm, slc=roi["slc"], slices=[2])
    assert len(one["planes"]) == 1 and one["planes"][0] == rep["planes"][2]


def test_worst_ratio_is_written(out_dir):
    """Runs last in this file: the worst |d| / bound seen above, for profiles/metrics_ssim.txt."""
    with open(os.path.join(out_dir, "metrics_worst_ratio.json"), "w") as f:
        json.dump(WORST, f)
    print("worst |d| / bound:", WORST)
    assert all(v <= 1.0 for v in WORST.values())
