"""-m gpu: the conv weight gradient on the fp32 matrix pipe (tm_op_conv_wgrad_dev -> conv_wgrad_mfma_kernel, csrc/tm_train.hip),
held to float64 references of its definition.  Rules as in test_gpu_train_ops.py: integer cases are exact (torch.equal against
float64), float cases get a bound derived from the kernel's own accumulation order, outputs start as NaN, and two runs must agree
in every bit (partials are added in chunk order, no float atomics)."""
import ctypes as C

import pytest
import torch

import train_op_ref as R
import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = R.U


def _st():
    return _lib.current_stream_ptr()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _call(xc, yc, dw, db, accumulate, N, Cin, Cout, Z, S, ksize):
    _lib.check(_lib.lib().tm_op_conv_wgrad_dev(_lib.ptr(xc), _lib.ptr(yc), _lib.ptr(dw), _lib.ptr(db), accumulate, N, Cin, Cout, Z, S, ksize,
                                               _st()), "tm_op_conv_wgrad_dev")


def _wgrad(x, dy, ksize, with_db):
    """Two calls on NaN-prefilled device outputs (accumulate 0): every element written, the same bits twice."""
    N, Cin, Z, S, _ = x.shape
    Cout = dy.shape[1]
    xc, yc = util.to_cb8(x.to(DEV)), util.to_cb8(dy.to(DEV))
    taps = 27 if ksize == 3 else 1
    outs = []
    for _ in range(2):
        dw = torch.full((Cout, Cin, taps), NAN, device=DEV)
        db = torch.full((Cout,), NAN, device=DEV) if with_db else None
        _call(xc, yc, dw, db, 0, N, Cin, Cout, Z, S, ksize)
        outs.append((dw, db))
    torch.cuda.synchronize()
    (dw, db), (dw2, db2) = outs
    assert _same_bits(dw, dw2) and (db is None or _same_bits(db, db2)), "wgrad not reproducible"
    assert not torch.isnan(dw).any(), f"dw: {int(torch.isnan(dw).sum())} elements not written"
    return dw.cpu(), None if db is None else db.cpu()


def _wgrad_ref(x, dy, ksize):
    k, pad = (3, 1) if ksize == 3 else (1, 0)
    dw = torch.nn.grad.conv3d_weight(x, (dy.shape[1], x.shape[1], k, k, k), dy, padding=pad)
    return dw.reshape(dy.shape[1], x.shape[1], -1), dy.sum((0, 2, 3, 4))


def _wgrad_ref_mm(x, dy):
    """The same 3x3x3 definition, tap by tap as [Cout, K] @ [K, Cin] float64 products (the wide cases, where conv3d_weight is slow)."""
    N, Cin, Z, S, _ = x.shape
    Cout = dy.shape[1]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1))
    dyf = dy.permute(1, 0, 2, 3, 4).reshape(Cout, -1)
    out = torch.empty((Cout, Cin, 27), dtype=torch.float64)
    for t in range(27):
        kz, ky, kx = t // 9, (t // 3) % 3, t % 3
        xs = xp[:, :, kz:kz + Z, ky:ky + S, kx:kx + S].permute(1, 0, 2, 3, 4).reshape(Cin, -1)
        out[:, :, t] = dyf @ xs.T
    return out


def _equal(name, got, ref):
    got = torch.as_tensor(got).double().cpu()
    assert torch.equal(got, ref), util.report(name, got, ref)


# the geometry list of test_gpu_train_ops.py (N, Cin, Cout, Z, S, ksize, db) ...
WGRAD_EXACT = [(1, 1, 8, 1, 4, 3, True), (5, 13, 40, 2, 12, 3, False), (1, 40, 13, 3, 8, 3, True), (2, 8, 1, 4, 64, 3, True),
               (1, 13, 8, 2, 9, 3, True), (2, 8, 13, 4, 7, 3, False), (5, 229, 40, 1, 4, 3, False), (1, 229, 229, 2, 8, 1, True),
               (1, 13, 229, 4, 12, 1, True), (5, 1, 13, 3, 64, 1, False), (2, 64, 64, 2, 16, 3, True)]
# ... plus: the widest decoder input; many chunks over few channel tiles; Cin % 32 != 0 (Cout a multiple); Cout % 32 != 0 (Cin a
# multiple), the latter two at Z = 3 (the 4 x 8 tile) and with the 1x1x1 form's wave split
WGRAD_MORE = [(1, 1253, 512, 2, 8, 3, True), (4, 64, 64, 2, 64, 3, True), (2, 72, 64, 3, 16, 3, True), (2, 64, 72, 3, 16, 1, True)]


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize,with_db", WGRAD_EXACT + WGRAD_MORE)
def test_wgrad_mfma_exact_integers(N, Cin, Cout, Z, S, ksize, with_db):
    """Integer operands in [-3, 3]: every partial sum is an integer below 2^24 (K <= 5 * 3 * 64^2 * 9), so any order is exact."""
    x = util.rand_int((N, Cin, Z, S, S), -3, 3, 21)
    dy = util.rand_int((N, Cout, Z, S, S), -3, 3, 22)
    dw, db = _wgrad(x, dy, ksize, with_db)
    rdw, rdb = _wgrad_ref(x.double(), dy.double(), ksize)
    _equal("dw", dw, rdw)
    if with_db:
        _equal("db", db, rdb)


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize", [(2, 40, 13, 2, 16, 3), (1, 229, 229, 2, 8, 1), (4, 64, 64, 2, 64, 3)])
def test_wgrad_mfma_accumulate(N, Cin, Cout, Z, S, ksize):
    """accumulate 0 overwrites a NaN-prefilled dw / db completely (_wgrad asserts it); two calls with accumulate 1 on zeroed buffers
    give exactly twice one call (integer data).  The first case reduces over chunks, the second writes dW directly, the third has
    128 chunks."""
    x = util.rand_int((N, Cin, Z, S, S), -3, 3, 25)
    dy = util.rand_int((N, Cout, Z, S, S), -3, 3, 26)
    dw1, db1 = _wgrad(x, dy, ksize, True)
    assert not torch.isnan(db1).any()
    xc, yc = util.to_cb8(x.to(DEV)), util.to_cb8(dy.to(DEV))
    dw = torch.zeros((Cout, Cin, 27 if ksize == 3 else 1), device=DEV)
    db = torch.zeros((Cout,), device=DEV)
    for _ in range(2):
        _call(xc, yc, dw, db, 1, N, Cin, Cout, Z, S, ksize)
    torch.cuda.synchronize()
    _equal("dw", dw.cpu(), 2.0 * dw1.double())
    _equal("db", db.cpu(), 2.0 * db1.double())


def _chunks(N, Z, S, Cin, Cout):
    """conv_wgrad_chunks (csrc/tm_train.hip): (in-plane tile, tiles per chunk, chunks) -- a function of the geometry alone."""
    tw = 8 if S >= 8 else 4
    th = 8 if (S >= 8 and Z <= 2) else 4
    tiles = N * ((S + th - 1) // th) * ((S + tw - 1) // tw)
    ct = ((Cout + 31) // 32) * ((Cin + 31) // 32)
    chunks = max(1, min(256, tiles, 1024 // ct, (16 << 20) // (Cout * Cin * 27)))
    per = (tiles + chunks - 1) // chunks
    return th, tw, per, (tiles + per - 1) // per


@pytest.mark.parametrize("N,Cin,Cout,Z,S", [(1, 256, 256, 2, 16), (2, 1253, 512, 2, 8), (4, 64, 64, 2, 64), (2, 72, 40, 2, 16)])
def test_wgrad_mfma_float(N, Cin, Cout, Z, S, capsys):
    """Random normal operands, |dw - ref| <= B U sum |x dy| elementwise against float64, U = 2^-24.

    B from the kernel's accumulation order (3x3x3 form).  One workgroup accumulates one chunk: `per` spatial tiles of Z * TH * TW
    voxels each, and a tap's accumulator register takes one v_mfma_f32_32x32x2_f32 per voxel pair of every tile, in order, each adding
    two products to the running sum.  Counting the two products of a k-step as two sequential additions (the worst order the unit
    could use), a product passes through at most  per * Z * TH * TW  roundings inside its chunk (fewer where a z plane of the tap
    falls outside the volume and the step is skipped).  conv_wgrad_reduce_kernel then adds the `chunks` partials in index order:
    chunks - 1 more roundings; the products themselves are exact inside the MFMA, and one unit of slack covers the second-order
    term of (1 + U)^B - 1 at B U < 1e-4:
        B = per * Z * TH * TW + (chunks - 1) + 1.
    At the four shapes: 256 -> 256, S 16: tile 8 x 8, 4 chunks of 1 tile, B = 132 (K + 5 = 517); 1253 -> 512, S 8, N 2: 640 channel
    tiles so 1 chunk of 2 tiles written directly, B = 257 (K + 5 = 261); 64 -> 64, S 64, N 4: 128 chunks of 2 tiles (the 64 MB cap
    on the partials), B = 384 (K + 5 = 32773); 72 -> 40, S 16, N 2 (partial channel tiles on both sides, through the reduction):
    8 chunks of 1 tile, B = 136 (K + 5 = 1029).  B may never exceed the VALU kernel's K + 5, K = N Z S^2: asserted below.
    db (chan_sum_kernel, unchanged): K / 256 + 9 as in test_conv_wgrad_float_production_shape.
    The worst |d| / bound of each case is printed before the assertion (pytest -s)."""
    g = torch.Generator().manual_seed(100 + Cin)
    x, dy = torch.randn((N, Cin, Z, S, S), generator=g), torch.randn((N, Cout, Z, S, S), generator=g)
    dw, db = _wgrad(x, dy, 3, True)
    rdw, mag = _wgrad_ref_mm(x.double(), dy.double()), _wgrad_ref_mm(x.double().abs(), dy.double().abs())
    th, tw, per, chunks = _chunks(N, Z, S, Cin, Cout)
    K = N * Z * S * S
    B = per * Z * th * tw + (chunks - 1) + 1
    assert B <= K + 5, (B, K)
    d = (dw.double() - rdw).abs()
    worst = float((d / (B * U * mag).clamp_min(1e-300)).max())
    with capsys.disabled():
        print(f"\nwgrad_mfma float {Cin}->{Cout} S={S} Z={Z} N={N}: chunks={chunks} per={per} B={B} (K+5={K + 5}) "
              f"max|d|={float(d.max()):.3e} worst|d|/bound={worst:.4f}")
    assert bool((d <= B * U * mag).all()) and not torch.isnan(dw).any(), f"dw: worst |d|/bound = {worst:.3g}"
    rdb, dbmag = dy.double().sum((0, 2, 3, 4)), dy.double().abs().sum((0, 2, 3, 4))
    assert bool(((db.double() - rdb).abs() <= (K // 256 + 9) * U * dbmag).all())


def test_wgrad_mfma_matches_conv3d_weight_reference():
    """The tap-by-tap float64 reference used for the wide float cases is conv3d_weight itself (float64, small case)."""
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn((2, 5, 3, 6, 6), generator=g).double(), torch.randn((2, 7, 3, 6, 6), generator=g).double()
    assert torch.allclose(_wgrad_ref_mm(x, dy), _wgrad_ref(x, dy, 3)[0], rtol=1e-12, atol=1e-12)


def test_wgrad_mfma_error_paths():
    """TM_ERR_ARG (-1) before any launch: the outputs keep their NaN prefill."""
    L = _lib.lib()
    xc = torch.zeros((1, 1, 2, 8, 8, 8), device=DEV)
    dw = torch.full((8, 8, 27), NAN, device=DEV)
    p, q, w = _lib.ptr(xc), _lib.ptr(xc), _lib.ptr(dw)
    assert L.tm_op_conv_wgrad_dev(p, q, w, None, 0, 1, 8, 8, 2, 8, 2, _st()) == -1 and b"ksize" in L.tm_last_error()
    assert L.tm_op_conv_wgrad_dev(p, q, w, None, 0, 1, 8, 8, 5, 8, 3, _st()) == -1 and b"Z" in L.tm_last_error()
    assert L.tm_op_conv_wgrad_dev(p, q, w, None, 0, 1, 8, 8, 0, 8, 3, _st()) == -1
    assert L.tm_op_conv_wgrad_dev(None, q, w, None, 0, 1, 8, 8, 2, 8, 3, _st()) == -1 and b"null" in L.tm_last_error()
    assert L.tm_op_conv_wgrad_dev(p, None, w, None, 0, 1, 8, 8, 2, 8, 3, _st()) == -1
    assert L.tm_op_conv_wgrad_dev(p, q, None, None, 0, 1, 8, 8, 2, 8, 3, _st()) == -1
    assert L.tm_op_conv_wgrad_dev(p, q, w, None, 2, 1, 8, 8, 2, 8, 3, _st()) == -1 and b"accumulate" in L.tm_last_error()
    assert L.tm_op_conv_wgrad_dev(p, q, w, None, 0, 0, 8, 8, 2, 8, 3, _st()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all())
