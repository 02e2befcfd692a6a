"""-m gpu: the resident conv ops at Z = 8 (rna_slc 16): the z-slab form of the MFMA weight gradient (tm_op_conv_wgrad_dev ->
conv_wgrad_mfma_slab_kernel, csrc/tm_train.hip) and the packed forward conv / data gradient (tm_op_conv_pack_dev,
tm_op_conv_mfma_packed, tm_op_conv_dgrad_packed), held to float64 references of their definitions.  Rules of
test_gpu_conv_wgrad_mfma.py: integer cases are exact (torch.equal against float64), the float cases get a bound derived from the
kernel's own accumulation order, outputs start as NaN, two calls must agree in every bit."""
import pytest
import torch
import torch.nn.functional as F

import train_op_ref as R
import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = R.U
Z8 = 8


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
    """The 3x3x3 definition tap by tap as [Cout, K] @ [K, Cin] float64 products (as in test_gpu_conv_wgrad_mfma.py, which checks it
    against conv3d_weight)."""
    N, Cin, Z, S, _ = x.shape
    Cout = dy.shape[1]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
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


# (N, Cin, Cout, Z, S, ksize, db): the smallest plane (the gene pyramid's S); an edge tile in both axes; two images, 4 x 8 tiles with
# an edge row; Cin % 32 != 0; Cout % 32 != 0; the widest gene input at S = 4; many chunks over one channel tile; the 1x1x1 form twice
WGRAD_Z8_EXACT = [(1, 1, 8, Z8, 4, 3, True), (1, 40, 13, Z8, 7, 3, True), (2, 13, 40, Z8, 12, 3, False), (1, 72, 64, Z8, 16, 3, True),
                  (1, 64, 72, Z8, 16, 3, True), (1, 229, 40, Z8, 4, 3, False), (2, 8, 8, Z8, 64, 3, True), (1, 13, 229, Z8, 12, 1, True),
                  (2, 64, 72, Z8, 16, 1, True)]


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize,with_db", WGRAD_Z8_EXACT)
def test_wgrad_z8_exact_integers(N, Cin, Cout, Z, S, ksize, with_db):
    """Integer operands in [-3, 3]: every partial sum is an integer below 2 * 8 * 64^2 * 9 * 9 < 2^24, so any order is exact."""
    x = util.rand_int((N, Cin, Z, S, S), -3, 3, 21)
    dy = util.rand_int((N, Cout, Z, S, S), -3, 3, 22)
    dw, db = _wgrad(x, dy, ksize, with_db)
    if ksize == 3 and S >= 64:
        rdw, rdb = _wgrad_ref_mm(x.double(), dy.double()), dy.double().sum((0, 2, 3, 4))
    else:
        rdw, rdb = _wgrad_ref(x.double(), dy.double(), ksize)
    _equal("dw", dw, rdw)
    if with_db:
        _equal("db", db, rdb)


def test_wgrad_z8_slab_seams():
    """dY nonzero in plane zy only, X in plane zx only, all 64 (zy, zx) pairs (N = 1, 8 -> 8, S = 4): dW equals the float64 reference,
    which is zero unless |zx - zy| <= 1 and then nonzero only in the taps kz = zx - zy + 1.  A missing or doubled halo plane at the
    boundary between the slabs z 0 .. 3 and 4 .. 7 shows here as a named (zy, zx) pair."""
    N, Ci, Co, S = 1, 8, 8, 4
    xf = util.rand_int((N, Ci, Z8, S, S), 1, 3, 31)          # strictly positive: an expected tap plane cannot cancel to zero
    yf = util.rand_int((N, Co, Z8, S, S), 1, 3, 32)
    bad = []
    for zy in range(Z8):
        for zx in range(Z8):
            x, dy = torch.zeros_like(xf), torch.zeros_like(yf)
            x[:, :, zx], dy[:, :, zy] = xf[:, :, zx], yf[:, :, zy]
            dw, _ = _wgrad(x, dy, 3, False)
            ref, _ = _wgrad_ref(x.double(), dy.double(), 3)
            kzs = sorted(set(int(k) for k in torch.nonzero(ref.reshape(Co, Ci, 3, 9).abs().sum((0, 1, 3))).reshape(-1)))
            assert kzs == ([zx - zy + 1] if abs(zx - zy) <= 1 else []), (zy, zx, kzs)          # the reference itself
            if not torch.equal(dw.double(), ref):
                bad.append((zy, zx))
    assert not bad, f"(zy, zx) pairs with a wrong dW: {bad}"


@pytest.mark.parametrize("N,Cin,Cout,S,ksize,direct", [(1, 40, 13, 16, 3, False), (1, 736, 736, 4, 3, True), (2, 64, 72, 16, 1, False)])
def test_wgrad_z8_accumulate(N, Cin, Cout, S, ksize, direct):
    """Two calls with accumulate 1 on zeroed buffers give exactly twice one call (integer data).  The first and third case go through
    the chunk reduction (16 and 32 chunks); in the second 23 x 23 = 529 channel tiles leave one chunk (its 2 slab tiles), so the kernel
    adds into dW itself."""
    assert (_chunks(N, Z8, S, Cin, Cout)[3] == 1) == direct
    x = util.rand_int((N, Cin, Z8, S, S), -3, 3, 25)
    dy = util.rand_int((N, Cout, Z8, S, S), -3, 3, 26)
    dw1, db1 = _wgrad(x, dy, ksize, True)
    assert not torch.isnan(db1).any()
    xc, yc = util.to_cb8(x.to(DEV)), util.to_cb8(dy.to(DEV))
    dw = torch.zeros((Cout, Cin, 27 if ksize == 3 else 1), device=DEV)
    db = torch.zeros((Cout,), device=DEV)
    for _ in range(2):
        _call(xc, yc, dw, db, 1, N, Cin, Cout, Z8, S, ksize)
    torch.cuda.synchronize()
    _equal("dw", dw.cpu(), 2.0 * dw1.double())
    _equal("db", db.cpu(), 2.0 * db1.double())


def _chunks(N, Z, S, Cin, Cout):
    """conv_wgrad_chunks at Z = 8 (csrc/tm_train.hip): the tile list is (n, z slab of 4 planes, ty, tx) with the in-plane tile 4 x 8
    from S = 8 on and 4 x 4 below; about 1024 workgroups, at most one chunk per tile, at most 256, at most 16 Mi floats of partials.
    Returns (th, tw, tiles per chunk, chunks) -- a function of the geometry alone."""
    assert Z == 8
    th, tw = 4, (8 if S >= 8 else 4)
    tiles = N * (Z // 4) * ((S + th - 1) // th) * ((S + tw - 1) // tw)
    ct = ((Cout + 31) // 32) * ((Cin + 31) // 32)
    chunks = max(1, min(256, tiles, 1024 // ct, (16 << 20) // (Cout * Cin * 27)))
    per = (tiles + chunks - 1) // chunks
    return th, tw, per, (tiles + per - 1) // per


@pytest.mark.parametrize("N,Cin,Cout,S", [(1, 64, 64, 16), (1, 72, 40, 16), (2, 16, 16, 64)])
def test_wgrad_z8_float(N, Cin, Cout, S, capsys):
    """Random normal operands, |dw - ref| <= B U sum |x dy| elementwise against float64, U = 2^-24.

    B from the slab kernel's accumulation order, derived as in test_gpu_conv_wgrad_mfma.py: one workgroup accumulates one chunk of
    `per` slab tiles of 4 * TH * TW output voxels each; a tap's accumulator takes one v_mfma_f32_32x32x2_f32 per voxel pair of every
    tile in order, each adding two products, counted as two sequential additions; so a product passes through at most
    per * 4 * TH * TW roundings inside its chunk (fewer where the tap's X plane is outside the volume), then the reduction adds the
    `chunks` partials in index order (chunks - 1 roundings), and one unit of slack covers the second-order term:
        B = per * 4 * TH * TW + (chunks - 1) + 1.
    64 -> 64, S 16: 16 tiles (2 slabs x 4 x 2), 16 chunks of 1, B = 144 (K + 5 = 2053); 72 -> 40, S 16: partial channel tiles on both
    sides, 16 chunks of 1, B = 144; 16 -> 16, S 64, N 2: 512 tiles, 256 chunks of 2, B = 512 (K + 5 = 65541).  B may never exceed
    the VALU kernel's K + 5, K = N Z S^2: asserted.  db (chan_sum_kernel, unchanged): K / 256 + 9.
    The worst |d| / bound of each case is printed before the assertion (pytest -s); measured: profiles/train_slc16.txt."""
    Z = Z8
    g = torch.Generator().manual_seed(100 + Cin)
    x, dy = torch.randn((N, Cin, Z, S, S), generator=g), torch.randn((N, Cout, Z, S, S), generator=g)
    dw, db = _wgrad(x, dy, 3, True)
    rdw, mag = _wgrad_ref_mm(x.double(), dy.double()), _wgrad_ref_mm(x.double().abs(), dy.double().abs())
    th, tw, per, chunks = _chunks(N, Z, S, Cin, Cout)
    K = N * Z * S * S
    B = per * 4 * th * tw + (chunks - 1) + 1
    assert B <= K + 5, (B, K)
    d = (dw.double() - rdw).abs()
    worst = float((d / (B * U * mag).clamp_min(1e-300)).max())
    with capsys.disabled():
        print(f"\nwgrad_z8 float {Cin}->{Cout} S={S} Z={Z} N={N}: chunks={chunks} per={per} B={B} (K+5={K + 5}) "
              f"max|d|={float(d.max()):.3e} worst|d|/bound={worst:.4f}")
    assert bool((d <= B * U * mag).all()) and not torch.isnan(dw).any(), f"dw: worst |d|/bound = {worst:.3g}"
    rdb, dbmag = dy.double().sum((0, 2, 3, 4)), dy.double().abs().sum((0, 2, 3, 4))
    assert bool(((db.double() - rdb).abs() <= (K // 256 + 9) * U * dbmag).all())


def test_wgrad_z8_error_paths():
    """Z = 5, 6, 7 return TM_ERR_ARG (-1) with Z in the message before any launch: the outputs keep their NaN prefill."""
    L = _lib.lib()
    xc = torch.zeros((1, 1, 8, 8, 8, 8), device=DEV)
    dw = torch.full((8, 8, 27), NAN, device=DEV)
    db = torch.full((8,), NAN, device=DEV)
    p, w, b = _lib.ptr(xc), _lib.ptr(dw), _lib.ptr(db)
    for Z in (5, 6, 7):
        assert L.tm_op_conv_wgrad_dev(p, p, w, b, 0, 1, 8, 8, Z, 8, 3, _st()) == -1 and b"Z" in L.tm_last_error(), Z
        assert L.tm_op_conv_wgrad_dev(p, p, w, b, 0, 1, 8, 8, Z, 8, 1, _st()) == -1 and b"Z" in L.tm_last_error(), Z
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())


# ---- the packed forward conv and data gradient at Z = 8 ---------------------------------------------------------------------------
def _pack(w_dev, Cout, Cin, ksize, Z, role):
    n = _lib.lib().tm_conv_pack_floats(Cout, Cin, ksize, Z, role)
    assert n > 0
    pk = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().tm_op_conv_pack_dev(_lib.ptr(w_dev), _lib.ptr(pk), Cout, Cin, ksize, Z, role, _st()), "tm_op_conv_pack_dev")
    return pk


def _nan_cb8(N, Cc, Z, S):
    return torch.full((N, (Cc + 7) // 8, Z, S, S, 8), NAN, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("N,Cin,Cout,S", [(2, 13, 40, 8), (1, 72, 64, 16)])
def test_packed_conv_and_dgrad_z8_exact_integers(N, Cin, Cout, S, ksize):
    """y = conv(x) + b and dx on device packs at Z = 8 against F.conv3d and its autograd in float64, integers in [-3, 3]: every sum is
    an integer below 72 * 27 * 9 < 2^24, so any order is exact.  Pad channel slots of the CB8 outputs are zero."""
    Z, k, pad = Z8, ksize, ksize // 2
    x = util.rand_int((N, Cin, Z, S, S), -3, 3, 41)
    w = util.rand_int((Cout, Cin, k, k, k), -3, 3, 42)
    b = util.rand_int((Cout,), -3, 3, 43)
    dy = util.rand_int((N, Cout, Z, S, S), -3, 3, 44)
    xl = x.double().clone().requires_grad_(True)
    ref = F.conv3d(xl, w.double(), b.double(), padding=pad)
    ref.backward(dy.double())
    wd = w.float().contiguous().to(DEV)
    pk0, pk1 = _pack(wd, Cout, Cin, ksize, Z, 0), _pack(wd, Cout, Cin, ksize, Z, 1)
    assert not torch.isnan(pk0).any() and not torch.isnan(pk1).any(), "pack not fully written"
    xc, yc, bd = util.to_cb8(x.float().to(DEV)), util.to_cb8(dy.float().to(DEV)), b.float().to(DEV)
    y, dx = _nan_cb8(N, Cout, Z, S), _nan_cb8(N, Cin, Z, S)
    _lib.check(_lib.lib().tm_op_conv_mfma_packed(_lib.ptr(xc), _lib.ptr(pk0), _lib.ptr(bd), _lib.ptr(y), N, Cin, Cout, Z, S, ksize, _st()),
               "tm_op_conv_mfma_packed")
    _lib.check(_lib.lib().tm_op_conv_dgrad_packed(_lib.ptr(yc), _lib.ptr(pk1), _lib.ptr(dx), N, Cin, Cout, Z, S, ksize, _st()),
               "tm_op_conv_dgrad_packed")
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(dx).any()
    _equal("y", util.from_cb8(y, Cout), ref.detach())
    _equal("dx", util.from_cb8(dx, Cin), xl.grad)
