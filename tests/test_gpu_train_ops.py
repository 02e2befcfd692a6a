"""-m gpu: every training-slice operator (include/teramind_hip.h, training slice sections; csrc/tm_train.hip) on its own, against
a float64 CPU reference of its definition (tests/train_op_ref.py), at the shapes where its tiles, chunks and grid caps end.

Rules of every case:
  * exact cases use small integers (util.rand_int in [-3, 3]), so every fp32 sum of products is exact: torch.equal against
    float64.  A dropped, doubled or mis-indexed term fails whatever K is.
  * float cases use randn data and a bound derived from the fp32 accumulation length of the kernel (fixed order) or from
    the ulp error of the transcendental (train_op_ref: U = 2^-24), never from the observed error.
  * outputs start as NaN (unless the op accumulates): every real element must be written, and the pad channel slots of a
    CB8 output must be zero (every consumer's K loop reads them).
  * every op runs twice on the same inputs and must give the same bits (fixed-order reductions, no float atomics)."""
import ctypes as C
import math

import pytest
import torch

import train_op_ref as R
import util
from oracle import teramind_cpu as tc
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = R.U


def _st():
    return _lib.current_stream_ptr()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, k=1.0):
    return torch.randn(shape, generator=_gen(seed)) * k


def _nan_cb8(N, Cc, Z, S):
    return torch.full((N, (Cc + 7) // 8, Z, S, S, 8), NAN, dtype=torch.float32, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _out_cb8(raw, Cc, name):
    """CB8 output -> float64 NCDHW on the CPU, after checking that nothing is NaN and the pad slots are zero."""
    assert not torch.isnan(raw).any(), f"{name}: {int(torch.isnan(raw).sum())} elements not written"
    if Cc % 8:
        assert float(raw[:, -1, ..., Cc % 8:].abs().max()) == 0.0, f"{name}: pad channel slots not zero"
    return util.from_cb8(raw, Cc).cpu().double()


def _within(name, got, ref, bound):
    got = torch.as_tensor(got).double().cpu()
    d = (got - ref).abs()
    ok = bool(((d <= bound) & ~torch.isnan(got)).all())
    worst = float((d / bound.clamp_min(1e-300)).max()) if got.numel() else 0.0
    assert ok, f"{name}: max|d|={float(d.max()):.3e}, worst |d|/bound={worst:.3g}, nan={int(torch.isnan(got).sum())}"


def _equal(name, got, ref):
    got = torch.as_tensor(got).double().cpu()
    assert torch.equal(got, ref), util.report(name, got, ref)


# ================================================================================================================= conv wgrad
def _wgrad(x, dy, ksize, with_db):
    N, Cin, Z, S, _ = x.shape
    Cout = dy.shape[1]
    xc, yc = util.to_cb8(x.to(DEV)), util.to_cb8(dy.to(DEV))
    taps = 27 if ksize == 3 else 1
    outs = []
    for _ in range(2):
        dw = torch.full((Cout, Cin, taps), NAN)
        db = torch.full((Cout,), NAN) if with_db else None
        _lib.check(_lib.lib().tm_op_conv_wgrad(_lib.ptr(xc), _lib.ptr(yc), _lib.ptr(dw), _lib.ptr(db), N, Cin, Cout, Z, S, ksize, _st()),
                   "tm_op_conv_wgrad")
        outs.append((dw, db))
    (dw, db), (dw2, db2) = outs
    assert _same_bits(dw, dw2) and (db is None or _same_bits(db, db2)), "wgrad not reproducible"
    return dw, db


def _wgrad_ref(x, dy, ksize):
    k, pad = (3, 1) if ksize == 3 else (1, 0)
    dw = torch.nn.grad.conv3d_weight(x, (dy.shape[1], x.shape[1], k, k, k), dy, padding=pad)
    return dw.reshape(dy.shape[1], x.shape[1], -1), dy.sum((0, 2, 3, 4))


# (N, Cin, Cout, Z, S, ksize, db): every Z the kernel stages (1-4); S below / on / above the 8 x 8 tile (7, 8, 9, 12) and many
# tiles (64); channel counts off the 8-block (1, 13, 229) and Cin != Cout
WGRAD_EXACT = [(1, 1, 8, 1, 4, 3, True), (5, 13, 40, 2, 12, 3, False), (1, 40, 13, 3, 8, 3, True), (2, 8, 1, 4, 64, 3, True),
               (1, 13, 8, 2, 9, 3, True), (2, 8, 13, 4, 7, 3, False), (5, 229, 40, 1, 4, 3, False), (1, 229, 229, 2, 8, 1, True),
               (1, 13, 229, 4, 12, 1, True), (5, 1, 13, 3, 64, 1, False), (2, 64, 64, 2, 16, 3, True)]


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize,with_db", WGRAD_EXACT)
def test_conv_wgrad_exact_integers(N, Cin, Cout, Z, S, ksize, with_db):
    x = util.rand_int((N, Cin, Z, S, S), -3, 3, 21)
    dy = util.rand_int((N, Cout, Z, S, S), -3, 3, 22)
    dw, db = _wgrad(x, dy, ksize, with_db)
    rdw, rdb = _wgrad_ref(x.double(), dy.double(), ksize)
    _equal("dw", dw, rdw)
    if with_db:
        _equal("db", db, rdb)


def test_conv_wgrad_float_production_shape():
    """C = 256 -> 256 at S = 16 (the 16-px level of the default model).  Every dW element is a sum of at most
    K = N Z S^2 = 512 products (fma), accumulated per 8 x 8 tile and then over the 4 tiles: at most K + 4 roundings of partial
    sums, so |err| <= (K + 5) U sum |x dy|.  db (chan_sum_kernel): 256 lanes of N Z S^2 / 256 terms, a 64-lane tree (6) and
    4 partials (2): at most K / 256 + 8 roundings."""
    N, Cin, Cout, Z, S = 1, 256, 256, 2, 16
    x, dy = _randn((N, Cin, Z, S, S), 23), _randn((N, Cout, Z, S, S), 24)
    dw, db = _wgrad(x, dy, 3, True)
    rdw, rdb = _wgrad_ref(x.double(), dy.double(), 3)
    mag, dbmag = _wgrad_ref(x.double().abs(), dy.double().abs(), 3)
    K = N * Z * S * S
    _within("dw", dw, rdw, (K + 5) * U * mag)
    _within("db", db, rdb, (K // 256 + 9) * U * dbmag)


# ================================================================================================================= conv dgrad
# (N, Cin (the output here), Cout, Z, S, ksize): Z 1-4, Cin 13 / 229 (pad slots), Cout 40 / 1792 (K up to 1792 * 27)
DGRAD_EXACT = [(1, 13, 40, 1, 4, 3), (2, 229, 40, 3, 8, 3), (1, 13, 1792, 2, 8, 1), (1, 229, 1792, 2, 4, 3), (2, 13, 40, 4, 16, 3),
               (1, 13, 40, 2, 64, 3), (3, 229, 40, 4, 8, 1), (1, 229, 1792, 1, 8, 1)]


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize", DGRAD_EXACT)
def test_conv_dgrad_exact_integers(N, Cin, Cout, Z, S, ksize):
    k, pad = (3, 1) if ksize == 3 else (1, 0)
    dy = util.rand_int((N, Cout, Z, S, S), -3, 3, 31)
    w = util.rand_int((Cout, Cin, k, k, k), -3, 3, 32)
    yc = util.to_cb8(dy.to(DEV))
    outs = []
    for _ in range(2):
        dx = _nan_cb8(N, Cin, Z, S)
        _lib.check(_lib.lib().tm_op_conv_dgrad(_lib.ptr(yc), _lib.ptr(w.contiguous()), _lib.ptr(dx), N, Cin, Cout, Z, S, ksize, _st()),
                   "tm_op_conv_dgrad")
        outs.append(dx)
    assert _same_bits(outs[0], outs[1])
    ref = torch.nn.grad.conv3d_input((N, Cin, Z, S, S), w.double(), dy.double(), padding=pad)
    _equal("dx", _out_cb8(outs[0], Cin, "dx"), ref)


# ================================================================================================================= gemm
SENT = -12345.5          # C border sentinel: must survive every call


def _strided(buf, batch, rows, cols, sr, sc, sb):
    return buf.as_strided((batch, rows, cols), (sb, sr, sc))


def _gemm(A, B, bias, M, N, K, ab_strides, batch, bias_mode, accumulate, alpha, c0):
    """Runs tm_op_gemm_f32 with C at leading dimension N + 3 (and a gap between batches) in a buffer whose border holds SENT.
    c0: [batch, M, N] prefill of C (accumulate) or None (NaN).  Returns the whole C buffer (host)."""
    ldc, scb = N + 3, M * (N + 3) + 5
    nC = (batch - 1) * scb + (M - 1) * ldc + N + 7
    sam, sak, sbk, sbn, sab, sbb = ab_strides
    st = (sam, sak, sbk, sbn, ldc, 1, sab, sbb, scb)
    Ad, Bd, biasd = A.to(DEV), B.to(DEV), (None if bias is None else bias.to(DEV))      # held until the calls return
    outs = []
    for _ in range(2):
        Cb = torch.full((nC,), SENT, dtype=torch.float32)
        _strided(Cb, batch, M, N, ldc, 1, scb).copy_(c0 if c0 is not None else torch.full((batch, M, N), NAN))
        Cd = Cb.to(DEV)
        arr = (C.c_long * 9)(*st)
        _lib.check(_lib.lib().tm_op_gemm_f32(_lib.ptr(Ad), _lib.ptr(Bd), _lib.ptr(biasd), _lib.ptr(Cd), M, N, K, C.cast(arr, C.c_void_p),
                                             batch, bias_mode, accumulate, alpha, _st()),
                   "tm_op_gemm_f32")
        outs.append(Cd.cpu())
    assert _same_bits(outs[0], outs[1]), "gemm not reproducible"
    return outs[0], (ldc, scb)


# The stride forms of teramind_amd.train_model (linear / its dx, dW, db; the gene-attention batched products), as functions
# of (M, N, K, batch) -> (sam, sak, sbk, sbn, sab, sbb) and the sizes of the A and B buffers.
FORMS = {
    "linear": lambda M, N, K, b: ((K, 1, 1, K, 0, 0), M * K, N * K),              # y = x W^T:   A x [M][K], B W [N][K]
    "linear_dx": lambda M, N, K, b: ((K, 1, N, 1, 0, 0), M * K, K * N),           # dx = g W:    A g [M][K], B W [K][N]
    "linear_dw": lambda M, N, K, b: ((1, M, N, 1, 0, 0), K * M, K * N),           # dW = g^T x:  A g [K][M], B x [K][N]
    "linear_db": lambda M, N, K, b: ((1, M, 0, 0, 0, 0), K * M, 1),               # db = g^T 1:  stride-0 B (N = 1)
    "qqT": lambda M, N, K, b: ((K, 1, 1, K, M * K, N * K), b * M * K, b * N * K),  # q q^T per batch
    "Pv": lambda M, N, K, b: ((K, 1, N, 1, M * K, K * N), b * M * K, b * K * N),   # P v
    "PTg": lambda M, N, K, b: ((1, M, N, 1, M * K, K * N), b * M * K, b * K * N),  # P^T g
}

# (form, M, N, K, batch, bias_mode, accumulate, alpha): M, N in {1, 63, 64, 65, 229}, K in {1, 15, 16, 17, 229, 4097}
GEMM_CASES = [
    ("linear", 65, 229, 17, 1, 1, 0, 1.0), ("linear", 1, 63, 4097, 1, 1, 0, 1.0), ("linear", 64, 65, 229, 1, 2, 0, 1.0),
    ("linear", 65, 64, 1, 1, 0, 0, 1.0), ("linear", 229, 63, 16, 3, 2, 1, 1.0),
    ("linear_dx", 229, 64, 16, 1, 0, 0, 1.0), ("linear_dx", 63, 1, 15, 1, 1, 1, 1.0),
    ("linear_dw", 63, 65, 4097, 1, 0, 0, 1.0), ("linear_dw", 229, 229, 15, 1, 0, 1, 1.0),
    ("linear_db", 229, 1, 1001, 1, 0, 0, 1.0), ("linear_db", 64, 1, 15, 1, 0, 0, 1.0),
    ("qqT", 65, 65, 15, 17, 0, 0, 1.0 / 15), ("qqT", 64, 64, 64, 3, 0, 0, 1.0 / 64),
    ("Pv", 63, 229, 63, 3, 0, 0, 1.0), ("Pv", 37, 17, 37, 17, 1, 0, 1.0),
    ("PTg", 1, 65, 1, 17, 0, 0, 1.0), ("PTg", 65, 64, 65, 3, 0, 1, 1.0 / 64), ("PTg", 37, 16, 37, 3, 0, 1, 1.0 / 16),
]


def _gemm_case(form, M, N, K, batch, bias_mode, accumulate, alpha, ints):
    st, na, nb = FORMS[form](M, N, K, batch)
    mk = (lambda n, s: util.rand_int((n,), -3, 3, s)) if ints else (lambda n, s: _randn((n,), s))
    A, B = mk(na, 41), (torch.ones(1) if form == "linear_db" else mk(nb, 42))
    bias = None if not bias_mode else util.rand_int(((N if bias_mode == 1 else M),), -3, 3, 43)
    c0 = util.rand_int((batch, M, N), -3, 3, 44) if accumulate else None
    got, (ldc, scb) = _gemm(A, B, bias, M, N, K, st, batch, bias_mode, accumulate, alpha, c0)
    sam, sak, sbk, sbn, sab, sbb = st
    Av, Bv = _strided(A.double(), batch, M, K, sam, sak, sab), _strided(B.double(), batch, K, N, sbk, sbn, sbb)
    prod, mag = torch.bmm(Av, Bv), torch.bmm(Av.abs(), Bv.abs())
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    bterm = torch.zeros(1, 1, 1, dtype=torch.float64) if bias is None else \
        (bias.double()[None, None, :] if bias_mode == 1 else bias.double()[None, :, None])
    cterm = c0.double() if accumulate else torch.zeros(1, 1, 1, dtype=torch.float64)
    region = torch.zeros(got.shape, dtype=torch.bool)
    _strided(region, batch, M, N, ldc, 1, scb).fill_(True)
    assert torch.equal(got[~region], torch.full_like(got[~region], SENT)), "gemm wrote outside C"
    g = _strided(got.double(), batch, M, N, ldc, 1, scb)
    return g, prod, mag, a32, bterm, cterm


@pytest.mark.parametrize("form,M,N,K,batch,bias_mode,accumulate,alpha", GEMM_CASES)
def test_gemm_f32_exact_integers(form, M, N, K, batch, bias_mode, accumulate, alpha):
    g, prod, mag, a32, bterm, cterm = _gemm_case(form, M, N, K, batch, bias_mode, accumulate, alpha, True)
    f32 = lambda t: t.float().double()
    if math.frexp(a32)[0] == 0.5:
        # alpha a power of two: the sum is exact, and so is alpha * sum; bias and C add with one rounding each
        _equal("C", g, f32(f32(prod * a32 + bterm) + cterm))
    else:
        # alpha * sum + bias (+ C): at most three roundings of those three terms (fma contraction only removes some)
        _within("C", g, prod * a32 + bterm + cterm, 3 * U * (prod.abs() * a32 + bterm.abs() + cterm.abs()))


@pytest.mark.parametrize("form,M,N,K,batch", [("linear_dw", 63, 65, 4097, 1), ("qqT", 65, 65, 229, 3)])
def test_gemm_f32_float(form, M, N, K, batch):
    """A k-ordered fma chain of K products per element: |err| <= (K + 1) U sum_k |a b| (one more for alpha)."""
    g, prod, mag, a32, bterm, cterm = _gemm_case(form, M, N, K, batch, 0, 0, 1.0, False)
    _within("C", g, prod, (K + 2) * U * mag)


# ================================================================================================================= rows
ROW_SHAPES = [(1, 1), (3, 37), (4, 63), (5, 64), (1001, 65), (3, 229), (5, 4096), (4, 4096)]
ROW_CASES = [(op, r, d) for op in range(4) for r, d in ROW_SHAPES] + [(op, 3, 8192) for op in (0, 2, 3)] + [(0, 1001, 229), (1, 1001, 64)]


def _rows(op, x, w, g, rows, D):
    xd = x.to(DEV)
    wd = None if w is None else w.to(DEV)
    gd = None if g is None else g.to(DEV)
    outs = []
    for _ in range(2):
        y = torch.full((rows, D), NAN, device=DEV)
        dw = torch.full((D,), NAN, device=DEV) if op == 1 else None
        _lib.check(_lib.lib().tm_op_rows(op, _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(gd), _lib.ptr(y), _lib.ptr(dw), rows, D, _st()),
                   "tm_op_rows")
        outs.append((y.cpu(), None if dw is None else dw.cpu()))
    (y, dw), (y2, dw2) = outs
    assert _same_bits(y, y2) and (dw is None or _same_bits(dw, dw2)), "rows not reproducible"
    return y, dw


@pytest.mark.parametrize("op,rows,D", ROW_CASES)
def test_rows(op, rows, D):
    """Bounds: a row sum over D terms passes through at most R.depth_wave(D) additions (D / 64 per lane, 6 shuffle levels);
    rstd = 1 / sqrt(sum / D + eps) adds 4 roundings; expf as R.exp_rel_bound."""
    x = _randn((rows, D), 51)
    if op == 3:
        x = torch.softmax(_randn((rows, D), 55, 2.0).double(), -1).float()
    elif op == 2 and rows > 1:
        x[1::2] = (torch.rand((rows // 2, D), generator=_gen(56)) * 160 - 80)             # +-80 spread: exp range of fp32
    w = torch.rand(D, generator=_gen(52)) + 0.5 if op <= 1 else None
    g = _randn((rows, D), 53) if op in (1, 3) else None
    y, dw = _rows(op, x, w, g, rows, D)
    xd, dep = x.double(), R.depth_wave(D)
    er = (dep + 6) * U                                                        # rstd, relative
    if op == 0:
        ref, _ = R.rms_rows(xd, w.double())
        _within("y", y, ref, (er + 3 * U) * ref.abs())
    elif op == 1:
        wd, gd = w.double(), g.double()
        rdx, rdw = R.rms_rows_bwd(xd, wd, gd)
        _, r = R.rms_rows(xd, wd)
        xh = xd * r
        E = er + (dep + 6) * U
        _within("dx", y, rdx, 2 * E * r * ((gd * wd).abs() + xh.abs() * (gd * wd * xh).abs().mean(-1, keepdim=True)))
        nwg = (rows + 3) // 4
        _within("dw", dw, rdw, (er + (2 + (nwg + 7) // 8 + 3 + 2) * U) * (gd * xh).abs().sum(0))
    elif op == 2:
        ref = torch.softmax(xd, -1)
        m = xd.max(-1, keepdim=True).values
        re = (xd - m).abs() * U + R.exp_rel_bound(xd - m)                     # exp(x - m): the argument's rounding + expf
        rs = (ref * re).sum(-1, keepdim=True) + dep * U                       # the sum: its terms' errors + D-sum roundings
        _within("y", y, ref, (re + rs + U) * ref + R.FLT_MIN)
        assert torch.allclose(y.double().sum(-1), torch.ones(rows, dtype=torch.float64), atol=(dep + 8) * U * 4)
    else:
        gd = g.double()
        ref = R.softmax_bwd(xd, gd)
        dot = (gd * xd).sum(-1, keepdim=True)
        _within("y", y, ref, xd * (dep + 3) * U * ((gd * xd).abs().sum(-1, keepdim=True) + gd.abs() + dot.abs()) + U * ref.abs())


# ================================================================================================================= elementwise
SPECIAL = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -3e-45, 1.1754944e-38, 20.0, -20.0, 100.0, -100.0, 1.0, -1.0, 0.5, -1.2785,
                        3.0, -3.0, 6.0, -6.0, 1e-3, -1e-3], dtype=torch.float32)
EW_N = [0, 1, 255, 256, 257, 4096 * 256 + 3]


def _ew_data(n, seed):
    x = _randn((max(n, 1),), seed, 4.0)
    k = min(n, SPECIAL.numel())
    x[:k] = SPECIAL[torch.randperm(SPECIAL.numel(), generator=_gen(seed))[:k]]
    return x[:n]


def _ew(op, a, b, c, n):
    pad = 13
    dev = lambda t: None if t is None else torch.cat([t, torch.zeros(pad)]).to(DEV)
    ad, bd, cd = dev(a), dev(b), dev(c)
    outs = []
    for _ in range(2):
        o1 = torch.full((n + pad,), NAN, device=DEV)
        o1[n:] = SENT
        o2 = o1.clone() if op == 1 else None
        _lib.check(_lib.lib().tm_op_ew(op, _lib.ptr(ad), _lib.ptr(bd), _lib.ptr(cd), _lib.ptr(o1), _lib.ptr(o2), n, _st()), "tm_op_ew")
        outs.append([t.cpu() for t in (o1, o2) if t is not None])
    for t, t2 in zip(*outs):
        assert _same_bits(t, t2), "ew not reproducible"
        assert torch.equal(t[n:], torch.full((pad,), SENT)), "ew wrote past n"
        assert not torch.isnan(t[:n]).any(), "ew left elements unwritten"
    return [t[:n] for t in outs[0]]


@pytest.mark.parametrize("n", EW_N)
@pytest.mark.parametrize("op", [0, 1, 6, 7, 8])
def test_ew_exact(op, n):
    a, b, c = (util.rand_int((n,), -3, 3, 60 + i) for i in range(3))
    got = _ew(op, a, b if op in (0, 1, 6) else None, c if op in (0, 1) else None, n)
    a, b, c = a.double(), b.double(), c.double()
    ref = {0: [a + b * c], 1: [a * b, a * c], 6: [a + b], 7: [4 * a], 8: [a / 4]}[op]
    for i, (t, r) in enumerate(zip(got, ref)):
        _equal(f"o{i + 1}", t, r)


@pytest.mark.parametrize("n", EW_N)
@pytest.mark.parametrize("op", range(9))
def test_ew_float(op, n):
    """Special values (+-0, subnormals, FLT_MIN, +-20, +-100) among randn * 4.  Ops 1, 6, 7, 8 are one IEEE operation each:
    bit-equal to the CPU's fp32 result.  Op 0 may be contracted to an fma: 2 U (|a| + |b c|).  tanhf is held to 2 ulp
    (4 U relative); expf(t) to R.exp_rel_bound(t) (an exp2 of the rounded product t log2 e).  The bound of each formula
    follows its roundings (below).  Results below FLT_MIN may be lost (FLT_MIN absolute)."""
    a, b, c = _ew_data(n, 70), _ew_data(n, 71), _ew_data(n, 72)
    need_b, need_c = op in (0, 1, 3, 5, 6), op in (0, 1)
    got = _ew(op, a, b if need_b else None, c if need_c else None, n)
    if op in (1, 6, 7, 8):
        ref = {1: [a * b, a * c], 6: [a + b], 7: [4 * a], 8: [a * 0.25]}[op]
        for i, (t, r) in enumerate(zip(got, ref)):
            assert _same_bits(t, r), util.report(f"o{i + 1}", t, r)
        return
    a, b, c = a.double(), b.double(), c.double()
    o = got[0]
    if op == 0:
        _within("o1", o, a + b * c, 2 * U * (a.abs() + (b * c).abs()) + 2.0 ** -149)
        return
    x = a if op in (2, 4) else b
    if op in (2, 3):
        inner = R.KB * (x + R.KK * x ** 3)
        th = torch.tanh(inner)
        d_in = 6 * U * R.KB * (x.abs() + R.KK * x.abs() ** 3)            # four roundings + the two constants
        d_th = (1 - th * th) * d_in + 4 * U * th.abs()                    # tanhf: 2 ulp
        if op == 2:
            ref = R.gelu_tanh(x)
            bound = 0.5 * x.abs() * (d_th + U * (1 + th)) + 2 * U * ref.abs()
        else:
            poly = R.KB * (1 + 3 * R.KK * x * x)
            dg = R.gelu_tanh_grad(x)
            d_d = 0.5 * d_th + 0.5 * x.abs() * poly * (2 * th.abs() * d_th + 6 * U * (1 - th * th)) + 4 * U * (0.5 * (1 + th) + 0.5 * x.abs() * (1 - th * th) * poly)
            ref = a * dg
            bound = a.abs() * d_d + U * ref.abs()
    elif op == 4:
        ref = R.silu(x)
        bound = (R.exp_rel_bound(x) + 2 * U) * ref.abs()                  # expf(-x), 1 + e, the division
    else:
        sg = torch.sigmoid(x)
        h = 1 + x * (1 - sg)
        d_sg = (R.exp_rel_bound(x) + 2 * U) * sg
        d_h = x.abs() * (d_sg + U * (1 - sg)) + U * (x * (1 - sg)).abs() + U * h.abs()
        ref = a * sg * h
        bound = a.abs() * (d_sg * h.abs() + sg * d_h) + 2 * U * ref.abs()
    _within("o1", o, ref, bound + R.FLT_MIN)


# ================================================================================================================= modnorm
# (N, C, Z, S): voxel counts 75, 216, 36, 90, 98 (none a multiple of 64) and one 16-px level
MODNORM_CASES = [(3, 13, 1, 5), (2, 64, 3, 6), (1, 229, 4, 3), (5, 512, 2, 3), (1, 1, 2, 7), (2, 229, 2, 16)]


def _modnorm_inputs(N, Cc, Z, S):
    x = _randn((N, Cc, Z, S, S), 81)
    w = torch.rand(Cc, generator=_gen(82)) + 0.5
    sc, sh, g = _randn((N, Cc, Z, S, S), 83, 0.3), _randn((N, Cc, Z, S, S), 84, 0.3), _randn((N, Cc, Z, S, S), 85)
    return x, w, sc, sh, g


@pytest.mark.parametrize("N,Cc,Z,S", MODNORM_CASES)
def test_modnorm_forward(N, Cc, Z, S):
    """rstd: a sum of C squares (<= C + 1 roundings) and 4 more: e_r <= (C + 5) U; y = xh w (1 + s) + sh adds 5."""
    x, w, sc, sh, _ = _modnorm_inputs(N, Cc, Z, S)
    xc, scc, shc = util.to_cb8(x.to(DEV)), util.to_cb8(sc.to(DEV)), util.to_cb8(sh.to(DEV))
    outs = []
    for _ in range(2):
        y = _nan_cb8(N, Cc, Z, S)
        _lib.check(_lib.lib().tm_op_modnorm(_lib.ptr(xc), _lib.ptr(w), _lib.ptr(scc), _lib.ptr(shc), _lib.ptr(y), N, Cc, Z, S, _st()),
                   "tm_op_modnorm")
        outs.append(y)
    assert _same_bits(outs[0], outs[1])
    xd, wd, scd, shd = x.double(), w.double(), sc.double(), sh.double()
    ref = R.modnorm(xd, wd, scd, shd)
    n = tc.rms_norm_channels(xd, wd)
    _within("y", _out_cb8(outs[0], Cc, "y"), ref, ((Cc + 5) * U + 5 * U) * (n * (1 + scd)).abs() + 2 * U * ref.abs())


@pytest.mark.parametrize("N,Cc,Z,S", MODNORM_CASES)
def test_modnorm_backward(N, Cc, Z, S):
    """dx = r (dn w - xh mean_c(dn w xh)), dn = g (1 + s): every factor within e_r + a few U of its float64 value and the
    mean a C-term sum: |err| <= 2 E r (|dn w| + |xh| mean|dn w xh|), E = (2 C + 12) U.  dscale = g xh w: e_r + 3 U relative.
    dshift = g exactly.  dw: 64-lane sums, then the workgroup partials in 8 chains (R.depth_two_stage)."""
    x, w, sc, _, g = _modnorm_inputs(N, Cc, Z, S)
    xc, scc, gc = util.to_cb8(x.to(DEV)), util.to_cb8(sc.to(DEV)), util.to_cb8(g.to(DEV))
    outs = []
    for _ in range(2):
        dx, dsc, dsh = _nan_cb8(N, Cc, Z, S), _nan_cb8(N, Cc, Z, S), _nan_cb8(N, Cc, Z, S)
        dw = torch.full((Cc,), NAN)
        _lib.check(_lib.lib().tm_op_modnorm_bwd(_lib.ptr(xc), _lib.ptr(gc), _lib.ptr(w), _lib.ptr(scc), _lib.ptr(dx), _lib.ptr(dsc),
                                                _lib.ptr(dsh), _lib.ptr(dw), N, Cc, Z, S, _st()), "tm_op_modnorm_bwd")
        outs.append((dx, dsc, dsh, dw))
    assert all(_same_bits(a, b) for a, b in zip(*outs)), "modnorm backward not reproducible"
    dx, dsc, dsh, dw = outs[0]
    xd, wd, scd, gd = x.double(), w.double(), sc.double(), g.double()
    leaves = [t.clone().requires_grad_(True) for t in (xd, wd, scd)]
    R.modnorm(leaves[0], leaves[1], leaves[2], torch.zeros_like(xd)).backward(gd)
    r = torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + R.EPS)
    xh, wb = xd * r, wd.reshape(1, -1, 1, 1, 1)
    dn = gd * (1 + scd)
    er = (Cc + 5) * U
    E = (2 * Cc + 12) * U
    _within("dx", _out_cb8(dx, Cc, "dx"), leaves[0].grad, 2 * E * r * ((dn * wb).abs() + xh.abs() * (dn * wb * xh).abs().mean(1, keepdim=True)))
    _within("dscale", _out_cb8(dsc, Cc, "dscale"), leaves[2].grad, (er + 3 * U) * leaves[2].grad.abs())
    _equal("dshift", _out_cb8(dsh, Cc, "dshift"), gd)
    nwg = (N * Z * S * S + 63) // 64
    _within("dw", dw, leaves[1].grad, (er + (R.depth_two_stage(nwg) + 3) * U) * (dn * xh).abs().sum((0, 2, 3, 4)))


# ================================================================================================================= resample
# (N, C, Z, S_out, mode): nearest x2 (1) and AvgPool(1,2,2) (2), S_out 2 / 4 / 32 / 64, Z 1-4
RESAMPLE_CASES = [(2, 13, 1, 2, 1), (1, 229, 2, 4, 1), (3, 13, 3, 32, 1), (1, 229, 4, 64, 1),
                  (2, 13, 1, 2, 2), (1, 229, 2, 4, 2), (3, 13, 3, 32, 2), (1, 229, 4, 64, 2), (2, 13, 2, 64, 2)]


@pytest.mark.parametrize("N,Cc,Z,So,mode", RESAMPLE_CASES)
def test_resample_exact_integers(N, Cc, Z, So, mode):
    Si = So // 2 if mode == 1 else 2 * So
    x = util.rand_int((N, Cc, Z, Si, Si), -3, 3, 91)
    xc = util.to_cb8(x.to(DEV))
    outs = []
    for _ in range(2):
        y = _nan_cb8(N, Cc, Z, So)
        _lib.check(_lib.lib().tm_op_resample(_lib.ptr(xc), _lib.ptr(y), N, Cc, Z, So, mode, _st()), "tm_op_resample")
        outs.append(y)
    assert _same_bits(outs[0], outs[1])
    ref = tc.up2_hw(x.double()) if mode == 1 else tc.down2_hw(x.double())
    _equal("y", _out_cb8(outs[0], Cc, "y"), ref)


# ================================================================================================================= attention core
# (N, C, Z, S): windows of T = Z (S/2)^2 = 32, 64, 128 tokens; C off the 16-channel staging chunk (8, 13, 40) and the widths
# of the default model (256 at T = 128, 512 at T = 32)
ATTN_CASES = [(2, 8, 2, 8), (1, 13, 4, 8), (1, 40, 2, 16), (2, 64, 1, 16), (1, 256, 2, 16), (1, 512, 2, 8), (1, 13, 2, 16), (1, 40, 2, 8)]


@pytest.mark.parametrize("N,Cc,Z,S", ATTN_CASES)
def test_window_attn_train(N, Cc, Z, S):
    """Bounds from the accumulation lengths: a logit is a C-term sum of operands that carry rstd (<= (C + 5) U) and two
    staging roundings: |dl| <= (3 C + 20) U max_l, max_l = max sum_c |qh kh| / C.  The probabilities then carry
    e_P = 2 |dl| + (2 max_l + T + 8) U (exp argument, R.exp_rel_bound, T-term sum, division).  o and dv are T-term sums of P times
    data: (e_P + (T + 2) U) times their magnitude.  dq, dk and the norm weight gradients chain dP (C terms), the row dot (T),
    dS, dqh (T), the RMSNorm backward (C) and the (token, workgroup) sums: 2 (e_P + (2 C + 3 T + depth + 40) U) times their
    magnitude (train_op_ref.window_attn_mag: the same sums over |terms|)."""
    T = Z * (S // 2) ** 2
    q, k, v, d = (_randn((N, Cc, Z, S, S), 100 + i) for i in range(4))
    qw, kw = torch.rand(Cc, generator=_gen(105)) + 0.5, torch.rand(Cc, generator=_gen(106)) + 0.5
    qc, kc, vc, dc = (util.to_cb8(t.to(DEV)) for t in (q, k, v, d))
    fwd, bwd = [], []
    for _ in range(2):
        o = _nan_cb8(N, Cc, Z, S)
        _lib.check(_lib.lib().tm_op_window_attn_train(_lib.ptr(qc), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(qw), _lib.ptr(kw), None, _lib.ptr(o),
                                                      None, None, None, None, None, N, Cc, Z, S, _st()), "tm_op_window_attn_train")
        fwd.append(o)
        dq, dk, dv = _nan_cb8(N, Cc, Z, S), _nan_cb8(N, Cc, Z, S), _nan_cb8(N, Cc, Z, S)
        dqw, dkw = torch.full((Cc,), NAN), torch.full((Cc,), NAN)
        _lib.check(_lib.lib().tm_op_window_attn_train(_lib.ptr(qc), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(qw), _lib.ptr(kw), _lib.ptr(dc),
                                                      None, _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(dqw), _lib.ptr(dkw), N, Cc, Z,
                                                      S, _st()), "tm_op_window_attn_train")
        bwd.append((dq, dk, dv, dqw, dkw))
    assert _same_bits(fwd[0], fwd[1]) and all(_same_bits(a, b) for a, b in zip(*bwd)), "attention core not reproducible"
    leaves = [t.double().clone().requires_grad_(True) for t in (q, k, v, qw, kw)]
    ref = R.window_attn(*leaves, Z, S)
    ref.backward(d.double())
    mag, lmax = R.window_attn_mag(*(t.double() for t in (q, k, v, qw, kw, d)), Z, S)
    dl = (3 * Cc + 20) * U * lmax
    eP = 2 * dl + (2 * lmax + T + 8) * U
    Eb = 2 * (eP + (2 * Cc + 3 * T + R.depth_two_stage(4 * N) + 40) * U)
    _within("o", _out_cb8(fwd[0], Cc, "o"), ref.detach(), (eP + (T + 2) * U) * mag["o"])
    dq, dk, dv, dqw, dkw = bwd[0]
    _within("dv", _out_cb8(dv, Cc, "dv"), leaves[2].grad, (eP + (T + 2) * U) * mag["dv"])
    _within("dq", _out_cb8(dq, Cc, "dq"), leaves[0].grad, Eb * mag["dq"])
    _within("dk", _out_cb8(dk, Cc, "dk"), leaves[1].grad, Eb * mag["dk"])
    _within("dqw", dqw, leaves[3].grad, Eb * mag["dqw"])
    _within("dkw", dkw, leaves[4].grad, Eb * mag["dkw"])


# ================================================================================================================= ResBlock prep
# (N, per_image, Z, S, C): per_image Z S^2 = 96 or 80 voxels (>= 64, not a multiple of 64), so workgroups of 64 voxels straddle
# two images and prep_bwd_reduce_mod_kernel takes their second slab; N = 7 is not a multiple of per_image (a partial image).
# The hooks refuse per_image Z S^2 < 64 (a workgroup could then span three images).
PREP_CASES = [(6, 3, 2, 4, 13, True), (5, 5, 1, 4, 40, False), (7, 3, 2, 4, 64, True), (3, 1, 2, 8, 229, True)]


def _prep_inputs(N, per_image, Z, S, Cc, drop):
    nimg = (N + per_image - 1) // per_image
    x = _randn((N, Cc, Z, S, S), 111)
    w = torch.rand(Cc, generator=_gen(112)) + 0.5
    sc, sh = _randn((nimg, Cc), 113, 0.3), _randn((nimg, Cc), 114, 0.3)
    mask = (torch.rand((N, Cc, Z, S, S), generator=_gen(115)) > 0.1).float() if drop else None
    return x, w, sc, sh, mask


def _prep_train(x, w, sc, sh, mask, per_image):
    N, Cc, Z, S, _ = x.shape
    xc, mc = util.to_cb8(x.to(DEV)), (None if mask is None else util.to_cb8(mask.to(DEV)))
    ds = float(1.0 / torch.tensor(0.9, dtype=torch.float32)) if mask is not None else 1.0
    outs = []
    for _ in range(2):
        y = _nan_cb8(N, Cc, Z, S)
        _lib.check(_lib.lib().tm_op_prep_train(_lib.ptr(xc), _lib.ptr(w), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(mc), ds, per_image, _lib.ptr(y),
                                               N, Cc, Z, S, _st()), "tm_op_prep_train")
        outs.append(y)
    assert _same_bits(outs[0], outs[1])
    return _out_cb8(outs[0], Cc, "y"), ds


@pytest.mark.parametrize("N,per_image,Z,S,Cc,drop", PREP_CASES)
def test_prep_train_silu_within_the_hw_approximation_bound(N, per_image, Z, S, Cc, drop, out_dir):
    """prep_kernel computes SiLU in fp32 on v_exp_f32 / v_rcp_f32 (silu_h16), not libm expf: the output is held to
    train_op_ref.silu_hw_rel_bound (derived from their 1-ulp accuracy) on top of the error of the pre-activation m
    (|silu'| <= 1.1 times |dm|, dm <= (C + 10) U |xh w (1 + s)| + U |m|).  The worst |d| / bound is written to the output directory."""
    x, w, sc, sh, mask = _prep_inputs(N, per_image, Z, S, Cc, drop)
    y, ds = _prep_train(x, w, sc, sh, mask, per_image)
    xd = x.double()
    ref, m = R.prep_train(xd, w.double(), sc.double(), sh.double(), per_image, None if mask is None else mask.double(), 1 - 1 / ds)
    img = torch.arange(N) // per_image
    nmod = (tc.rms_norm_channels(xd, w.double()) * (1 + sc.double()[img][:, :, None, None, None])).abs()
    dm = (Cc + 10) * U * nmod + U * m.abs()
    keep = torch.ones_like(m) if mask is None else mask.double() * ds
    bound = keep * (R.silu_hw_rel_bound(m) * R.silu(m).abs() + 1.1 * dm) + U * ref.abs() + R.FLT_MIN
    _within("y", y, ref, bound)
    hw = keep * R.silu_hw_rel_bound(m) * R.silu(m).abs()
    worst = float(((y - ref).abs() / bound).max())
    with open(f"{out_dir}/prep_train_silu_err.txt", "a") as f:
        f.write(f"N={N} per_image={per_image} Z={Z} S={S} C={Cc} drop={drop}: max|d|={float((y - ref).abs().max()):.3e}, "
                f"worst |d|/bound={worst:.3f}, largest silu_hw term {float(hw.max()):.3e}\n")


@pytest.mark.parametrize("N,per_image,Z,S,Cc,drop", PREP_CASES)
def test_prep_bwd_straddling_images(N, per_image, Z, S, Cc, drop):
    """float64 autograd of the forward above.  Per element, every factor of dm = ds sg (1 + m (1 - sg)) is within
    E = (C + 16 + 2 max|m|) U of its value (rstd (C + 5), expf by R.exp_rel_bound, the products), and m's own error moves dm by at most
    |ds| |silu''| |dm| <= 0.5 |ds| E (|n (1 + s)| + |sh|): dm_mag = |ds| (sg (1 + |m| (1 - sg)) + 0.5 (|n (1 + s)| + |sh|)).
    dx: 2 E r (dm_mag |1 + s| |w| + |xh| mean_c(...)).  dw, dscale, dshift: sums over voxels through 64-lane sums and the
    workgroup partials (R.depth_two_stage)."""
    x, w, sc, sh, mask = _prep_inputs(N, per_image, Z, S, Cc, drop)
    g = _randn((N, Cc, Z, S, S), 116)
    xc, gc = util.to_cb8(x.to(DEV)), util.to_cb8(g.to(DEV))
    mc = None if mask is None else util.to_cb8(mask.to(DEV))
    ds = float(1.0 / torch.tensor(0.9, dtype=torch.float32)) if mask is not None else 1.0
    nimg = sc.shape[0]
    outs = []
    for _ in range(2):
        dx = _nan_cb8(N, Cc, Z, S)
        dw, dsc, dsh = torch.full((Cc,), NAN), torch.full((nimg, Cc), NAN), torch.full((nimg, Cc), NAN)
        _lib.check(_lib.lib().tm_op_prep_bwd(_lib.ptr(xc), _lib.ptr(gc), _lib.ptr(w), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(mc), ds, per_image,
                                             _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(dsc), _lib.ptr(dsh), N, Cc, Z, S, _st()), "tm_op_prep_bwd")
        outs.append((dx, dw, dsc, dsh))
    assert all(_same_bits(a, b) for a, b in zip(*outs)), "prep backward not reproducible"
    dx, dw, dsc, dsh = outs[0]
    xd, wd, scd, shd, gd = x.double(), w.double(), sc.double(), sh.double(), g.double()
    leaves = [t.clone().requires_grad_(True) for t in (xd, wd, scd, shd)]
    y, m = R.prep_train(*leaves, per_image, None if mask is None else mask.double(), 1 - 1 / ds)
    y.backward(gd)
    img = torch.arange(N) // per_image
    s5, h5 = scd[img][:, :, None, None, None], shd[img][:, :, None, None, None]
    r = torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + R.EPS)
    xh, wb = xd * r, wd.reshape(1, -1, 1, 1, 1)
    n = xh * wb
    m = m.detach()
    sg = torch.sigmoid(m)
    dsv = (gd * (1.0 if mask is None else mask.double() * ds)).abs()
    dm_mag = dsv * (sg * (1 + m.abs() * (1 - sg)) + 0.5 * ((n * (1 + s5)).abs() + h5.abs()))
    E = (Cc + 16 + 2 * float(m.abs().max())) * U
    t = dm_mag * (1 + s5).abs() * wb.abs()
    _within("dx", _out_cb8(dx, Cc, "dx"), leaves[0].grad, 2 * E * r * (t + xh.abs() * (t * xh.abs()).mean(1, keepdim=True)))
    nwg = (N * Z * S * S + 63) // 64
    _within("dw", dw, leaves[1].grad, (2 * E + R.depth_two_stage(nwg) * U) * (dm_mag * (1 + s5).abs() * xh.abs()).sum((0, 2, 3, 4)))
    per_img = lambda t: torch.zeros(nimg, Cc, dtype=torch.float64).index_add_(0, img, t.sum((2, 3, 4)))
    Ei = 2 * E + R.depth_two_stage((per_image * Z * S * S) // 64 + 2) * U
    _within("dscale", dsc, leaves[2].grad, Ei * per_img(dm_mag * n.abs()))
    _within("dshift", dsh, leaves[3].grad, Ei * per_img(dm_mag))


def test_prep_bwd_rejects_images_below_one_workgroup():
    """per_image Z S^2 < 64: a workgroup of 64 voxels could span three images; the backward refuses such a geometry."""
    N, Cc, Z, S = 4, 8, 1, 4
    z = torch.zeros((N, 1, Z, S, S, 8), device=DEV)
    host = torch.zeros(Cc)
    rc = _lib.lib().tm_op_prep_bwd(_lib.ptr(z), _lib.ptr(z), _lib.ptr(host), _lib.ptr(torch.zeros(N, Cc)), _lib.ptr(torch.zeros(N, Cc)),
                                   None, 1.0, 1, _lib.ptr(torch.empty_like(z)), _lib.ptr(torch.empty(Cc)), _lib.ptr(torch.empty(N, Cc)),
                                   _lib.ptr(torch.empty(N, Cc)), N, Cc, Z, S, _st())
    assert rc != 0


# ================================================================================================================= optimizer
@pytest.mark.parametrize("n", [1, 255, 257, 262144, 30_000_000])
def test_sumsq(n):
    """nwg = min(1024, ceil(n / 256)) workgroups; a thread chains ceil(n / (256 nwg)) fmas, then a 64-lane tree (6), 4
    partials (2) and the partials in 8 chains (R.depth_two_stage without its wave part): |err| <= L U sum x^2."""
    gen = torch.Generator(device=DEV).manual_seed(121)
    x = torch.randn(n, generator=gen, device=DEV)
    outs = []
    for _ in range(2):
        o = C.c_float(NAN)
        _lib.check(_lib.lib().tm_op_sumsq(_lib.ptr(x), n, C.byref(o), _st()), "tm_op_sumsq")
        outs.append(o.value)
    assert outs[0] == outs[1] or (math.isnan(outs[0]) and math.isnan(outs[1]))
    ref = float(x.cpu().double().pow(2).sum())
    nwg = min(1024, (n + 255) // 256)
    L = -(-n // (256 * nwg)) + 6 + 2 + (nwg + 7) // 8 + 3
    assert abs(outs[0] - ref) <= L * U * ref, (outs[0], ref)


@pytest.mark.parametrize("n,step,wd,gscale", [(1, 1, 0.0, 1.0), (100003, 1, 0.01, 0.37), (257, 1000, 0.05, 1.7), (100003, 1000, 0.01, 0.37)])
def test_adam(n, step, wd, gscale):
    """One step against the float64 formula.  Roundings: g' (2 U of |g gs| + |wd p|), m' and v' (3 / 4 U of their terms), powf
    2 ulp in the bias corrections, then the quotient (a handful of U relative, plus m' and v' errors carried through)."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p, g = _randn((n,), 131), _randn((n,), 132)
    m0 = _randn((n,), 133, 0.1) if step > 1 else torch.zeros(n)
    v0 = torch.rand(n, generator=_gen(134)) * 0.01 if step > 1 else torch.zeros(n)
    outs = []
    for _ in range(2):
        pd, gd, md, vd = p.to(DEV), g.to(DEV), m0.to(DEV), v0.to(DEV)
        _lib.check(_lib.lib().tm_op_adam(_lib.ptr(pd), _lib.ptr(gd), _lib.ptr(md), _lib.ptr(vd), n, lr, b1, b2, eps, wd, step, gscale, _st()),
                   "tm_op_adam")
        outs.append([t.cpu() for t in (pd, md, vd)])
    assert all(_same_bits(a, b) for a, b in zip(*outs)), "adam not reproducible"
    gp, gm, gv = outs[0]
    pd, gd, md, vd = p.double(), g.double(), m0.double(), v0.double()
    p2, m2, v2, g2, upd = R.adam(pd, gd, md, vd, lr, b1, b2, eps, wd, step, gscale)
    f = lambda a: float(torch.tensor(a, dtype=torch.float32))
    lr32, b1_32, b2_32, eps32, gs32, wd32 = map(f, (lr, b1, b2, eps, gscale, wd))
    dg = 2 * U * ((gd * gs32).abs() + (wd32 * pd).abs())
    dm = (1 - b1_32) * dg + 3 * U * (md.abs() + g2.abs())
    dv = 4 * U * v2 + 2 * (1 - b2_32) * g2.abs() * dg
    _within("m", gm, m2, dm + 1e-45)
    _within("v", gv, v2, dv + 1e-45)
    bc1, bc2 = 1 - b1_32 ** step, 1 - b2_32 ** step
    e1 = (4 * U * b1_32 ** step + U * bc1) / bc1
    e2 = (4 * U * b2_32 ** step + U * bc2) / bc2
    sq = torch.sqrt(v2) / math.sqrt(bc2)
    den = sq + eps32
    rel_den = (dv / (2 * v2).clamp_min(1e-300) + e2 / 2 + 3 * U) * sq / den + U
    dupd = upd.abs() * (e1 + 3 * U + rel_den) + (lr32 / bc1) * dm / den
    _within("p", gp, p2, dupd + U * p2.abs())
