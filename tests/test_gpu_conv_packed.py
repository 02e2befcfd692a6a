"""-m gpu: conv weights packed on the device (tm_op_conv_pack_dev) and the conv ops that run on a ready pack
(tm_op_conv_mfma_packed, tm_op_conv_dgrad_packed).  The criterion is bit equality with the host-weight entry points
(tm_op_conv_mfma, tm_op_conv_dgrad) on random normal data: the same kernel reads the pack, so equal output bits for every
input means the pack bytes are the ones conv_pack_host writes for the plain and the pair form."""
import pytest
import torch

import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _st():
    return _lib.current_stream_ptr()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pack(w_dev, Cout, Cin, ksize, Z, role):
    n = _lib.lib().tm_conv_pack_floats(Cout, Cin, ksize, Z, role)
    assert n > 0
    pk = torch.full((n,), NAN, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().tm_op_conv_pack_dev(_lib.ptr(w_dev), _lib.ptr(pk), Cout, Cin, ksize, Z, role, _st()), "tm_op_conv_pack_dev")
    return pk


def _nan_cb8(N, Cc, Z, S):
    return torch.full((N, (Cc + 7) // 8, Z, S, S, 8), NAN, dtype=torch.float32, device=DEV)


def _fwd_host(xc, w, b, N, Cin, Cout, Z, S, ksize):
    y = _nan_cb8(N, Cout, Z, S)
    _lib.check(_lib.lib().tm_op_conv_mfma(_lib.ptr(xc), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), N, Cin, Cout, Z, S, ksize, 0, 0, 0, _st()),
               "tm_op_conv_mfma")
    return y


def _fwd_packed(xc, pk, b_dev, N, Cin, Cout, Z, S, ksize):
    y = _nan_cb8(N, Cout, Z, S)
    _lib.check(_lib.lib().tm_op_conv_mfma_packed(_lib.ptr(xc), _lib.ptr(pk), _lib.ptr(b_dev), _lib.ptr(y), N, Cin, Cout, Z, S, ksize, _st()),
               "tm_op_conv_mfma_packed")
    torch.cuda.synchronize()
    return y


# (N, Cin, Cout, Z, S, ksize): ksize 3 at Z = 1, 2 (pair form), 3, 4 and ksize 1; Cin in {13, 229, 256, 1253}, Cout in {1, 40, 64, 512}
CASES = [(2, 13, 40, 1, 8, 3), (1, 229, 64, 2, 8, 3), (2, 256, 1, 2, 16, 3), (1, 1253, 512, 2, 8, 3), (1, 13, 64, 3, 8, 3),
         (1, 229, 40, 4, 4, 3), (2, 256, 512, 2, 8, 1), (1, 1253, 40, 4, 8, 1), (1, 13, 1, 1, 16, 1), (1, 256, 64, 3, 16, 3)]


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize", CASES)
def test_packed_forward_equals_host_weights(N, Cin, Cout, Z, S, ksize):
    g = torch.Generator().manual_seed(7 * Cin + Cout)
    k = ksize
    x = torch.randn((N, Cin, Z, S, S), generator=g)
    w = torch.randn((Cout, Cin, k, k, k), generator=g).contiguous()
    b = torch.randn((Cout,), generator=g)
    xc = util.to_cb8(x.to(DEV))
    ref = _fwd_host(xc, w, b, N, Cin, Cout, Z, S, ksize)
    pk = _pack(w.to(DEV), Cout, Cin, ksize, Z, 0)
    assert not torch.isnan(pk).any(), "pack not fully written"
    got = _fwd_packed(xc, pk, b.to(DEV), N, Cin, Cout, Z, S, ksize)
    assert not torch.isnan(got).any()
    assert _same_bits(got, ref), f"packed forward differs: max|d| = {float((got - ref).abs().max()):.3e}"


@pytest.mark.parametrize("N,Cin,Cout,Z,S,ksize", CASES)
def test_packed_dgrad_equals_host_weights(N, Cin, Cout, Z, S, ksize):
    g = torch.Generator().manual_seed(11 * Cin + Cout)
    k = ksize
    dy = torch.randn((N, Cout, Z, S, S), generator=g)
    w = torch.randn((Cout, Cin, k, k, k), generator=g).contiguous()
    yc = util.to_cb8(dy.to(DEV))
    ref = _nan_cb8(N, Cin, Z, S)
    _lib.check(_lib.lib().tm_op_conv_dgrad(_lib.ptr(yc), _lib.ptr(w), _lib.ptr(ref), N, Cin, Cout, Z, S, ksize, _st()), "tm_op_conv_dgrad")
    pk = _pack(w.to(DEV), Cout, Cin, ksize, Z, 1)
    assert not torch.isnan(pk).any(), "pack not fully written"
    got = _nan_cb8(N, Cin, Z, S)
    _lib.check(_lib.lib().tm_op_conv_dgrad_packed(_lib.ptr(yc), _lib.ptr(pk), _lib.ptr(got), N, Cin, Cout, Z, S, ksize, _st()),
               "tm_op_conv_dgrad_packed")
    torch.cuda.synchronize()
    assert not torch.isnan(got).any()
    assert _same_bits(got, ref), f"packed dgrad differs: max|d| = {float((got - ref).abs().max()):.3e}"


def test_repack_after_weight_change():
    """The library keeps no pack of its own: after the device weight changes in place, a new tm_op_conv_pack_dev gives the new result."""
    N, Cin, Cout, Z, S = 1, 40, 40, 2, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn((N, Cin, Z, S, S), generator=g)
    w1, w2 = torch.randn((Cout, Cin, 3, 3, 3), generator=g), torch.randn((Cout, Cin, 3, 3, 3), generator=g)
    b = torch.randn((Cout,), generator=g)
    xc, bd = util.to_cb8(x.to(DEV)), b.to(DEV)
    wd = w1.to(DEV).contiguous()
    pk = _pack(wd, Cout, Cin, 3, Z, 0)
    y1 = _fwd_packed(xc, pk, bd, N, Cin, Cout, Z, S, 3)
    wd.copy_(w2.to(DEV))
    y_stale = _fwd_packed(xc, pk, bd, N, Cin, Cout, Z, S, 3)
    assert _same_bits(y_stale, y1), "the op must read the pack it is given, not the weight"
    pk2 = _pack(wd, Cout, Cin, 3, Z, 0)
    y2 = _fwd_packed(xc, pk2, bd, N, Cin, Cout, Z, S, 3)
    assert _same_bits(y1, _fwd_host(xc, w1.contiguous(), b, N, Cin, Cout, Z, S, 3))
    assert _same_bits(y2, _fwd_host(xc, w2.contiguous(), b, N, Cin, Cout, Z, S, 3))
    assert not _same_bits(y1, y2)


def test_packed_error_paths():
    L = _lib.lib()
    t = torch.zeros(4096, device=DEV)
    p = _lib.ptr(t)
    assert L.tm_conv_pack_floats(8, 8, 2, 2, 0) == -1 and L.tm_conv_pack_floats(8, 8, 3, 2, 2) == -1
    assert L.tm_conv_pack_floats(64, 8, 3, 2, 0) == 27 * 512 and L.tm_conv_pack_floats(64, 8, 3, 2, 1) == 8 * 27 * 512
    assert L.tm_op_conv_pack_dev(None, p, 8, 8, 3, 2, 0, _st()) == -1 and b"null" in L.tm_last_error()
    assert L.tm_op_conv_pack_dev(p, p, 8, 8, 5, 2, 0, _st()) == -1 and b"ksize" in L.tm_last_error()
    assert L.tm_op_conv_mfma_packed(p, p, None, p, 1, 8, 8, 2, 4, 3, _st()) == -1
    assert L.tm_op_conv_mfma_packed(p, p, p, p, 1, 8, 8, 5, 4, 3, _st()) == -1 and b"Z" in L.tm_last_error()
    assert L.tm_op_conv_dgrad_packed(p, None, p, 1, 8, 8, 2, 4, 3, _st()) == -1
    assert L.tm_op_conv_dgrad_packed(p, p, p, 1, 8, 8, 2, 4, 4, _st()) == -1
