"""GPU: tm_op_rank_sum, the only arithmetic of the data-parallel gradient exchange (teramind_amd.train_dist), against sequential
torch adds on the host -- IEEE fp32 additions in slice order, starting from slice 0's value.  Every comparison is bit for bit
(int32 views, torch.equal) and `out` is NaN-prefilled, so an element the kernel never wrote shows.

Shapes: n = 1, 3 run the scalar tail alone; 1023, 4100 and 65 536 + 5 a vector body, then a tail of 3, 0 and 1 (and, for W > 1,
slices that start off a 16-byte boundary); W = 16 is two load groups of eight, W = 3 a single short one.  The grid is sized to the
chip (8 workgroups of 256 threads per compute unit, four floats per thread), so only n > 8 * 256 * 4 * CUs makes a thread take a
second pass of the grid-stride loop: GRID_WRAP_N does on a chip of up to 304 compute units."""
import ctypes as C

import pytest
import torch

from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
WS, NS = (1, 2, 3, 8, 16), (1, 3, 1023, 4100, 65536 + 5)
GRID_WRAP_N = 2 * 304 * 8 * 256 * 4 + 5


def _st():
    return _lib.current_stream_ptr()


def make_parts(W, n, seed=0):
    """Standard normals times 2^k, k in [-8, 8]: sums that round, and round differently in a different order; a few -0.0."""
    g = torch.Generator().manual_seed(77 * W + n % 1000 + seed)
    x = torch.randn(W, n, generator=g) * torch.exp2(torch.randint(-8, 9, (W, n), generator=g).float())
    x[:, 0] = -0.0
    return x


def sequential(parts, order=None):
    order = range(parts.shape[0]) if order is None else order
    acc = None
    for k in order:
        acc = parts[k].clone() if acc is None else acc + parts[k]
    return acc


def rank_sum(parts_dev, out_dev, W, n):
    rc = _lib.lib().tm_op_rank_sum(_lib.ptr(parts_dev), _lib.ptr(out_dev), W, n, _st())
    torch.cuda.synchronize()
    return rc


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("W", WS)
def test_rank_sum_equals_sequential_adds(W, n):
    parts = make_parts(W, n)
    want = sequential(parts)
    if W >= 3 and n >= 1023:                                      # otherwise the case proves nothing about order (n = 1, 3: too few sums to tell)
        assert not torch.equal(bits(sequential(parts, reversed(range(W)))), bits(want)), "the inputs do not tell the orders apart"
    d = parts.to(DEV)
    off = 1 if n == 1023 else 4                                   # 1: `out` itself off a 16-byte boundary
    out = torch.full((n + 8,), NAN, device=DEV)
    assert rank_sum(d, out[off:off + n], W, n) == 0
    assert torch.equal(bits(out[off:off + n]), bits(want))
    assert torch.isnan(out[:off]).all() and torch.isnan(out[off + n:]).all()      # nothing outside [0, n) is written
    again = torch.full((n,), NAN, device=DEV)
    assert rank_sum(d, again, W, n) == 0
    assert torch.equal(bits(again), bits(out[off:off + n]))       # two calls give the same bits
    assert torch.equal(bits(d), bits(parts))                      # the slices are read only


def test_more_elements_than_one_grid_pass():
    W, n = 3, GRID_WRAP_N
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n // 4 > 8 * 256 * cus, "raise GRID_WRAP_N: this chip's grid covers it in one pass"
    parts = make_parts(W, n)
    want = sequential(parts)
    assert not torch.equal(bits(sequential(parts, (2, 1, 0))), bits(want))
    out = torch.full((n,), NAN, device=DEV)
    assert rank_sum(parts.to(DEV), out, W, n) == 0
    assert torch.equal(bits(out), bits(want))


def test_one_slice_is_a_bit_copy():
    """W = 1 starts from slice 0's value and adds nothing: -0.0, denormals, infinities and NaN payloads pass unchanged."""
    pat = torch.tensor([-0.0, 0.0, 1e-45, -1e-45, 1.17549421e-38, -5.87747175e-39, float("inf"), float("-inf"), 1.0, -3.5])
    for n in (3, 10, 4100):
        src = pat.repeat((n + 9) // 10)[:n].clone().view(torch.int32)
        if n > 8:
            src[7] = 0x7FC01234                                     # a NaN with a payload
        d = src.view(torch.float32).reshape(1, n).to(DEV)
        out = torch.full((n,), NAN, device=DEV)
        assert rank_sum(d, out, 1, n) == 0
        assert torch.equal(bits(out), src)
    # and the first add of W = 2 is slice 0 + slice 1, not 0 + slice 0 + slice 1: -0.0 + -0.0 keeps its sign
    d = torch.full((2, 5), -0.0, device=DEV)
    out = torch.full((5,), NAN, device=DEV)
    assert rank_sum(d, out, 2, 5) == 0
    assert (bits(out) == torch.tensor(-0.0).view(torch.int32)).all()


def test_empty_sum_writes_nothing():
    d = torch.ones(2, 8, device=DEV)
    out = torch.full((8,), NAN, device=DEV)
    assert rank_sum(d, out, 2, 0) == 0
    assert torch.isnan(out).all()


def test_error_paths_return_before_any_launch():
    L = _lib.lib()
    n = 64
    buf = torch.ones(4 * n, device=DEV)
    out = torch.full((n,), NAN, device=DEV)
    p, o, st = _lib.ptr(buf), _lib.ptr(out), _st()

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == -1 and word in L.tm_last_error(), L.tm_last_error()
        assert torch.isnan(out).all()

    refused(L.tm_op_rank_sum(p, o, 0, n, st), b"W = 0")
    refused(L.tm_op_rank_sum(p, o, 65, n, st), b"W = 65")
    refused(L.tm_op_rank_sum(None, o, 2, n, st), b"null")
    refused(L.tm_op_rank_sum(p, None, 2, n, st), b"null")
    refused(L.tm_op_rank_sum(p, o, 2, -1, st), b"n = -1")
    # overlapping ranges (floats): out inside parts; out ending on parts' first float; out starting on parts' last float
    both = torch.full((5 * n,), NAN, device=DEV)
    base = both.data_ptr()
    at = lambda i: C.c_void_p(base + 4 * i)                                          # noqa: E731
    for parts_at, W, out_at in ((0, 4, n), (n, 3, 1), (0, 4, 4 * n - 1)):
        rc = L.tm_op_rank_sum(at(parts_at), at(out_at), W, n, st)
        torch.cuda.synchronize()
        assert rc == -1 and b"overlap" in L.tm_last_error()
    assert torch.isnan(both).all() and torch.isnan(out).all()
    # out directly behind parts is not an overlap
    assert L.tm_op_rank_sum(C.c_void_p(base), C.c_void_p(base + 4 * 4 * n), 4, n, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(both).all()                                # NaN + NaN: written, and still NaN -- only the call's success is asserted
    ms = C.c_float(0)
    assert L.tm_op_rank_sum_time(0, n, 1, 1, C.byref(ms), st) == -1
    assert L.tm_op_rank_sum_time(2, 0, 1, 1, C.byref(ms), st) == -1
    assert L.tm_op_rank_sum_time(2, n, 1, 1, None, st) == -1
