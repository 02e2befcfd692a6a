"""-m gpu: tm_u8_shrink2 (one pyramid level from the one above) against the numpy 2 x 2 rule, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from teramind_amd import _lib, ometiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def shrink2_ref(a):
    """(a + b + c + d + 2) >> 2 over 2 x 2 blocks, an odd last row / column repeated."""
    h, w = a.shape
    ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    b = a[np.ix_(ys, xs)].astype(np.int32)
    return ((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def _img(h, w, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    a[0, 0], a[-1, -1] = 255, 255                # the sums reach 4 * 255 + 2 somewhere when a block is all 255
    if h > 1 and w > 1:
        a[:2, :2] = 255
    return a


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (255, 257), (600, 520)])
def test_shrink2_equals_the_numpy_rule(h, w):
    a = _img(h, w, h * 1000 + w)
    got = ometiff.shrink2(torch.from_numpy(a).to(DEV))
    assert got.shape == ((h + 1) // 2, (w + 1) // 2)
    assert torch.equal(got.cpu(), torch.from_numpy(shrink2_ref(a)))


@pytest.mark.parametrize("h,w,sp,dp,soff,doff", [(600, 520, 544, 272, 0, 0),       # 16-byte loads, 8-byte stores, pitched
                                                 (255, 257, 300, 131, 0, 0),       # pitches that break the alignment
                                                 (37, 70, 80, 40, 3, 5)])          # aligned pitches, unaligned base pointers
def test_shrink2_pitched_leaves_the_rest_of_the_destination_alone(h, w, sp, dp, soff, doff):
    a = _img(h, w, 7)
    hd, wd = (h + 1) // 2, (w + 1) // 2
    src = torch.full((h * sp + soff + 16,), 9, dtype=torch.uint8, device=DEV)
    src[soff:soff + h * sp].view(h, sp)[:, :w] = torch.from_numpy(a).to(DEV)
    dst = torch.full((hd * dp + doff + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().tm_u8_shrink2(C.c_void_p(src.data_ptr() + soff), h, w, sp, C.c_void_p(dst.data_ptr() + doff), dp,
                                        _lib.current_stream_ptr()), "tm_u8_shrink2")
    want = torch.full_like(dst, 0xA5).cpu()
    want[doff:doff + hd * dp].view(hd, dp)[:, :wd] = torch.from_numpy(shrink2_ref(a))
    assert torch.equal(dst.cpu(), want)


def test_build_pyramid_levels():
    a = _img(600, 520, 11)
    levels = ometiff.build_pyramid(torch.from_numpy(a).to(DEV))
    assert [tuple(p.shape) for p in levels] == [(600, 520), (300, 260), (150, 130)]
    ref = a
    for p in levels[1:]:
        ref = shrink2_ref(ref)
        assert torch.equal(p.cpu(), torch.from_numpy(ref))
