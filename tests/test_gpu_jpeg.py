"""-m gpu: tm_jpeg_encode_tiles against the numpy restatement of baseline JPEG (jpeg_cases.py, itself held to libjpeg's
bytes by test_jpeg_cases_host.py): every tile's bytes and length, exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


def encode(plane, H, W, pitch, quality, tile0, ntiles, slot_bytes, compact=True, extra_slots=1):
    """-> (slots [ntiles + extra][slot_bytes], need [ntiles], packed bytes or None, offsets or None), host arrays.  Every
    output buffer is prefilled with FILL / -1."""
    slots = torch.full(((ntiles + extra_slots) * slot_bytes,), FILL, dtype=torch.uint8, device=DEV)
    need = torch.full((ntiles + 1,), -1, dtype=torch.int32, device=DEV)
    packed = torch.full((ntiles * slot_bytes + 64,), FILL, dtype=torch.uint8, device=DEV) if compact else None
    offsets = torch.full((ntiles + 2,), -1, dtype=torch.int64, device=DEV) if compact else None
    _lib.check(_lib.lib().tm_jpeg_encode_tiles(C.c_void_p(plane.data_ptr()), H, W, pitch, quality, tile0, ntiles,
                                               _lib.ptr(slots), slot_bytes, _lib.ptr(need), _lib.ptr(packed), _lib.ptr(offsets),
                                               _lib.current_stream_ptr()), "tm_jpeg_encode_tiles")
    torch.cuda.synchronize()
    assert int(need[ntiles]) == -1                                               # need[] has ntiles entries
    return (slots.cpu().numpy().reshape(ntiles + extra_slots, slot_bytes), need[:ntiles].cpu().numpy(),
            None if packed is None else packed.cpu().numpy(), None if offsets is None else offsets.cpu().numpy())


def check_tiles(slots, need, packed, offsets, want, slot_bytes):
    """Slot k holds exactly want[k] followed by its prefill; need[k] is its length; the packed copy is the scans back to back."""
    n = len(want)
    assert need.tolist() == [len(w) for w in want]
    for k, w in enumerate(want):
        assert slots[k, :len(w)].tobytes() == w, f"tile {k}: bytes differ"
        assert (slots[k, len(w):] == FILL).all(), f"tile {k}: wrote past its length"
    assert (slots[n:] == FILL).all(), "wrote a slot that is not in the range"
    if packed is not None:
        ends = np.cumsum([0] + [len(w) for w in want])
        assert offsets[:n + 1].tolist() == ends.tolist() and offsets[n + 1] == -1
        assert packed[:ends[-1]].tobytes() == b"".join(want)
        assert (packed[ends[-1]:] == FILL).all()


def slot_for(want):
    return max(len(w) for w in want) + 8


@pytest.mark.parametrize("quality", jc.QUALITIES)
@pytest.mark.parametrize("name", list(jc.CASES))
def test_tile_bytes_equal_the_restatement(name, quality):
    img = jc.image(name)
    H, W = img.shape
    want = jc.reference_scans(name, quality)
    assert len(want) == jc.grid_of(H, W)[0] * jc.grid_of(H, W)[1]
    plane = torch.from_numpy(img.copy()).to(DEV)
    sb = slot_for(want)
    check_tiles(*encode(plane, H, W, W, quality, 0, len(want), sb), want, sb)


def test_sub_range_writes_only_its_slots():
    img, q = jc.image("p264x520"), 75
    want = jc.reference_scans("p264x520", q)[2:5]
    plane = torch.from_numpy(img.copy()).to(DEV)
    sb = slot_for(want)
    check_tiles(*encode(plane, 264, 520, 520, q, 2, 3, sb, extra_slots=3), want, sb)


@pytest.mark.parametrize("pitch,off", [(528, 0), (523, 0), (520, 3)])        # aligned pitch, odd pitch, unaligned base
def test_pitched_plane_gives_the_bytes_of_the_contiguous_one(pitch, off):
    img, q = jc.image("p264x520"), 90
    want = jc.reference_scans("p264x520", q)
    buf = torch.full((264 * pitch + off + 16,), 77, dtype=torch.uint8, device=DEV)
    buf[off:off + 264 * pitch].view(264, pitch)[:, :520] = torch.from_numpy(img.copy()).to(DEV)
    sb = slot_for(want)
    check_tiles(*encode(buf[off:], 264, 520, pitch, q, 0, 6, sb), want, sb)


def test_slot_too_small_reports_need_and_keeps_the_prefill():
    img, q = jc.image("noise"), 75
    want = jc.reference_scans("noise", q)
    assert len(want[0]) > 16384
    plane = torch.from_numpy(img.copy()).to(DEV)
    slots, need, packed, offsets = encode(plane, 256, 256, 256, q, 0, 1, 16384)
    assert need.tolist() == [len(want[0])]
    assert (slots == FILL).all() and (packed == FILL).all()
    assert offsets[:2].tolist() == [0, 0]                                     # nothing packed for the slot that did not fit
    sb = int(need[0])                                                        # the second call: a slot of exactly that size
    check_tiles(*encode(plane, 256, 256, 256, q, 0, 1, sb), want, sb)


def test_mixed_batch_packs_only_the_filled_slots():
    """Six tiles, a slot size between the smallest and the largest scan: the small ones are written and packed, the rest only
    report their length."""
    img = np.array(jc.image("p264x520"))
    img[:, :256] = 128                                                       # tiles 0 and 3 are flat: a few hundred bytes
    want = jc.encode_image_tiles(img, 75)
    lens = [len(w) for w in want]
    sb = (min(lens) + max(lens)) // 2
    fits = [n <= sb for n in lens]
    assert any(fits) and not all(fits)
    slots, need, packed, offsets = encode(torch.from_numpy(img).to(DEV), 264, 520, 520, 75, 0, 6, sb)
    assert need.tolist() == lens
    ends = np.cumsum([0] + [n if f else 0 for n, f in zip(lens, fits)])
    assert offsets[:7].tolist() == ends.tolist()
    for k, w in enumerate(want):
        if fits[k]:
            assert slots[k, :lens[k]].tobytes() == w and (slots[k, lens[k]:] == FILL).all()
            assert packed[ends[k]:ends[k + 1]].tobytes() == w
        else:
            assert (slots[k] == FILL).all()
    assert (packed[ends[-1]:] == FILL).all()


def test_two_calls_give_the_same_bytes():
    img, q = jc.image("p264x520"), 75
    plane = torch.from_numpy(img.copy()).to(DEV)
    a = encode(plane, 264, 520, 520, q, 0, 6, 40000)
    b = encode(plane, 264, 520, 520, q, 0, 6, 40000)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
