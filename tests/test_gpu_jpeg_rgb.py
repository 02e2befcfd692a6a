"""-m gpu: tm_jpeg_encode_tiles_rgb and tm_rgb_compose against the numpy restatement of the colour composite and its 4:4:4
JPEG (jpeg_rgb_cases.py, itself held to libjpeg's bytes by test_jpeg_rgb_cases_host.py): every tile's bytes and length, and
every composite pixel, exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_rgb_cases as rc
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


def source(planes, pitches, H, W, bright=1.0, overlay=None, alpha=100):
    """The leading arguments of the two entry points; planes are device tensors or None."""
    ptrs = (C.c_void_p * 3)(*[None if p is None else p.data_ptr() for p in planes])
    pit = (C.c_int64 * 3)(*pitches)
    oh, ow = (0, 0) if overlay is None else overlay.shape[:2]
    return ptrs, pit, H, W, bright, _lib.ptr(overlay), oh, ow, alpha


def upload(planes):
    return [None if p is None else torch.from_numpy(p.copy()).to(DEV) for p in planes]


def encode(src, quality, tile0, ntiles, slot_bytes, compact=True, extra_slots=1):
    """-> (slots [ntiles + extra][slot_bytes], need [ntiles], packed bytes or None, offsets or None), host arrays.  Every
    output buffer is prefilled with FILL / -1."""
    slots = torch.full(((ntiles + extra_slots) * slot_bytes,), FILL, dtype=torch.uint8, device=DEV)
    need = torch.full((ntiles + 1,), -1, dtype=torch.int32, device=DEV)
    packed = torch.full((ntiles * slot_bytes + 64,), FILL, dtype=torch.uint8, device=DEV) if compact else None
    offsets = torch.full((ntiles + 2,), -1, dtype=torch.int64, device=DEV) if compact else None
    _lib.check(_lib.lib().tm_jpeg_encode_tiles_rgb(*src, quality, tile0, ntiles, _lib.ptr(slots), slot_bytes, _lib.ptr(need),
                                                   _lib.ptr(packed), _lib.ptr(offsets), _lib.current_stream_ptr()),
               "tm_jpeg_encode_tiles_rgb")
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


def case_source(name, **kw):
    pl = rc.planes(name)
    H, W = rc.image(name).shape[:2]
    dev = upload(pl)
    return dev, source(dev, [0 if p is None else W for p in pl], H, W, **kw)


@pytest.mark.parametrize("quality", rc.QUALITIES)
@pytest.mark.parametrize("name", list(rc.CASES))
def test_tile_bytes_equal_the_restatement(name, quality):
    want = rc.reference_scans(name, quality)
    keep, src = case_source(name)
    sb = slot_for(want)
    check_tiles(*encode(src, quality, 0, len(want), sb), want, sb)


def test_sub_range_writes_only_its_slots():
    want = rc.reference_scans("p264x520", 75)[2:5]
    keep, src = case_source("p264x520")
    sb = slot_for(want)
    check_tiles(*encode(src, 75, 2, 3, sb, extra_slots=3), want, sb)


@pytest.mark.parametrize("pitch,off", [(528, 0), (523, 0), (520, 3)])        # aligned pitch, odd pitch, unaligned base
def test_pitched_planes_give_the_bytes_of_the_contiguous_ones(pitch, off):
    """Each plane in its own pitched buffer; the green one keeps pitch 520 at an aligned base, so that the vector path needs
    all three to qualify."""
    q = 90
    want = rc.reference_scans("p264x520", q)
    bufs, views, pitches = [], [], []
    for k, p in enumerate(rc.planes("p264x520")):
        pt, of = (520, 0) if k == 1 else (pitch, off)
        buf = torch.full((264 * pt + of + 16,), 77, dtype=torch.uint8, device=DEV)
        buf[of:of + 264 * pt].view(264, pt)[:, :520] = torch.from_numpy(p.copy()).to(DEV)
        bufs.append(buf)
        views.append(buf[of:])
        pitches.append(pt)
    sb = slot_for(want)
    check_tiles(*encode(source(views, pitches, 264, 520), q, 0, 6, sb), want, sb)


@pytest.mark.parametrize("missing", [0, 1, 2])
def test_a_null_plane_is_all_zeros(missing):
    pl = list(rc.planes("p264x520"))
    pl[missing] = None
    want = rc.encode_image_tiles(rc.compose(pl), 75)
    dev = upload(pl)
    sb = slot_for(want)
    check_tiles(*encode(source(dev, [0 if p is None else 520 for p in pl], 264, 520), 75, 0, 6, sb), want, sb)


@pytest.mark.parametrize("bright", [0.5, 2.0])
def test_brightness_is_applied_in_the_block_load(bright):
    pl = rc.planes("p264x520")
    want = rc.encode_image_tiles(rc.compose(pl, bright=bright), 75)
    keep, src = case_source("p264x520", bright=bright)
    sb = slot_for(want)
    check_tiles(*encode(src, 75, 0, 6, sb), want, sb)


def test_overlay_of_a_size_that_does_not_divide_is_blended_in_the_block_load():
    pl, ov = rc.planes("p264x520"), rc.overlay_case()
    want = rc.encode_image_tiles(rc.compose(pl, bright=1.3, overlay=ov, alpha=100), 75)
    ovd = torch.from_numpy(ov).to(DEV)
    keep, src = case_source("p264x520", bright=1.3, overlay=ovd, alpha=100)
    sb = slot_for(want)
    check_tiles(*encode(src, 75, 0, 6, sb), want, sb)


def test_slot_too_small_reports_need_and_keeps_the_prefill():
    q = 75
    want = rc.reference_scans("noise3", q)
    assert len(want[0]) > 16384
    keep, src = case_source("noise3")
    slots, need, packed, offsets = encode(src, q, 0, 1, 16384)
    assert need.tolist() == [len(want[0])]
    assert (slots == FILL).all() and (packed == FILL).all()
    assert offsets[:2].tolist() == [0, 0]                                     # nothing packed for the slot that did not fit
    sb = int(need[0])                                                        # the second call: a slot of exactly that size
    check_tiles(*encode(src, q, 0, 1, sb), want, sb)


def test_mixed_batch_packs_only_the_filled_slots():
    """Six tiles, a slot size between the smallest and the largest scan: the small ones are written and packed, the rest only
    report their length."""
    pl = [np.array(p) for p in rc.planes("p264x520")]
    for p in pl:
        p[:, :256] = 128                                                     # tiles 0 and 3 are flat: a few hundred bytes
    want = rc.encode_image_tiles(rc.compose(pl), 75)
    lens = [len(w) for w in want]
    sb = (min(lens) + max(lens)) // 2
    fits = [n <= sb for n in lens]
    assert any(fits) and not all(fits)
    dev = upload(pl)
    slots, need, packed, offsets = encode(source(dev, [520] * 3, 264, 520), 75, 0, 6, sb)
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
    keep, src = case_source("p264x520")
    a = encode(src, 75, 0, 6, 120000)
    b = encode(src, 75, 0, 6, 120000)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kw", [dict(), dict(bright=2.0), dict(bright=0.5, overlay=True, alpha=100), dict(overlay=True, alpha=255),
                                dict(overlay=True, alpha=0)])
def test_compose_equals_the_numpy_compose(kw):
    """A pitched destination: the bytes between rows keep their prefill."""
    pl = list(rc.planes("p264x520"))
    pl[0] = None
    ov = rc.overlay_case() if kw.pop("overlay", False) else None
    want = rc.compose(pl, overlay=ov, **kw)
    dev = upload(pl)
    ovd = None if ov is None else torch.from_numpy(ov).to(DEV)
    pitch = 3 * 520 + 5
    dst = torch.full((264, pitch), FILL, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().tm_rgb_compose(*source(dev, [0, 520, 520], 264, 520, overlay=ovd, **kw), _lib.ptr(dst), pitch,
                                         _lib.current_stream_ptr()), "tm_rgb_compose")
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[:, :3 * 520].reshape(264, 520, 3), want)
    assert (got[:, 3 * 520:] == FILL).all()
