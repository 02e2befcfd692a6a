"""-m gpu: the Blosc-lz4 encoder (tm_blosc_compress, tm_blosc_compress_tiles) on the case table of tests/blosc_cases.py.

Every frame is written into a buffer prefilled with a guard byte (nothing past the returned length may change), encoded
twice (equal bytes), decoded by the strict Python decoder of blosc_cases and by tm_blosc_decompress -- the decoder pinned on
real c-blosc frames -- and held to the bound helper.  Compression strength: a derived figure for a constant stream, and
<= 1.15 x c-blosc 1.21's own frame on the fixture's fp16 buffers.

Measured on an MI355X (frame bytes / c-blosc's frame bytes): f16_default 1.0076, f16_small_default 0.9724,
f16_blocks64k_leftover 0.9912, f16_clevel9_blocks 1.0136; f32_counts (recorded, not bounded) 1.0036."""
import numpy as np
import pytest
import torch

import blosc_cases as bc
from teramind_amd import _lib, formats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5
TM_DTYPE_F32, TM_DTYPE_F16 = 0, 2


def _dev_bytes(data: bytes, shift: int = 0):
    """The bytes on the device, `shift` bytes into an allocation (an unaligned source)."""
    t = torch.empty(len(data) + shift, dtype=torch.uint8, device=DEV)
    t[shift:].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t[shift:]


def gpu_frame(data: bytes, typesize: int, blocksize: int, shift: int = 0) -> bytes:
    L = _lib.lib()
    src = _dev_bytes(data, shift)
    bound = L.tm_blosc_bound(len(data), typesize, blocksize)
    assert bound == bc.bound(len(data), typesize, blocksize)
    got = []
    for _ in range(2):
        buf = torch.full((bound + 256,), GUARD, dtype=torch.uint8, device=DEV)
        n = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        _lib.check(L.tm_blosc_compress(_lib.c_void_p(src.data_ptr()), len(data), typesize, blocksize, _lib.ptr(buf), bound, _lib.ptr(n),
                                       _lib.current_stream_ptr()), "tm_blosc_compress")
        n, host = int(n.item()), buf.cpu().numpy()
        assert 16 < n <= bound
        assert (host[n:] == GUARD).all(), "bytes past the frame were written"
        got.append(host[:n].tobytes())
    assert got[0] == got[1], "two calls gave different bytes"
    return got[0]


def check_frame(frame: bytes, data: bytes, typesize: int, blocksize: int):
    p = bc.parse_frame(frame)                                       # strict: raises at the first broken rule
    assert p["plain"] == data
    assert formats._blosc_decode(frame) == data                     # the decoder pinned on real c-blosc frames
    bs, nblocks, _leftover, split = bc.geometry(len(data), typesize, blocksize)
    assert (p["typesize"], p["nbytes"], p["blocksize"], len(p["bstarts"])) == (typesize, len(data), bs, nblocks)
    assert p["flags"] == bc.F_LZ4 | (bc.F_SHUFFLE if typesize > 1 else 0) | (0 if split else bc.F_DONT_SPLIT)
    return p


@pytest.mark.parametrize("name", list(bc.CASES))
def test_cases(name):
    make, ts, bs, _why = bc.CASES[name]
    data = make()
    frame = gpu_frame(data, ts, bs)
    p = check_frame(frame, data, ts, bs)
    stored = [s[4] for s in p["streams"]]
    if name == "random":
        assert all(stored) and len(frame) == bc.bound(len(data), ts, bs)                    # the frame equals the bound exactly
    if name == "smooth_f16":
        assert stored == [True, False]                              # low bytes stored, high bytes compressed
    if name in ("n1_ts1", "n12", "n13"):
        assert stored == [True]                                     # below 13 bytes there is no match; 13 constant bytes do not pay
    if name in ("const_32k", "n200_ts2", "ext_runs", "literal_runs", "offsets", "stream64k"):
        assert not any(stored)
    if name == "const_32k":                                         # derived: at worst 64 literals, one match with a 129-byte
        print(f"blosc const_32k: stream of {len(p['streams'][0][3])} bytes")
        assert len(p["streams"][0][3]) <= 256                       # length extension and 5 closing literals


def test_unaligned_source():
    """The bytes entry takes any address: the same frame from a source one and three bytes into its allocation."""
    data = bc.mixed_bytes(3 * 1024 + 5, "shift")
    want = gpu_frame(data, 4, 1024)
    assert gpu_frame(data, 4, 1024, shift=1) == want and gpu_frame(data, 4, 1024, shift=3) == want
    check_frame(want, data, 4, 1024)


@pytest.mark.parametrize("name", list(bc.FIXTURE_CASES))
def test_fixture_buffers_with_cblosc_block_size(name):
    """Each fixture buffer whose c-blosc block size the encoder takes, called with that block size: header bytes 0-11 and
    bstarts[0] are c-blosc's (the flag byte apart from what the fixture asked c-blosc for and the encoder does not offer)."""
    data, ref = bc.fixture(name)
    ts, bs = ref[3], int.from_bytes(ref[8:12], "little")
    frame = gpu_frame(data, ts, max(256, (bs + 3) & ~3))            # the call's block size is a multiple of 4 >= 256: the effective one is c-blosc's
    check_frame(frame, data, ts, max(256, (bs + 3) & ~3))
    assert frame[:2] == ref[:2] and frame[3:12] == ref[3:12]
    assert frame[2] ^ ref[2] == bc.FIXTURE_CASES[name]
    if not ref[2] & bc.F_MEMCPY:
        assert frame[16:20] == ref[16:20]                           # bstarts[0]


def test_strength_against_cblosc():
    """<= 1.15 x c-blosc's frame on the four fp16 buffers (the margin the coarsest acceptable search needed in simulation:
    12.2 %); f32_counts is recorded only."""
    ratios = {}
    for name, bs in list(bc.RATIO_CASES.items()) + [("f32_counts", 65536)]:
        data, ref = bc.fixture(name)
        bs = bs or int.from_bytes(ref[8:12], "little")
        frame = gpu_frame(data, ref[3], bs)
        check_frame(frame, data, ref[3], bs)
        ratios[name] = len(frame) / len(ref)
        print(f"blosc strength {name}: {len(frame)} bytes, c-blosc {len(ref)}, ratio {ratios[name]:.4f}")
    for name in bc.RATIO_CASES:
        assert ratios[name] <= 1.15, ratios


# ---- state tiles cut out of a canvas ------------------------------------------------------------------
def _canvas():
    """fp32 [3, 256 + 64, 512 + 64 + 8]: a frame of -1 around 2 tiles, rows pitched; signal, background and the values
    where float32 -> float16 can go wrong."""
    g = torch.Generator().manual_seed(5)
    cv = torch.full((3, 320, 584), -1.0)
    cv[:, 32:288, 32:544] = torch.randn((3, 256, 512), generator=g) * 0.5
    cv[1, 32:288, 32:300] = -1.0                                    # background inside the first tile
    special = torch.tensor([-0.0, 0.0, 65504.0, -65504.0, 65520.0, -65520.0, 65519.99, 1e-8, -1e-8, 6e-8, 5.96e-8, 2.98e-8, 2.9802326e-8,
                            6.1e-5, 6.0975552e-5, float("nan"), float("inf"), -float("inf"), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                            1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -20, 2049.0, 2051.0, 1e30, -1e30, 1e-30])
    cv[0, 40, 40:40 + special.numel()] = special
    cv[2, 287, 544 - special.numel():544] = special                 # the last row of the second tile
    return cv


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_state_tiles_from_a_pitched_canvas(dtype):
    L = _lib.lib()
    cv = _canvas().to(DEV)
    if dtype == "fp16":
        cv = cv.half()
    C_, TH, TW = 3, 256, 256
    orig = torch.tensor([32 * cv.stride(1) + 32 + c * 256 for c in range(2)], dtype=torch.int64)
    orig_dev = orig.to(DEV)
    bound = L.tm_blosc_bound(C_ * TH * TW * 2, 2, 65536)
    got = []
    for _ in range(2):
        packed = torch.full((2 * bound + 256,), GUARD, dtype=torch.uint8, device=DEV)
        offs = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        _lib.check(L.tm_blosc_compress_tiles(_lib.ptr(cv), TM_DTYPE_F32 if dtype == "fp32" else TM_DTYPE_F16, cv.numel(), C_, TH, TW,
                                             cv.stride(0), cv.stride(1), _lib.ptr(orig_dev), _lib.ptr(orig), 2, _lib.ptr(packed), 2 * bound,
                                             _lib.ptr(offs), _lib.current_stream_ptr()), "tm_blosc_compress_tiles")
        o, host = offs.cpu().tolist(), packed.cpu().numpy()
        assert o[0] == 0 and o[0] < o[1] < o[2] <= 2 * bound
        assert (host[o[2]:] == GUARD).all(), "bytes past the frames were written"
        got.append((o, host[:o[2]].tobytes()))
    assert got[0] == got[1], "two calls gave different bytes"
    o, buf = got[0]
    for c in range(2):
        want = cv[:, 32:288, 32 + c * 256:32 + (c + 1) * 256].half().contiguous().cpu().numpy().tobytes()    # Tensor.half()
        frame = buf[o[c]:o[c + 1]]
        p = check_frame(frame, want, 2, 65536)
        assert len(p["streams"]) == 12 and len(frame) <= bound
    assert np.frombuffer(want, np.float16)[-1] == np.float16(1e-30) == 0        # the specials are in the second tile's last row


def test_constant_background_tile_is_tiny():
    """A tile of constant -1 (empty background) takes under 1 % of its plain size."""
    L = _lib.lib()
    cv = torch.full((16, 256, 256), -1.0, dtype=torch.float16, device=DEV)
    bound = L.tm_blosc_bound(cv.numel() * 2, 2, 65536)
    packed = torch.empty(bound, dtype=torch.uint8, device=DEV)
    offs = torch.empty(2, dtype=torch.int64, device=DEV)
    orig = torch.zeros(1, dtype=torch.int64)
    _lib.check(L.tm_blosc_compress_tiles(_lib.ptr(cv), TM_DTYPE_F16, cv.numel(), 16, 256, 256, cv.stride(0), cv.stride(1),
                                         _lib.ptr(orig.to(DEV)), _lib.ptr(orig), 1, _lib.ptr(packed), bound, _lib.ptr(offs),
                                         _lib.current_stream_ptr()), "tm_blosc_compress_tiles")
    n = int(offs[1].item())
    frame = packed[:n].cpu().numpy().tobytes()
    assert bc.decode_frame(frame) == cv.cpu().numpy().tobytes()
    print(f"blosc background tile: {n} bytes, {n / (cv.numel() * 2):.5f} of plain")
    assert n < 0.01 * cv.numel() * 2, n
