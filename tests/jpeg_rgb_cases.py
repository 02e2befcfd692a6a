"""The colour composite and its baseline 4:4:4 YCbCr JPEG, restated in numpy; and the case list of the colour tile encoder's
tests.  The 8 x 8 DCT, the zigzag order, the luminance tables and the code assignment come from jpeg_cases; added here are
the composite, libjpeg's fixed-point colour conversion, the chrominance tables of T.81 Annex K.2 / K.4 / K.6 and the
interleaved scan.

The contract (exact integer work, so the bytes are a function of the stain planes and the settings alone):
  composite of pixel (y, x) of a level [H, W]: the planes' bytes as R, G, B (0 for a missing plane) -> brightness
  min(255, trunc(float32(bright) * float32(v))) unless bright == 1 -> overlay pixel ov = overlay[(y oh) // H][(x ow) // W],
  blended in where any of its channels is non-zero: (ov alpha + v (255 - alpha) + 127) // 255
  -> Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
  -> per component the grey pipeline of jpeg_cases (level shift, islow DCT, quantiser, zigzag); Y with the K.1 quantiser
  and the K.3 / K.5 codes, Cb and Cr with K.2 (scaled and clipped like K.1) and K.4 / K.6
  -> one scan, the blocks interleaved Y Cb Cr per 8 x 8 MCU in raster order, DC predicted per component
  -> MSB-first bits, 0x00 after every 0xFF, one-bit padding.
A tile is 256 x 256 and always full: pixels beyond the image repeat the composite's last row / column.
"""
import functools

import numpy as np

import jpeg_cases as jc

TILE = jc.TILE
QUALITIES = jc.QUALITIES

K2_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                      47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)
DC_BITS_C = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
AC_BITS_C = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_VALS_C = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def _code_arrays(codes, n):
    """{symbol: (code, length)} -> (code[n], length[n]) arrays."""
    c, ln = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for sym, (code, length) in codes.items():
        c[sym], ln[sym] = code, length
    return c, ln


# index 0: the luminance tables (component Y), 1: the chrominance tables (Cb, Cr)
_DC = [_code_arrays(jc.DC_CODES, 16), _code_arrays(jc.huff_codes(DC_BITS_C, jc.DC_VALS), 16)]
_AC = [_code_arrays(jc.AC_CODES, 256), _code_arrays(jc.huff_codes(AC_BITS_C, AC_VALS_C), 256)]
DC_CODE, DC_LEN = np.stack([t[0] for t in _DC]), np.stack([t[1] for t in _DC])
AC_CODE, AC_LEN = np.stack([t[0] for t in _AC]), np.stack([t[1] for t in _AC])


def quant_table(quality, chroma):
    """K.1 (luminance) or K.2 (chrominance) at `quality`, natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip(((K2_CHROMA if chroma else jc.K1_LUMA) * s + 50) // 100, 1, 255)


# ---- the composite -----------------------------------------------------------------------------------------------------
def brighten(v, bright):
    """uint8 array -> min(255, trunc(float32(bright) * float32(v)))."""
    return np.minimum(255, np.trunc(np.float32(bright) * v.astype(np.float32))).astype(np.uint8)


def compose(planes, bright=1.0, overlay=None, alpha=100):
    """(r, g, b) uint8 [H, W] planes (entries may be None) -> the composite, uint8 [H, W, 3]."""
    H, W = next(p for p in planes if p is not None).shape
    v = np.stack([np.zeros((H, W), dtype=np.uint8) if p is None else p for p in planes], -1)
    if bright != 1:
        v = brighten(v, bright)
    if overlay is not None:
        oh, ow = overlay.shape[:2]
        ov = overlay[(np.arange(H) * oh) // H][:, (np.arange(W) * ow) // W].astype(np.int64)
        mixed = (ov * alpha + v.astype(np.int64) * (255 - alpha) + 127) // 255
        v = np.where(ov.any(-1)[:, :, None], mixed, v).astype(np.uint8)
    return v


def ycc(rgb):
    """uint8 [..., 3] RGB -> int64 [..., 3] Y Cb Cr in 0 .. 255 (libjpeg's 16-bit fixed point)."""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                     (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16], -1)


# ---- the scan ----------------------------------------------------------------------------------------------------------
def quantised_component(comp, qtable):
    """int64 [8 m, 8 n] samples 0 .. 255 -> int64 [m n, 64] quantised coefficients in zigzag order, blocks in raster order."""
    h, w = comp.shape
    b = comp.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128
    b = jc._fdct_pass(b, True)
    b = jc._fdct_pass(b.transpose(0, 2, 1), False).transpose(0, 2, 1)
    qv = (qtable << 3).reshape(8, 8)
    return ((np.abs(b) + (qv >> 1)) // qv * np.sign(b)).reshape(-1, 64)[:, jc.ZIGZAG]


def _nbits(a):
    a = np.abs(a)
    s = np.zeros(a.shape, dtype=np.int64)
    for k in range(16):
        s += (a >> k) > 0
    return s


def _vbits(v, s):
    return np.where(v >= 0, v, v - 1) & ((1 << s) - 1)


def entropy_code(zz, table, dc_diff):
    """The scan of blocks zz int64 [blocks, 64] in scan order; table[blocks] is 0 (luminance codes) or 1 (chrominance),
    dc_diff[blocks] the DC difference of each block to the one before it of its component.  Every code of the scan gets the key
    (block, zigzag position, rank): the DC code at position 0, the ZRLs of a coefficient before its own code, EOB at 64."""
    nb = zz.shape[0]
    blk = np.arange(nb)
    s = _nbits(dc_diff)
    items = [(blk, np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64),
              (DC_CODE[table, s] << s) | _vbits(dc_diff, s), DC_LEN[table, s] + s)]
    b, k = np.nonzero(zz[:, 1:])
    k = k + 1
    first = np.concatenate([[True], b[1:] != b[:-1]]) if b.size else np.zeros(0, dtype=bool)
    run = k - np.where(first, 0, np.concatenate([[0], k[:-1]])) - 1
    v = zz[b, k]
    s = _nbits(v)
    tb = table[b]
    for j in range(3):                                             # up to three ZRLs (runs of 16 zeros) before a coefficient
        m = (run >> 4) > j
        items.append((b[m], k[m], np.full(int(m.sum()), j), AC_CODE[tb[m], 0xF0], AC_LEN[tb[m], 0xF0]))
    sym = ((run & 15) << 4) | s
    items.append((b, k, np.full(b.size, 3), (AC_CODE[tb, sym] << s) | _vbits(v, s), AC_LEN[tb, sym] + s))
    eob = zz[:, 63] == 0
    items.append((blk[eob], np.full(int(eob.sum()), 64), np.zeros(int(eob.sum()), dtype=np.int64), AC_CODE[table[eob], 0],
                  AC_LEN[table[eob], 0]))
    B, K, R, codes, lens = (np.concatenate([it[j] for it in items]) for j in range(5))
    order = np.lexsort((R, K, B))
    codes, lens = codes[order], lens[order]
    sh = lens[:, None] - 1 - np.arange(27)[None, :]                # a code is 26 bits at most (16 + 10)
    assert lens.max() <= 27
    bits = ((codes[:, None] >> np.maximum(sh, 0)) & 1)[sh >= 0].astype(np.uint8)
    raw = np.packbits(np.concatenate([bits, np.ones((-bits.size) % 8, dtype=np.uint8)]))
    out = np.zeros(raw.size * 2, dtype=np.uint8)
    ff = raw == 255
    out[np.arange(raw.size) + np.concatenate([[0], np.cumsum(ff)[:-1]])] = raw
    return out[:raw.size + int(ff.sum())].tobytes()


def encode_tile(rgb, quality):
    """uint8 [8 m, 8 n, 3] RGB -> the entropy-coded segment of its 4:4:4 scan."""
    c = ycc(rgb)
    zz = np.stack([quantised_component(c[..., k], quant_table(quality, k > 0)) for k in range(3)], 1)    # [mcu, 3, 64]
    dc = zz[:, :, 0]
    diff = dc - np.concatenate([np.zeros((1, 3), dtype=np.int64), dc[:-1]])
    table = np.tile(np.array([0, 1, 1]), zz.shape[0])
    return entropy_code(zz.reshape(-1, 64), table, diff.reshape(-1))


def tile_of(img, ty, tx):
    """The full 256 x 256 tile (ty, tx) of uint8 [H, W, 3]: the last row / column repeated beyond the image."""
    H, W = img.shape[:2]
    ys = np.minimum(np.arange(ty * TILE, (ty + 1) * TILE), H - 1)
    xs = np.minimum(np.arange(tx * TILE, (tx + 1) * TILE), W - 1)
    return img[ys][:, xs]


def encode_image_tiles(img, quality):
    """The scan of every tile of the composite's grid, row-major."""
    gy, gx = jc.grid_of(*img.shape[:2])
    return [encode_tile(tile_of(img, ty, tx), quality) for ty in range(gy) for tx in range(gx)]


# ---- the cases: (r, g, b) plane triples --------------------------------------------------------------------------------
def _flat(v, h=256, w=256):
    return np.full((h, w), v, dtype=np.uint8)


FULL_CASES = {                    # one tile each
    "noise3": lambda: tuple(jc._noise(256, 256, 11 + k) for k in range(3)),
    "stains": lambda: (_flat(0), jc._smooth(), jc._sparse()),
    "checker": lambda: (jc._checker(1), jc._checker(8), _flat(255)),
    "flat": lambda: (_flat(10), _flat(200), _flat(90)),
    "rnone": lambda: (None, jc._noise(256, 256, 21), jc._smooth()),          # the exported form: no red plane
}
PARTIAL_CASES = {                 # tiles completed by edge replication
    "p16x24": lambda: tuple(jc._noise(16, 24, 31 + k) for k in range(3)),
    "p8x8": lambda: tuple(jc._noise(8, 8, 41 + k) for k in range(3)),
    "p264x520": lambda: tuple(jc._noise(264, 520, 51 + k) for k in range(3)),    # 2 x 3 tiles, 8 px left over both ways
}
CASES = {**FULL_CASES, **PARTIAL_CASES}


@functools.lru_cache(maxsize=None)
def planes(name):
    out = CASES[name]()
    for p in out:
        if p is not None:
            p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def image(name):
    """The plain composite (bright 1, no overlay) of a case."""
    a = compose(planes(name))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference_scans(name, quality):
    """Per-tile scans of a case's plain composite, computed once per process and shared (tuples: not to be changed)."""
    return tuple(encode_image_tiles(image(name), quality))


def overlay_case(oh=37, ow=53, seed=7):
    """A small overlay with black (not blended) regions: sizes that divide neither 264 x 520 nor 256 x 256."""
    rng = np.random.default_rng(seed)
    ov = rng.integers(0, 256, (oh, ow, 3), dtype=np.uint8)
    ov[rng.random((oh, ow)) < 0.4] = 0
    ov[0, 0] = (0, 0, 9)                                          # one channel is enough to blend
    return ov
