"""Baseline JPEG of one 8-bit grey component, restated in numpy from ITU-T T.81 and the published integer "islow" forward
DCT, with the tables as data; and the case list of the JPEG tile encoder's tests.

The contract (exact integer work at every step, so the bytes are a function of the pixels alone):
  level shift 128 -> 8 x 8 forward DCT (CONST_BITS 13, PASS1_BITS 2: rows first, outputs 0 and 4 shifted left by 2 and the
  others descaled by 11; then columns, outputs 0 and 4 descaled by 2 and the others by 15) -> quantiser
  (|c| + (qv >> 1)) // qv with qv = q << 3 -> zigzag -> DC difference to the previous block (0 at the start) -> the typical
  luminance Huffman tables of Annex K.3, ZRL for runs above 15, EOB -> MSB-first bits, 0x00 after every 0xFF, the last byte
  padded with one-bits, no restart markers.
A tile is 256 x 256 and always full: pixels beyond the image repeat the last row / column.
"""
import functools

import numpy as np

TILE = 256
QUALITIES = (1, 10, 75, 90, 100)

K1_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
                   53, 60, 61, 54, 47, 55, 62, 63])
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def huff_codes(bits, vals):
    """symbol -> (code, length), the code assignment of T.81 Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = huff_codes(DC_BITS, DC_VALS)
AC_CODES = huff_codes(AC_BITS, AC_VALS)


def quant_table(quality):
    """The K.1 luminance table at `quality`, natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((K1_LUMA * s + 50) // 100, 1, 255)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass over the last axis of int64 [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = np.empty_like(d)
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[..., 0], o[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[..., 2] = _descale(z1 + t13 * 6270, n)
    o[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7] = _descale(t4 + z1 + z3, n)
    o[..., 5] = _descale(t5 + z2 + z4, n)
    o[..., 3] = _descale(t6 + z2 + z3, n)
    o[..., 1] = _descale(t7 + z1 + z4, n)
    return o


def quantised_blocks(tile, quality):
    """uint8 [8 m, 8 n] -> int64 [m n, 64] quantised coefficients in zigzag order, blocks in raster order."""
    h, w = tile.shape
    b = tile.astype(np.int64).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128
    b = _fdct_pass(b, True)                                        # rows
    b = _fdct_pass(b.transpose(0, 2, 1), False).transpose(0, 2, 1)  # columns
    qv = (quant_table(quality) << 3).reshape(8, 8)
    q = (np.abs(b) + (qv >> 1)) // qv * np.sign(b)
    return q.reshape(-1, 64)[:, ZIGZAG]


def _nbits(v):
    return int(abs(int(v))).bit_length()


def _vbits(v, s):
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def entropy_code(zz):
    """int64 [blocks, 64] zigzag coefficients -> the entropy-coded segment (stuffed, padded) as bytes."""
    codes, lens = [], []
    prev = 0
    for blk in zz:
        diff = int(blk[0]) - prev
        prev = int(blk[0])
        s = _nbits(diff)
        c, n = DC_CODES[s]
        codes.append((c << s) | _vbits(diff, s))
        lens.append(n + s)
        last = 0
        for k in np.flatnonzero(blk[1:]) + 1:
            run = int(k) - last - 1
            while run > 15:
                c, n = AC_CODES[0xF0]
                codes.append(c)
                lens.append(n)
                run -= 16
            v = int(blk[k])
            s = _nbits(v)
            c, n = AC_CODES[(run << 4) | s]
            codes.append((c << s) | _vbits(v, s))
            lens.append(n + s)
            last = int(k)
        if last != 63:
            c, n = AC_CODES[0]
            codes.append(c)
            lens.append(n)
    codes, lens = np.asarray(codes, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    sh = lens[:, None] - 1 - np.arange(32)[None, :]
    bits = ((codes[:, None] >> np.maximum(sh, 0)) & 1)[sh >= 0].astype(np.uint8)
    pad = (-bits.size) % 8
    raw = np.packbits(np.concatenate([bits, np.ones(pad, dtype=np.uint8)]))
    out = np.zeros(raw.size * 2, dtype=np.uint8)
    ff = raw == 255
    pos = np.arange(raw.size) + np.concatenate([[0], np.cumsum(ff)[:-1]])
    out[pos] = raw
    return out[:raw.size + int(ff.sum())].tobytes()


def tile_of(img, ty, tx):
    """The full 256 x 256 tile (ty, tx) of uint8 [H, W]: the last row / column repeated beyond the image."""
    H, W = img.shape
    ys = np.minimum(np.arange(ty * TILE, (ty + 1) * TILE), H - 1)
    xs = np.minimum(np.arange(tx * TILE, (tx + 1) * TILE), W - 1)
    return img[np.ix_(ys, xs)]


def grid_of(H, W):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def encode_tile(tile, quality):
    return entropy_code(quantised_blocks(tile, quality))


def encode_image_tiles(img, quality):
    """The scan of every tile of the image's grid, row-major."""
    gy, gx = grid_of(*img.shape)
    return [encode_tile(tile_of(img, ty, tx), quality) for ty in range(gy) for tx in range(gx)]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _smooth():
    y, x = np.mgrid[0:256, 0:256]
    return (127.5 + 80 * np.sin(x / 37.0) * np.cos(y / 23.0) + 40 * np.sin((x + y) / 91.0)).astype(np.uint8)


def _sparse():
    a = np.full((256, 256), 128, dtype=np.uint8)       # +90 on every 8th row and on the last column of each block: long zero runs
    a[7::8, :] = 218
    a[:, 7::8] = 218
    return a


def _checker(px):
    y, x = np.mgrid[0:256, 0:256]
    return ((((y // px) + (x // px)) & 1) * 255).astype(np.uint8)


FULL_CASES = {                    # one tile each
    "noise": lambda: _noise(256, 256, 1),
    "smooth": _smooth,
    "flat0": lambda: np.zeros((256, 256), dtype=np.uint8),
    "flat255": lambda: np.full((256, 256), 255, dtype=np.uint8),
    "checker1": lambda: _checker(1),
    "checker8": lambda: _checker(8),
    "sparse": _sparse,
}
PARTIAL_CASES = {                 # tiles completed by edge replication
    "p16x24": lambda: _noise(16, 24, 2),
    "p8x8": lambda: _noise(8, 8, 3),
    "p264x520": lambda: _noise(264, 520, 4),      # 2 x 3 tiles, 8 px left over both ways
}
CASES = {**FULL_CASES, **PARTIAL_CASES}


@functools.lru_cache(maxsize=None)
def image(name):
    a = CASES[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference_scans(name, quality):
    """Per-tile scans of a case, computed once per process and shared (tuples: not to be changed)."""
    return tuple(encode_image_tiles(image(name), quality))
