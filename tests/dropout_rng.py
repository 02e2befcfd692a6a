"""Numpy restatement of the ResBlock dropout keep mask that the training kernels draw, shared by the tests and
tools/make_train_dropout_golden.py.

Philox4x32-10 (Random123 constants).  Element (n, c, z, y, x) of a [N, C, Z, S, S] activation: voxel index
v = ((n Z + z) S + y) S + x, counter (v mod 2^32, v >> 32, site, c >> 2), key (key mod 2^32, key >> 32); the element's word is
output word c & 3; it is dropped iff word < T, T = min(floor(p 2^32), 2^32 - 1) with p taken as float32 (the C ABI's type).
A kept element is multiplied by float32(1) / float32(1 - p)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of uint32 words broadcast together, key: (k0, k1) ints -> 4 uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _LO for w in ctr]
    c = np.broadcast_arrays(*c)
    c = [w.copy() for w in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _LO, p1 >> np.uint64(32), p1 & _LO
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def threshold(p):
    """T of the rule: drop iff word < T."""
    return int(min(np.floor(float(np.float32(p)) * 2.0 ** 32), 2.0 ** 32 - 1))


def drop_scale(p):
    return np.float32(1.0) / np.float32(1.0 - float(np.float32(p)))


def keep_words(key, site, v, c):
    """The Philox word that decides element (voxel index v, channel c); v and c broadcast together."""
    v = np.asarray(v, dtype=np.uint64)
    c = np.asarray(c, dtype=np.int64)
    w = philox4x32_10((v & _LO, v >> np.uint64(32), np.uint64(site), (c >> 2).astype(np.uint64)), (key & 0xFFFFFFFF, key >> 32))
    out = np.broadcast_arrays(*w, c)
    sel = out[4] & 3
    return np.choose(sel, out[:4])


def keep_mask(key, site, p, shape):
    """bool keep mask of shape [N, C, Z, S, S] (True = kept)."""
    N, C, Z, S, S2 = shape
    assert S == S2
    v = np.arange(N * Z * S * S, dtype=np.uint64).reshape(N, 1, Z, S, S)
    c = np.arange(C, dtype=np.int64).reshape(1, C, 1, 1, 1)
    return keep_words(key, site, v, c) >= np.uint32(threshold(p))
