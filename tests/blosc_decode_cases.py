"""Frames for the Blosc-lz4 decoder on the GPU (tm_blosc_decompress_dev / _tiles): the case table of
tests/test_blosc_decode_cases_host.py, tests/test_gpu_blosc_decode.py and tools/blosc_decode_check.cpp (no GPU here).

  good frames     every bc.CASES buffer encoded by bc.encode_frame, the ten real c-blosc 1.21 frames of the fixture, and
                  hand-made long streams (longer than the 64 KiB ring the kernel keeps its history in)
  corrupt streams one broken LZ4 stream inside an otherwise valid frame that also holds good streams
  corrupt frames  refused on the host before any launch, and frames that are "host only"
  chunk grids     zarr arrays of several chunks, one with a clipped edge chunk

`python tests/blosc_decode_cases.py corpus.bin` writes the streams of every good and every corrupt-stream case for
tools/blosc_decode_check.cpp."""
import functools
import json
import struct
import sys
import zipfile

import numpy as np

import blosc_cases as bc

RING = 65536                     # the kernel's window: positions p and p + RING share a slot


# ---- hand-made streams -----------------------------------------------------------------------------
def build_stream(seqs):
    """[(literals, offset, match length)], the last with offset 0 -> (compressed, plain)"""
    comp, plain = bytearray(), bytearray()
    for lits, off, ml in seqs:
        bc._put_sequence(comp, lits, off, ml)
        plain += lits
        if off:
            assert 1 <= off <= len(plain) and ml >= 4
            start = len(plain)
            plain += (bytes(plain[start - off:start]) * (ml // off + 1))[:ml] if off < ml else plain[start - off:start - off + ml]
    return bytes(comp), bytes(plain)


def one_stream_frame(comp: bytes, nplain: int) -> bytes:
    """A typesize-1 frame of one block whose one stream is `comp` (block size = nplain >= 128: "split" into one stream)."""
    assert nplain >= 128 and len(comp) < nplain
    cbytes = bc.HEADER + 4 + 4 + len(comp)
    return (bytes((2, 1, bc.F_LZ4, 1)) + nplain.to_bytes(4, "little") * 2 + cbytes.to_bytes(4, "little") + (bc.HEADER + 4).to_bytes(4, "little")
            + len(comp).to_bytes(4, "little") + comp)


class _Uniq:
    """unique literals on demand (no accidental repeats: what a case copies is what it placed)"""
    def __init__(self, tag):
        self.buf, self.k = bc.unique_bytes(400000, tag), 0

    def __call__(self, n):
        self.k += n
        assert self.k <= len(self.buf)
        return self.buf[self.k - n:self.k]


def far_match():
    """140000 literals, then a match at distance 65535 whose source [74465, 76465) lies beyond position 65536."""
    u = _Uniq("far")
    return build_stream([(u(140000), 65535, 2000), (u(12), 0, 0)])


def wrap_straddle():
    """Literal runs and matches that straddle the positions 65536 and 131072, where a 64 KiB ring wraps."""
    u = _Uniq("wrap")
    seqs = [(u(65530), 7, 4),                 # -> 65534
            (u(10), 20000, 80),               # literals [65534, 65544) straddle 65536; match -> 65624
            (u(65436), 31, 31),               # literals -> 131060; the match [131060, 131091) straddles 131072
            (u(5), 65535, 3000),              # a far match behind the second wrap -> 134096
            (u(62430), 1000, 60),             # -> 196586
            (u(40), 0, 0)]                    # literals [196586, 196626) straddle 196608
    comp, plain = build_stream(seqs)
    assert len(plain) == 196626
    return comp, plain


def overlap_wrap():
    """Overlapping matches (offset 1, 3 and 63) across the wrap, and one of offset 3 that is longer than the ring itself."""
    u = _Uniq("ovl")
    seqs = [(u(65500), 1, 100),               # [65500, 65600)
            (u(65440), 3, 100),               # [131040, 131140)
            (u(65430), 63, 200),              # [196570, 196770)
            (u(30), 3, 70000),                # [196800, 266800): its own output comes round the ring
            (u(12), 0, 0)]
    return build_stream(seqs)


def lz4_runs(s: bytes) -> bytes:
    """A fast strict encoder for the large cases: runs of one byte (>= 8) become a match at offset 1, the rest literals."""
    n = len(s)
    a = np.frombuffer(s, np.uint8)
    cut = np.flatnonzero(np.diff(a)) + 1
    starts, ends = np.concatenate(([0], cut)), np.concatenate((cut, [n]))
    out, anchor = bytearray(), 0
    for st, en in zip(starts.tolist(), ends.tolist()):
        en = min(en, n - bc.LASTLITERALS)
        if en - st < 9 or st + 1 > n - bc.MFLIMIT:
            continue
        bc._put_sequence(out, s[anchor:st + 1], 1, en - st - 1)
        anchor = en
    bc._put_sequence(out, s[anchor:], 0, 0)
    return bytes(out)


def big_chunk():
    """A [25, 64, 128] float16 chunk (409600 bytes) at block size 262144: two 131072-byte streams and a 147456-byte unsplit
    leftover, as c-blosc frames a chunk of the reference's tiles."""
    plain = bc.half_background(204800)
    return bc.encode_frame(plain, 2, 262144, lz4=lz4_runs), plain


FIXTURE_NAMES = ["f16_default", "f16_small_default", "f16_blocks64k_leftover", "f16_noshuffle", "f16_gauss", "f16_clevel0_memcpy",
                 "f16_tiny_nosplit", "f16_clevel9_blocks", "f32_counts", "u8_random"]
LONG_CASES = {"far_match": far_match, "wrap_straddle": wrap_straddle, "overlap_wrap": overlap_wrap}
GOOD_NAMES = [f"case/{n}" for n in bc.CASES] + [f"fixture/{n}" for n in FIXTURE_NAMES] + [f"long/{n}" for n in LONG_CASES] + ["long/big_chunk"]


@functools.lru_cache(maxsize=None)
def good(name: str):
    """-> (frame, plain)"""
    kind, n = name.split("/")
    if kind == "case":
        make, ts, bs, _ = bc.CASES[n]
        plain = make()
        return bc.encode_frame(plain, ts, bs), plain
    if kind == "fixture":
        plain, frame = bc.fixture(n)
        return frame, plain
    if n == "big_chunk":
        return big_chunk()
    comp, plain = LONG_CASES[n]()
    return one_stream_frame(comp, len(plain)), plain


# ---- corrupt streams -----------------------------------------------------------------------------
HOST_PLAIN = 2048                # the plain size of the stream that is replaced


def _seq(*seqs):
    return build_stream(list(seqs))[0]


_U = bc.unique_bytes(4096, "bad")
# name -> the broken stream (decodes, if at all, against a plain size of 2048)
CORRUPT_STREAMS = {
    "offset_zero": bytes((0x44,)) + _U[:4] + b"\x00\x00" + bytes((0x00,)),
    "offset_beyond_produced": bytes((0x40,)) + _U[:4] + b"\x05\x00" + bytes((0x50,)) + _U[4:9],
    "literals_past_the_stream": bytes((0xF0, 100)) + _U[:10],
    "length_extension_off_the_end": bytes((0x4F,)) + _U[:4] + b"\x01\x00" + b"\xff\xff",
    "literal_extension_off_the_end": bytes((0xF0, 0xFF, 0xFF)),
    "offset_cut": bytes((0x44,)) + _U[:4] + b"\x01",
    "literals_overrun": _seq((_U[:100], 1, 1940), (_U[100:120], 0, 0)),
    "match_overrun": _seq((_U[:100], 1, 2000), (_U[100:112], 0, 0)),
    "ends_short": _seq((_U[:100], 1, 1000), (_U[100:112], 0, 0)),
}


@functools.lru_cache(maxsize=None)
def _host_frame():
    plain = bc.mixed_bytes(4 * 4096 + 1002, "host")
    return bc.encode_frame(plain, 2, 4096), plain


def rebuild(frame: bytes, replace: dict) -> bytes:
    """The strict frame with stream k replaced by replace[k]; lengths, bstarts and cbytes follow."""
    p = bc.parse_frame(frame)
    nblocks = len(p["bstarts"])
    body, bstarts, last = bytearray(), [], -1
    for k, (j, _sp, _ne, data, _stored) in enumerate(p["streams"]):
        if j != last:
            bstarts.append(bc.HEADER + 4 * nblocks + len(body))
            last = j
        data = replace.get(k, data)
        body += len(data).to_bytes(4, "little") + data
    cbytes = bc.HEADER + 4 * nblocks + len(body)
    return frame[:12] + cbytes.to_bytes(4, "little") + b"".join(b.to_bytes(4, "little") for b in bstarts) + bytes(body)


@functools.lru_cache(maxsize=None)
def corrupt_stream_frame(name: str) -> bytes:
    """The host frame (four split blocks and a leftover: nine streams) with its stream 3 broken."""
    frame, _ = _host_frame()
    assert bc.parse_frame(frame)["streams"][3][2] == HOST_PLAIN
    bad = CORRUPT_STREAMS[name]
    assert len(bad) != HOST_PLAIN
    return rebuild(frame, {3: bad})


def flipped_stream_byte(frame: bytes) -> bytes:
    """One byte changed inside the first LZ4 stream that has a match: its first offset's high byte becomes 0xFF, and the offset
    points before the start of the stream."""
    for src, cl, pl, _dst in walk_frame(frame)[0]:
        if cl == pl or cl < 1:
            continue
        ll, at = frame[src] >> 4, src + 1                           # token, literal-length extension, literals, offset LE16
        if ll == 15:
            while at < src + cl:
                ll += frame[at]
                at += 1
                if frame[at - 1] != 255:
                    break
        pos = at + ll + 1
        if pos < src + cl and ll < 0xFF00 and frame[pos] != 0xFF:
            return frame[:pos] + b"\xff" + frame[pos + 1:]
    raise AssertionError("no LZ4 stream whose first sequence has a match")


# ---- corrupt frames ----------------------------------------------------------------------------------
def _patched(frame: bytes, at: int, data: bytes) -> bytes:
    return frame[:at] + data + frame[at + len(data):]


def corrupt_frames():
    """name -> (frame, "refused" | "host only")"""
    f, _ = _host_frame()
    cbytes = len(f)
    return {
        "short_header": (f[:10], "refused"),
        "cbytes_beyond_the_buffer": (f[:-5], "refused"),
        "bstarts_outside": (_patched(f, bc.HEADER + 4, (cbytes + 100).to_bytes(4, "little")), "refused"),
        "stream_length_outside": (_patched(f, bc.HEADER + 4 * 5, (cbytes + 1).to_bytes(4, "little")), "refused"),
        "bit_shuffle": (_patched(f, 2, bytes((f[2] | bc.F_BITSHUFFLE,))), "host only"),
        "other_codec": (_patched(f, 2, bytes(((f[2] & 0x1F) | (2 << 5),))), "host only"),
        "typesize_8": (_patched(f, 3, bytes((8,))), "host only"),
    }


# ---- the lenient walk (the rules of blosc_decompress in tm_io.hip), for the corpus -----------------------------
def walk_frame(frame: bytes):
    """-> (streams [(src offset, compressed length, plain length, offset in the shuffled image)], shuffled?, typesize, block size)"""
    flags, ts = frame[2], frame[3] or 1
    le32 = lambda o: int.from_bytes(frame[o:o + 4], "little")
    nbytes, bs, cbytes = le32(4), le32(8), le32(12)
    assert cbytes <= len(frame)
    if flags & bc.F_MEMCPY:
        return [(bc.HEADER, nbytes, nbytes, 0)], False, ts, max(nbytes, 1)
    nblocks, leftover = (nbytes + bs - 1) // bs, nbytes % bs
    out = []
    for j in range(nblocks):
        short = j == nblocks - 1 and leftover > 0
        bsize = leftover if short else bs
        ns = ts if (not flags & bc.F_DONT_SPLIT and bsize // ts >= 128 and not short) else 1
        ip = le32(bc.HEADER + 4 * j)
        for sp in range(ns):
            cb = le32(ip)
            ip += 4
            assert ip + cb <= cbytes
            out.append((ip, cb, bsize // ns, j * bs + sp * (bsize // ns)))
            ip += cb
    return out, bool(flags & bc.F_SHUFFLE) and ts > 1, ts, bs


def shuffled_image(plain: bytes, shuffled: bool, ts: int, bs: int) -> bytes:
    if not shuffled:
        return plain
    return b"".join(bc.shuffle_block(plain[o:o + bs], ts) for o in range(0, len(plain), bs))


def write_corpus(path):
    """Every stream of every good frame (with its plain bytes) and every stream of every corrupt-stream frame (the broken one
    marked).  Records: u32 name length, name, u32 expect (0 decodes, 1 must be refused), u32 clen, u32 plen, the stream, and
    for expect == 0 the plain bytes."""
    recs = []
    for name in GOOD_NAMES:
        frame, plain = good(name)
        streams, sh, ts, bs = walk_frame(frame)
        img = shuffled_image(plain, sh, ts, bs)
        for k, (src, cl, pl, dst) in enumerate(streams):
            recs.append((f"{name}#{k}", 0, frame[src:src + cl], pl, img[dst:dst + pl]))
    _, plain = _host_frame()
    for name in CORRUPT_STREAMS:
        frame = corrupt_stream_frame(name)
        streams, sh, ts, bs = walk_frame(frame)
        img = shuffled_image(plain, sh, ts, bs)
        for k, (src, cl, pl, dst) in enumerate(streams):
            recs.append((f"corrupt/{name}#{k}", int(k == 3), frame[src:src + cl], pl, img[dst:dst + pl]))
    with open(path, "wb") as f:
        f.write(b"TMBLZ4C1" + struct.pack("<I", len(recs)))
        for name, expect, comp, pl, plain in recs:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<III", expect, len(comp), pl) + comp)
            if not expect:
                assert len(plain) == pl
                f.write(plain)
    return len(recs)


# ---- chunk grids -------------------------------------------------------------------------------------
GRID_CASES = {"grid_6x40x48": ((6, 40, 48), (3, 40, 48)), "grid_5x40x48_clipped": ((5, 40, 48), (3, 40, 48)),
              "grid_clipped_rows_cols": ((4, 37, 50), (2, 20, 32))}


def grid_array(shape):
    r = bc._rng("grid" + "x".join(map(str, shape)))
    a = r.standard_normal(shape).astype(np.float16)
    a[:, : shape[1] // 2] = np.float16(-1.0)
    return a


def write_grid_zip(path, shape, chunks, blocksize=4096):
    """What zarr.save_array writes for an array of several chunks: every chunk full size (edge chunks padded with the fill
    value), one Blosc frame each, members '{i}.{j}.{k}' -> the array."""
    a = grid_array(shape)
    meta = {"chunks": list(chunks), "compressor": {"blocksize": 0, "clevel": 5, "cname": "lz4", "id": "blosc", "shuffle": 1}, "dtype": "<f2",
            "fill_value": 0.0, "filters": None, "order": "C", "shape": list(shape), "zarr_format": 2}
    grid = [range((s + c - 1) // c) for s, c in zip(shape, chunks)]
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as z:
        z.writestr(".zarray", json.dumps(meta, indent=4, sort_keys=True))
        for i in grid[0]:
            for j in grid[1]:
                for k in grid[2]:
                    blk = np.zeros(chunks, np.float16)
                    part = a[i * chunks[0]:(i + 1) * chunks[0], j * chunks[1]:(j + 1) * chunks[1], k * chunks[2]:(k + 1) * chunks[2]]
                    blk[:part.shape[0], :part.shape[1], :part.shape[2]] = part
                    z.writestr(f"{i}.{j}.{k}", bc.encode_frame(blk.tobytes(), 2, blocksize))
    return a


if __name__ == "__main__":
    print(f"{write_corpus(sys.argv[1])} streams -> {sys.argv[1]}")
