"""Blosc-1 / LZ4 frames of the snapshot encoder: a strict frame parser, a strict LZ4 block decoder, a greedy reference
encoder in pure Python, the data makers and the case table of tests/test_gpu_blosc.py (no GPU here).

The strict decoder enforces what `LZ4_decompress_safe` and c-blosc's `blosc_decompress` check or assume and what the
project's lenient decoder (tm_blosc_decompress) does not:
  frame   16-byte header (version 2, lz4 format 1, flags out of {0x01 shuffle, 0x10 don't split, codec lz4 = 0x20}),
          cbytes == len(frame), bstarts[0] == 16 + 4 nblocks, every block where the previous one ended, blocks split into
          `typesize` streams iff blocksize / typesize >= 128 -- and then flag 0x10 is clear, else set --, a short last block
          never split, no byte after the last stream;
  stream  length == plain size: stored.  Anything else is an LZ4 block that is SHORTER than the plain size and decodes to it;
  LZ4     [token][literal-length extension][literals][offset LE16][match-length extension], extensions are runs of 255 ended
          by a byte below 255, minimum match 4, 1 <= offset <= bytes produced so far, the last sequence has literals only,
          no match reaches into the last 5 bytes, no match starts in the last 12 bytes.
"""
import numpy as np

HEADER = 16
MIN_SPLIT_ELEMS = 128            # BLOSC_MIN_BUFFERSIZE
LASTLITERALS, MFLIMIT = 5, 12
F_SHUFFLE, F_MEMCPY, F_BITSHUFFLE, F_DONT_SPLIT, F_LZ4 = 0x01, 0x02, 0x04, 0x10, 0x20


class BloscError(ValueError):
    pass


def _need(cond, msg):
    if not cond:
        raise BloscError(msg)


# ---- LZ4 ----------------------------------------------------------------------------------------
def lz4_sequences(src: bytes, n: int):
    """Strict decode of one LZ4 block that must give exactly n bytes -> (plain, [(literals, offset, match length)]);
    the last entry has offset 0 and match length 0."""
    src = bytes(src)
    out = bytearray()
    seqs = []
    ip, end = 0, len(src)
    _need(end > 0, "empty LZ4 block")
    while True:
        _need(ip < end, "LZ4 block ends where a token is due")
        tok = src[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                _need(ip < end, "literal-length extension runs off the block")
                b = src[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        _need(ip + ll <= end, "literals run off the block")
        out += src[ip:ip + ll]
        ip += ll
        if ip == end:                                   # the last sequence: literals only
            _need((tok & 15) == 0, "last sequence carries a match length")
            seqs.append((ll, 0, 0))
            break
        _need(ip + 2 <= end, "offset runs off the block")
        off = src[ip] | (src[ip + 1] << 8)
        ip += 2
        _need(off >= 1, "offset 0")
        _need(off <= len(out), f"offset {off} beyond the {len(out)} bytes produced")
        ml = tok & 15
        if ml == 15:
            while True:
                _need(ip < end, "match-length extension runs off the block")
                b = src[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        start = len(out)
        _need(start <= n - MFLIMIT, f"match starts at {start}, fewer than {MFLIMIT} bytes before the end {n}")
        _need(start + ml <= n - LASTLITERALS, f"match [{start}, {start + ml}) reaches into the last {LASTLITERALS} bytes of {n}")
        if off >= ml:
            out += out[start - off:start - off + ml]
        else:                                           # overlapping copies are the RLE case: the last `off` bytes repeat
            out += (bytes(out[start - off:start]) * (ml // off + 1))[:ml]
        seqs.append((ll, off, ml))
    _need(len(out) == n, f"LZ4 block decodes to {len(out)} bytes, expected {n}")
    return bytes(out), seqs


def lz4_decode_strict(src: bytes, n: int) -> bytes:
    """A stream of a frame that is not stored: strict LZ4, and shorter than its plain size (length == plain size means stored)."""
    _need(len(src) < n, f"LZ4 stream of {len(src)} bytes is not shorter than its {n} plain bytes")
    return lz4_sequences(src, n)[0]


def _put_len(out: bytearray, v: int):
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)


def _put_sequence(out: bytearray, lits: bytes, off: int, ml: int):
    ll = len(lits)
    m = ml - 4 if off else 0
    out.append((min(ll, 15) << 4) | min(m, 15))
    if ll >= 15:
        _put_len(out, ll - 15)
    out += lits
    if off:
        out += bytes((off & 255, off >> 8))
        if m >= 15:
            _put_len(out, m - 15)


def lz4_greedy(s: bytes) -> bytes:
    """Reference encoder: greedy parse, every position inserted, the most recent earlier occurrence of the 4 bytes (exact: a
    dict, no hash collisions), strict end-of-block rules.  May return more than len(s) bytes (the caller stores the stream)."""
    s = bytes(s)
    n = len(s)
    out = bytearray()
    last = {}
    anchor = ip = 0
    while ip <= n - MFLIMIT:
        key = s[ip:ip + 4]
        c = last.get(key)
        last[key] = ip
        if c is None or ip - c > 65535:
            ip += 1
            continue
        ml = 4
        while ip + ml < n - LASTLITERALS and s[c + ml] == s[ip + ml]:
            ml += 1
        _put_sequence(out, s[anchor:ip], ip - c, ml)
        for q in range(ip + 1, min(ip + ml, n - MFLIMIT + 1)):
            last[s[q:q + 4]] = q
        ip += ml
        anchor = ip
    _put_sequence(out, s[anchor:], 0, 0)
    return bytes(out)


# ---- frames -------------------------------------------------------------------------------------
def effective_blocksize(nbytes: int, typesize: int, blocksize: int) -> int:
    bs = min(blocksize, nbytes)
    if bs > typesize:
        bs -= bs % typesize
    return bs


def geometry(nbytes: int, typesize: int, blocksize: int):
    """-> (effective block size, nblocks, leftover bytes, split?)"""
    bs = effective_blocksize(nbytes, typesize, blocksize)
    return bs, (nbytes + bs - 1) // bs, nbytes % bs, bs // typesize >= MIN_SPLIT_ELEMS


def bound(nbytes: int, typesize: int, blocksize: int) -> int:
    """16 + 4 nblocks + 4 (number of streams) + nbytes: every stream stored."""
    bs, nblocks, leftover, split = geometry(nbytes, typesize, blocksize)
    nfull = nbytes // bs
    return HEADER + 4 * nblocks + 4 * (nfull * (typesize if split else 1) + (1 if leftover else 0)) + nbytes


def shuffle_block(blk: bytes, typesize: int) -> bytes:
    nel = len(blk) // typesize
    a = np.frombuffer(blk, np.uint8)
    return a[:nel * typesize].reshape(nel, typesize).T.tobytes() + a[nel * typesize:].tobytes()


def unshuffle_block(blk: bytes, typesize: int) -> bytes:
    nel = len(blk) // typesize
    a = np.frombuffer(blk, np.uint8)
    return a[:nel * typesize].reshape(typesize, nel).T.tobytes() + a[nel * typesize:].tobytes()


def parse_frame(frame: bytes):
    """Strict parse -> dict(plain, flags, typesize, nbytes, blocksize, bstarts, streams), streams = [(block, split, plain
    size, stream bytes, stored?)].  Raises BloscError at the first rule a frame breaks."""
    frame = bytes(frame)
    _need(len(frame) >= HEADER, "frame shorter than its header")
    _need(frame[0] == 2, f"format version {frame[0]}, expected 2")
    _need(frame[1] == 1, f"lz4 format version {frame[1]}, expected 1")
    flags, typesize = frame[2], frame[3]
    le32 = lambda o: int.from_bytes(frame[o:o + 4], "little")
    nbytes, blocksize, cbytes = le32(4), le32(8), le32(12)
    _need(cbytes == len(frame), f"cbytes {cbytes} but the frame has {len(frame)} bytes")
    _need(not flags & F_MEMCPY, "memcpyed frame")
    _need(not flags & F_BITSHUFFLE, "bit-shuffled frame")
    _need(flags & ~(F_SHUFFLE | F_DONT_SPLIT) == F_LZ4, f"flags {flags:#x}: codec is not lz4, or unknown bits")
    _need(typesize >= 1 and nbytes >= 1, "typesize / nbytes must be positive")
    _need(1 <= blocksize <= nbytes, f"block size {blocksize} outside [1, nbytes]")
    _need(blocksize <= typesize or blocksize % typesize == 0, "block size is not a multiple of the typesize")
    nblocks, leftover = (nbytes + blocksize - 1) // blocksize, nbytes % blocksize
    split = typesize <= 16 and blocksize // typesize >= MIN_SPLIT_ELEMS
    _need(split == (not flags & F_DONT_SPLIT), f"blocks of {blocksize // typesize} elements are {'split' if split else 'not split'}"
          f" but flag 0x10 is {'set' if flags & F_DONT_SPLIT else 'clear'}")
    _need(HEADER + 4 * nblocks <= cbytes, "block table truncated")
    bstarts = [le32(HEADER + 4 * j) for j in range(nblocks)]
    ip = HEADER + 4 * nblocks
    plain, streams = bytearray(), []
    for j in range(nblocks):
        _need(bstarts[j] == ip, f"bstarts[{j}] = {bstarts[j]}, the block starts at {ip}")
        bsize = leftover if (j == nblocks - 1 and leftover) else blocksize
        nsplits = typesize if (split and bsize == blocksize) else 1
        neblock = bsize // nsplits
        blk = bytearray()
        for sp in range(nsplits):
            _need(ip + 4 <= cbytes, "stream length out of range")
            cb = le32(ip)
            ip += 4
            _need(1 <= cb <= neblock, f"stream of {cb} bytes for {neblock} plain bytes")
            _need(ip + cb <= cbytes, "stream out of range")
            data = frame[ip:ip + cb]
            ip += cb
            blk += data if cb == neblock else lz4_decode_strict(data, neblock)
            streams.append((j, sp, neblock, data, cb == neblock))
        plain += unshuffle_block(bytes(blk), typesize) if (flags & F_SHUFFLE and typesize > 1) else blk
    _need(ip == cbytes, f"{cbytes - ip} bytes after the last stream")
    return dict(plain=bytes(plain), flags=flags, typesize=typesize, nbytes=nbytes, blocksize=blocksize, bstarts=bstarts, streams=streams)


def decode_frame(frame: bytes) -> bytes:
    return parse_frame(frame)["plain"]


def encode_frame(plain: bytes, typesize: int, blocksize: int, lz4=lz4_greedy) -> bytes:
    """The frame rules of the encoder in Python (reference encoder for the streams): what the case checks run on the CPU."""
    plain = bytes(plain)
    nbytes = len(plain)
    bs, nblocks, leftover, split = geometry(nbytes, typesize, blocksize)
    flags = F_LZ4 | (F_SHUFFLE if typesize > 1 else 0) | (0 if split else F_DONT_SPLIT)
    body, bstarts = bytearray(), []
    for j in range(nblocks):
        bstarts.append(HEADER + 4 * nblocks + len(body))
        blk = plain[j * bs:(j + 1) * bs]
        if typesize > 1:
            blk = shuffle_block(blk, typesize)
        nsplits = typesize if (split and len(blk) == bs) else 1
        ne = len(blk) // nsplits
        for sp in range(nsplits):
            s = blk[sp * ne:(sp + 1) * ne]
            c = lz4(s)
            if len(c) >= len(s):
                c = s
            body += len(c).to_bytes(4, "little") + c
    cbytes = HEADER + 4 * nblocks + len(body)
    head = bytes((2, 1, flags, typesize)) + nbytes.to_bytes(4, "little") + bs.to_bytes(4, "little") + cbytes.to_bytes(4, "little")
    return head + b"".join(b.to_bytes(4, "little") for b in bstarts) + bytes(body)


# ---- data ----------------------------------------------------------------------------------------
def _rng(tag: str):
    return np.random.default_rng(int.from_bytes(tag.encode(), "little") % (2 ** 63))


def random_bytes(n: int, tag: str = "rnd") -> bytes:
    return _rng(f"{tag}{n}").integers(0, 256, n, dtype=np.uint8).tobytes()


def unique_bytes(n: int, tag: str = "uniq") -> bytes:
    """n bytes in which no 4-byte group occurs twice: positions counted in base 200 behind a marker byte, so that a repeat
    found in a construction is one the construction placed.  Values 200 .. 254 do not occur: free for separators."""
    assert n <= 4 * 200 ** 3
    k = np.arange((n + 3) // 4, dtype=np.int64)
    perm = _rng(tag).permutation(200)
    a = np.stack([np.full_like(k, 255), perm[k % 200], perm[(k // 200) % 200], perm[(k // 40000) % 200]], 1).astype(np.uint8)
    return a.tobytes()[:n]


def mixed_bytes(n: int, tag: str = "mix") -> bytes:
    """Compressible but not trivially: short repeats at many distances, runs, and noise between them."""
    r = _rng(f"{tag}{n}")
    out = bytearray()
    while len(out) < n:
        kind = r.integers(0, 4)
        if kind == 0 or len(out) < 8:
            out += r.integers(0, 256, int(r.integers(1, 24)), dtype=np.uint8).tobytes()
        elif kind == 1:
            out += bytes([int(r.integers(0, 256))]) * int(r.integers(4, 80))
        else:
            d = int(r.integers(1, min(len(out), 5000) + 1))
            ln = int(r.integers(4, 60))
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out[:n])


def constant(n: int) -> bytes:
    return b"\xbc" * n


def ext_boundary_runs() -> bytes:
    """Constant runs between unique bytes: a run of R bytes is one match of R - 1 (offset 1), R - 1 - 19 = 254, 0, 1 mod 255."""
    u = unique_bytes(4096, "ext")
    out, k = bytearray(), 0
    for i, ml in enumerate((18, 19, 20, 273, 274, 275, 528, 529, 530)):
        out += u[k:k + 24]
        k += 24
        out += bytes([201 + i]) * (ml + 1)
    return bytes(out + u[k:k + 24])


EXT_MATCH_LENGTHS = (18, 19, 20, 273, 274, 275, 528, 529, 530)     # 18: the token alone; 19: the first extension byte (0)
LITERAL_RUNS = (14, 15, 16, 269, 270, 271)


def literal_runs() -> bytes:
    """A 32-byte marker twice (more than a round of the encoder apart), then for each L: L bytes found nowhere else and the marker again -- literal runs of exactly L
    between matches of exactly 32 (every run starts and ends with a byte of its own, so no match grows into it)."""
    u = unique_bytes(4096, "lit")
    marker = bytes(range(1, 33))
    out, k = bytearray(marker + b"\xe6" + u[:100] + b"\xe7" + marker), 100
    for i, L in enumerate(LITERAL_RUNS):
        out += bytes([200 + i]) + u[k:k + L - 2] + bytes([220 + i]) + marker
        k += L
    return bytes(out + b"\xe8" + u[k:k + 24])


OFFSETS = (1, 4, 63, 64, 65, 4095, 65524)


def offset_pattern() -> bytes:
    """65536 unique bytes with 64-byte copies (enough to pay for the literal-length bytes of 64 KiB of literals) placed 1, 4, 63, 64, 65 and 4095 bytes behind their source, and one at the
    largest distance a stream of 65536 bytes admits: a match starts at most 12 bytes before the end, so 65524 (65535 would
    need a match that starts at the last byte)."""
    s = bytearray(unique_bytes(65536, "off"))
    p = 5000
    for d in OFFSETS[:-1]:
        for k in range(64):
            s[p + k] = s[p + k - d]
        p += 5000
    for k in range(7):                                      # [65524, 65531) = [0, 7): ends 5 bytes before the end
        s[65524 + k] = s[k]
    return bytes(s)


def smooth_f16_noisy(nel: int) -> bytes:
    """Smooth signal (exponent and top mantissa bits move slowly: the high bytes repeat) with noise over the low 8 mantissa bits."""
    r = _rng("smooth")
    x = np.arange(nel)
    hi = (0x3C00 + 0x100 * ((x // 97) % 3)).astype(np.uint16)
    return (hi | r.integers(0, 256, nel).astype(np.uint16)).astype("<u2").tobytes()


def tail_only(n: int = 200) -> bytes:
    return random_bytes(n, "tail") + b"\x07" * 16


def half_background(nel: int) -> bytes:
    """The shape of a state tile: half constant background (-1), half smooth signal with noisy mantissas."""
    a = np.full(nel, -1.0, np.float16).view(np.uint16)
    a[nel // 2:] = np.frombuffer(smooth_f16_noisy(nel - nel // 2), "<u2")
    return a.astype("<u2").tobytes()


# name -> (data maker, typesize, blocksize, what the case is there for)
CASES = {
    # sizes
    "n1_ts1": (lambda: b"\x55", 1, 256, "one byte: a 1-byte block, stored"),
    "n1_ts2": (lambda: b"\x55", 2, 256, "one byte at typesize 2: block below the typesize, no whole element to shuffle"),
    "n1_ts4": (lambda: b"\x55", 4, 256, "one byte at typesize 4"),
    "n12": (lambda: constant(12), 1, 256, "12 bytes: below the 13 an LZ4 block needs for a match, stored"),
    "n13": (lambda: constant(13), 1, 256, "13 bytes: the shortest stream a match fits in"),
    "n200_ts2": (lambda: constant(200), 2, 256, "100 elements: unsplit, flag 0x10, one compressible stream"),
    "n254_ts2": (lambda: mixed_bytes(254), 2, 256, "127 elements: just below the split rule"),
    "n256_ts2": (lambda: mixed_bytes(256), 2, 256, "128 elements: the smallest split block"),
    "n258_ts2": (lambda: mixed_bytes(258), 2, 256, "one split block of 128 elements and a 2-byte leftover"),
    "n258_ts2_oneblock": (lambda: mixed_bytes(258), 2, 65536, "129 elements in one split block"),
    "block_exact": (lambda: mixed_bytes(4096), 2, 4096, "exactly one block"),
    "block_plus2": (lambda: mixed_bytes(4098), 2, 4096, "one block + 2: a one-element leftover"),
    "block_plus3_ts2": (lambda: mixed_bytes(4099), 2, 4096, "one block + 3: leftover of one element and one odd byte"),
    "block_plus3_ts4": (lambda: mixed_bytes(4099), 4, 4096, "one block + 3 at typesize 4: leftover below the typesize"),
    "blocks4_leftover": (lambda: mixed_bytes(4 * 4096 + 1002), 2, 4096, "four blocks and a leftover (the shape of f16_blocks64k_leftover)"),
    "ts4_blocks": (lambda: mixed_bytes(3 * 1024), 4, 1024, "typesize 4: four streams per block"),
    "stream64k": (lambda: mixed_bytes(65536), 1, 65536, "a 65536-byte stream: positions up to 65535"),
    "stream64k_x2": (lambda: mixed_bytes(2 * 65536 + 7), 1, 65536, "two 65536-byte streams and a 7-byte leftover"),
    # content
    "const_32k": (lambda: constant(32768), 1, 32768, "constant: one match to the end (at most 256 bytes)"),
    "ext_runs": (ext_boundary_runs, 1, 4096, "match lengths at the 255-extension boundaries"),
    "literal_runs": (literal_runs, 1, 4096, "literal runs of 14, 15, 16, 269, 270, 271 between matches"),
    "offsets": (offset_pattern, 1, 65536, "repeats 1, 4, 63, 64, 65, 4095 and 65524 bytes back only"),
    "random": (lambda: random_bytes(2 * 4096 + 6), 2, 4096, "uniform random bytes: every stream stored, frame == bound"),
    "smooth_f16": (lambda: smooth_f16_noisy(32768), 2, 65536, "smooth fp16, noisy mantissas: high bytes compressed, low bytes stored"),
    "tail_only": (tail_only, 1, 4096, "compressible in its last 16 bytes only: the end-of-block rules"),
    "half_background": (lambda: half_background(3 * 32768), 2, 65536, "half background, half signal: three state-tile blocks"),
}

# fixture buffers (tests/golden/io_blosc_frames.npz) the encoder can be called on with c-blosc's own block size; the flag
# byte differs from c-blosc's where the fixture asked c-blosc for something the encoder does not offer
FIXTURE_CASES = {
    "f16_small_default": 0, "f16_blocks64k_leftover": 0, "f16_gauss": 0, "f16_tiny_nosplit": 0, "f16_clevel9_blocks": 0,
    "f16_noshuffle": F_SHUFFLE,          # c-blosc was told not to shuffle
    "f16_clevel0_memcpy": F_MEMCPY,      # clevel 0: c-blosc copies; no bstarts in its frame
    "u8_random": F_SHUFFLE,              # c-blosc sets the shuffle flag at typesize 1 too (a no-op there)
}
# c-blosc frame sizes the compression strength is held against (<= 1.15 x): same buffer; c-blosc's block size where the
# encoder takes it, 65536 for f16_default (c-blosc used 262144 there: larger blocks, so its frame is no larger for it)
RATIO_CASES = {"f16_default": 65536, "f16_small_default": None, "f16_blocks64k_leftover": None, "f16_clevel9_blocks": None}


def fixture(name: str):
    """-> (plain bytes, c-blosc frame bytes) of tests/golden/io_blosc_frames.npz"""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io_blosc_frames.npz")) as z:
        return z[f"{name}/plain"].tobytes(), z[f"{name}/frame"].tobytes()
