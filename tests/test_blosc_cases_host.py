"""CPU: the strict Blosc / LZ4 decoder of tests/blosc_cases.py reads what c-blosc writes and refuses what breaks a rule; the
case table of tests/test_gpu_blosc.py exercises what it claims (checked on the Python reference encoder); the host-only parts
of the encoder's C ABI (bound, argument refusals) and the container writer."""
import ctypes as C
import json
import zipfile

import numpy as np
import pytest

import blosc_cases as bc
import util
from teramind_amd import _lib, formats

FIXTURE_NAMES = ["f16_default", "f16_small_default", "f16_blocks64k_leftover", "f16_noshuffle", "f16_gauss", "f16_clevel0_memcpy",
                 "f16_tiny_nosplit", "f32_counts", "u8_random", "f16_clevel9_blocks"]


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_strict_decoder_reads_real_cblosc_frames(name):
    """The strict rules are the ones real c-blosc 1.21.0 / LZ4 streams obey (every frame of the fixture but the memcpyed one)."""
    plain, frame = bc.fixture(name)
    if frame[2] & bc.F_MEMCPY:
        with pytest.raises(bc.BloscError, match="memcpyed"):
            bc.parse_frame(frame)
        return
    got = bc.parse_frame(frame)
    assert got["plain"] == plain
    assert any(not stored for *_, stored in got["streams"]) or name in ("f16_gauss", "u8_random")


# ---- hand-made violations -------------------------------------------------------------------------
def _lz4(*seqs):
    out = bytearray()
    for lits, off, ml in seqs:
        bc._put_sequence(out, lits, off, ml)
    return bytes(out)


A = b"a"
GOOD_32 = _lz4((A, 1, 26), (A * 5, 0, 0))                      # 1 literal, a match to 5 before the end, 5 literals


def test_strict_lz4_accepts_the_baseline():
    assert bc.lz4_decode_strict(GOOD_32, 32) == A * 32
    assert bc.lz4_sequences(GOOD_32, 32)[1] == [(1, 1, 26), (5, 0, 0)]


@pytest.mark.parametrize("what,stream,n,msg", [
    ("a match reaching into the last 5 bytes", _lz4((A, 1, 27), (A * 4, 0, 0)), 32, "last 5 bytes"),
    ("a last match starting fewer than 12 bytes before the end", _lz4((A, 1, 40), (A * 12, 1, 4), (A * 7, 0, 0)), 64, "fewer than 12"),
    ("offset 0", bytes([0x1F, 0x61, 0, 0, 7, 0x50]) + A * 5, 32, "offset 0"),
    ("an offset beyond the produced bytes", _lz4((A, 2, 26), (A * 5, 0, 0)), 32, "beyond"),
    ("an LZ4 stream as long as the plain stream", _lz4((b"abcd", 4, 4), (b"0123456789AB", 0, 0)), 20, "shorter"),
    ("a match length on the last sequence", GOOD_32[:-6] + bytes([0x51]) + A * 5, 32, "last sequence"),
    ("a stream that decodes to fewer bytes", GOOD_32, 33, "decodes to"),
    ("a truncated stream", GOOD_32[:3], 32, "runs off"),
])
def test_strict_lz4_rejects(what, stream, n, msg):
    with pytest.raises(bc.BloscError, match=msg):
        bc.lz4_decode_strict(stream, n)


def _frame(flags=0x21, typesize=2, nbytes=None, blocksize=None, cbytes=None, bstarts=None, body=b"", tail=b""):
    nblocks = (nbytes + blocksize - 1) // blocksize
    if bstarts is None:
        bstarts = [16 + 4 * nblocks]
    table = b"".join(int(b).to_bytes(4, "little") for b in bstarts)
    total = 16 + len(table) + len(body) + len(tail) if cbytes is None else cbytes
    head = bytes((2, 1, flags, typesize)) + nbytes.to_bytes(4, "little") + blocksize.to_bytes(4, "little") + total.to_bytes(4, "little")
    return head + table + body + tail


def test_strict_frame_parser_rejects():
    plain = bc.mixed_bytes(512, "viol")
    good = bc.encode_frame(plain, 2, 256)                        # two split blocks
    got = bc.parse_frame(good)
    assert got["plain"] == plain and got["flags"] == 0x21 and len(got["streams"]) == 4
    body = good[24:]

    def bad(msg, **kw):
        args = dict(nbytes=512, blocksize=256, bstarts=got["bstarts"], body=body)
        args.update(kw)
        with pytest.raises(bc.BloscError, match=msg):
            bc.parse_frame(_frame(**args))

    assert bc.parse_frame(_frame(nbytes=512, blocksize=256, bstarts=got["bstarts"], body=body))["plain"] == plain
    bad("bstarts", bstarts=[got["bstarts"][0], got["bstarts"][1] + 1])          # a wrong bstarts entry
    bad("bstarts", bstarts=[got["bstarts"][0] + 4, got["bstarts"][1]])
    bad("cbytes", cbytes=len(good) + 1)                                             # a wrong cbytes
    bad("cbytes", cbytes=len(good) - 1)
    bad("flag 0x10", flags=0x31)                                                    # a split frame that carries "don't split"
    bad("after the last stream", tail=b"\0")                                        # trailing garbage, counted in cbytes
    bad("memcpyed", flags=0x23)
    bad("bit-shuffled", flags=0x25)
    bad("codec", flags=0x41)
    with pytest.raises(bc.BloscError, match="format version"):
        bc.parse_frame(b"\x03" + good[1:])
    with pytest.raises(bc.BloscError, match="cbytes"):
        bc.parse_frame(good + b"\0")                                                # trailing garbage behind the frame
    # an unsplit frame (100 elements) without the flag
    small = bc.encode_frame(bc.constant(200), 2, 256)
    assert small[2] == 0x31 and bc.decode_frame(small) == bc.constant(200)
    with pytest.raises(bc.BloscError, match="flag 0x10"):
        bc.parse_frame(small[:2] + b"\x21" + small[3:])
    # a stream that claims more bytes than its plain size
    with pytest.raises(bc.BloscError, match="stream of"):
        bc.parse_frame(_frame(flags=0x31, nbytes=200, blocksize=200, body=(201).to_bytes(4, "little") + bytes(201)))


# ---- the case table ---------------------------------------------------------------------------------
def _sequences(frame):
    out = []
    for _, _, n, data, stored in bc.parse_frame(frame)["streams"]:
        if not stored:
            out += bc.lz4_sequences(data, n)[1]
    return out


@pytest.mark.parametrize("name", list(bc.CASES))
def test_cases_round_trip_on_the_reference_encoder(name):
    make, ts, bs, _why = bc.CASES[name]
    data = make()
    frame = bc.encode_frame(data, ts, bs)
    assert bc.decode_frame(frame) == data
    assert len(frame) <= bc.bound(len(data), ts, bs)
    assert _lib.lib().tm_blosc_bound(len(data), ts, bs) == bc.bound(len(data), ts, bs)


def test_cases_exercise_what_they_claim():
    enc = lambda name: bc.encode_frame(bc.CASES[name][0](), *bc.CASES[name][1:3])
    flags = lambda name: enc(name)[2]
    # sizes: the split rule and its flag, leftovers
    assert flags("n200_ts2") == 0x31 and flags("n254_ts2") == 0x31 and flags("n256_ts2") == 0x21 and flags("n1_ts1") == 0x30
    assert [s[2] for s in bc.parse_frame(enc("n258_ts2"))["streams"]] == [128, 128, 2]
    assert [s[2] for s in bc.parse_frame(enc("n258_ts2_oneblock"))["streams"]] == [129, 129]
    assert [s[2] for s in bc.parse_frame(enc("block_plus3_ts2"))["streams"]] == [2048, 2048, 3]
    assert [s[2] for s in bc.parse_frame(enc("block_plus3_ts4"))["streams"]] == [1024] * 4 + [3]
    assert [s[2] for s in bc.parse_frame(enc("blocks4_leftover"))["streams"]] == [2048] * 8 + [1002]
    assert [s[2] for s in bc.parse_frame(enc("stream64k"))["streams"]] == [65536]
    assert all(s[4] for s in bc.parse_frame(enc("n12"))["streams"])                         # stored
    # content
    seqs = _sequences(enc("const_32k"))
    assert seqs == [(1, 1, 32768 - 5 - 1), (5, 0, 0)] and len(enc("const_32k")) <= 16 + 4 + 4 + 256
    assert set(bc.EXT_MATCH_LENGTHS) <= {ml for _, _, ml in _sequences(enc("ext_runs"))}
    assert set(bc.LITERAL_RUNS) <= {ll for ll, off, _ in _sequences(enc("literal_runs")) if off}
    assert set(bc.OFFSETS) <= {off for _, off, _ in _sequences(enc("offsets")) if off}
    rnd = bc.parse_frame(enc("random"))
    assert all(s[4] for s in rnd["streams"]) and len(enc("random")) == bc.bound(2 * 4096 + 6, 2, 4096)
    assert [s[4] for s in bc.parse_frame(enc("smooth_f16"))["streams"]] == [True, False]     # low bytes stored, high bytes compressed
    assert _sequences(enc("tail_only")) == [(201, 1, 10), (5, 0, 0)]                         # the one match lies in the last 16 bytes


# ---- host-only parts of the C ABI ----------------------------------------------------------------------
def test_bound_and_argument_refusals_without_device():
    """Everything outside the accepted arguments is TM_ERR_ARG with a reason before any device call: the pointers are host memory."""
    L = _lib.lib()
    assert L.tm_blosc_bound(13107200, 2, 65536) == 16 + 4 * 200 + 4 * 400 + 13107200          # a state tile
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    for nbytes, ts, bs, word in [(0, 2, 65536, b"nbytes"), (100, 3, 65536, b"typesize"), (100, 8, 65536, b"typesize"),
                                 (100, 2, 128, b"blocksize"), (100, 2, 65540, b"blocksize"), (100, 2, 258, b"blocksize"),
                                 (2 ** 31, 2, 65536, b"2^31")]:
        assert L.tm_blosc_bound(nbytes, ts, bs) == 0 and word in L.tm_last_error()
        assert L.tm_blosc_compress(p, nbytes, ts, bs, p, 4096, p, None) == -1 and word in L.tm_last_error()
    assert L.tm_blosc_compress(None, 100, 2, 256, p, 4096, p, None) == -1 and b"null" in L.tm_last_error()
    assert L.tm_blosc_compress(p, 100, 2, 256, p, 4096, None, None) == -1 and b"null" in L.tm_last_error()
    assert L.tm_blosc_compress(p, 1000, 2, 256, p, 1000, p, None) == -1 and b"bound" in L.tm_last_error()
    org = (C.c_int64 * 2)(0, 16)
    o = C.cast(org, C.c_void_p)
    base = dict(canvas=p, dtype=2, elems=1024, C=2, TH=8, TW=16, cs=512, pitch=32, org=o, org_h=o, n=2, packed=p, cap=4096, offs=p, st=None)
    tiles = lambda **kw: L.tm_blosc_compress_tiles(*{**base, **kw}.values())
    for kw, word in [(dict(canvas=None), b"null"), (dict(org_h=None), b"null"), (dict(offs=None), b"null"), (dict(dtype=1), b"dtype"),
                     (dict(C=0), b"positive"), (dict(n=0), b"ntiles"), (dict(n=65536), b"ntiles"), (dict(pitch=15), b"pitch"),
                     (dict(cs=200), b"channel stride"), (dict(elems=767), b"leaves the canvas"), (dict(cap=1000), b"packed buffer"),
                     (dict(canvas=C.c_void_p(p.value + 1)), b"aligned")]:
        assert tiles(**kw) == -1 and word in L.tm_last_error(), kw
    org[1] = -1
    assert tiles() == -1 and b"leaves the canvas" in L.tm_last_error()


def test_blosc_container_writer(tmp_path):
    """write_zarr_zip_blosc: the metadata zarr writes (the fixture's, apart from shape and chunks), one stored chunk, read back
    through read_zarr_zip and the c-blosc-pinned decoder."""
    a = np.frombuffer(bc.half_background(3 * 8 * 16), "<f2").reshape(3, 8, 16)
    frame = bc.encode_frame(a.tobytes(), 2, 65536)
    path = tmp_path / "t.zip"
    formats.write_zarr_zip_blosc(path, a.shape, "<f2", frame, date_time=(2024, 1, 2, 3, 4, 6))
    assert np.array_equal(formats.read_zarr_zip(path).view(np.uint16), a.view(np.uint16))
    with zipfile.ZipFile(path) as z, zipfile.ZipFile(util.ROOT + "/tests/golden/io_state_tile_blosc.zip") as ref:
        assert z.namelist() == [".zarray", "0.0.0"] and z.read("0.0.0") == frame
        meta, want = json.loads(z.read(".zarray")), json.loads(ref.read(".zarray"))
        assert z.read(".zarray") == json.dumps(meta, indent=4, sort_keys=True).encode()
        for i, r in zip(z.infolist(), ref.infolist()):
            assert (i.compress_type, i.external_attr) == (r.compress_type, r.external_attr) and i.date_time == (2024, 1, 2, 3, 4, 6)
    assert meta.pop("shape") == [3, 8, 16] and meta.pop("chunks") == [3, 8, 16]
    want.pop("shape"), want.pop("chunks")
    assert meta == want
    with pytest.raises(ValueError):
        formats.write_zarr_zip_blosc(path, (3, 8, 17), "<f2", frame)
