"""Tiled pyramidal OME-TIFF of one slice image.

The reference writes its stitched slices with libvips (infer_brn.py:11-54: `tiffsave(tile=True, compression='jpeg',
pyramid=True, bigtiff=True, tile_height=256, tile_width=256)` with a minimal OME-XML image description).  This module writes
the same kind of file without libvips: the 2 x 2 reductions and the JPEG tile scans are kernels of the library
(tm_u8_shrink2, tm_jpeg_encode_tiles) run on the resident uint8 plane, the container is a hand-written little-endian BigTIFF.

File layout: header (magic 43, 8-byte offsets), the tile data of every level in level / tile order, then one IFD per level as
successive pages (NewSubfileType 1 on the reduced ones), ImageDescription on the first page only.  Offsets and byte counts are
LONG8.  A JPEG tile is an abbreviated stream SOI SOF0 SOS <scan> EOI; the tables are in the JPEGTables tag
(tm_jpeg_tables: the statement the kernel encodes with).  The same pixels give the same file bytes.

Pinned: the JPEG bytes equal libjpeg's for the same tile and quality; the container is read back by libtiff through Pillow.
Not pinned: byte equality with a libvips-written file, libvips' level sizes at odd dimensions (here ceil(n / 2), the last
row / column repeated), and QuPath / Bio-Formats, which were never run on these files.

Colour pages (write_pyramid_rgb): the two-stain composite of utils/vis_mba.py:193-195 (PolyT green, DAPI blue), optionally
brightened and with an ontology image blended over it as onto_overlay does (:118-179), as pages of three samples: YCbCr 4:4:4
JPEG tiles (tm_jpeg_encode_tiles_rgb forms the composite in its block load; Photometric 6, YCbCrSubSampling 1 1).  4:4:4
because DAPI sits in blue, which weighs 0.114 in Y: nearly all of its detail is in Cb, and 4:2:0 would halve the nuclei's
resolution.  Pinned: the tile bytes equal libjpeg's for the composite at `subsampling=0`, Pillow / libtiff opens the pages as
RGB.  Not pinned: the blend rounding (ours: (ov alpha + v (255 - alpha) + 127) / 255; libvips' composite('over') was never
compared), the OME-XML channel element under Bio-Formats.
"""
import ctypes as C
import struct
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch

from . import _lib

TILE = 256
BATCH_TILES = 1024           # tiles per encode call and device-to-host copy
SLOT_BYTES = 65536           # bytes per tile slot of a batch; a tile that needs more is encoded again with a sized slot


def pyramid_sizes(H: int, W: int, tile: int = TILE) -> List[Tuple[int, int]]:
    """[(H, W), (ceil(H / 2), ceil(W / 2)), ...] down to the first level that fits in one tile (libvips' stopping rule)."""
    out = [(H, W)]
    while H > tile or W > tile:
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def ome_xml(W: int, H: int, samples: int = 1) -> str:
    """The image description of infer_brn.get_ome (infer_brn.py:32-48) for one band; samples = 3: one channel of three
    samples per pixel (the colour composite)."""
    if samples == 3:
        return ome_xml(W, H).replace('SizeC="1"', 'SizeC="3"').replace(
            '>\n            </Pixels>', '>\n                <Channel ID="Channel:0:0" SamplesPerPixel="3"/>\n            </Pixels>')
    return f"""<?xml version="1.0" encoding="UTF-8"?>
    <OME xmlns="http://www.openmicroscopy.org/Schemas/OME/2016-06"
        xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance"
        xsi:schemaLocation="http://www.openmicroscopy.org/Schemas/OME/2016-06 http://www.openmicroscopy.org/Schemas/OME/2016-06/ome.xsd">
        <Image ID="Image:0">
            <!-- Minimum required fields about image dimensions -->
            <Pixels DimensionOrder="XYCZT"
                    ID="Pixels:0"
                    SizeC="1"
                    SizeT="1"
                    SizeX="{W}"
                    SizeY="{H}"
                    SizeZ="1"
                    Type="uint8">
            </Pixels>
        </Image>
    </OME>"""


def jpeg_tables(quality: int) -> bytes:
    """SOI DQT DHT(DC) DHT(AC) EOI for `quality` (host only: needs no GPU)."""
    n = C.c_size_t(0)
    L = _lib.lib()
    _lib.check(L.tm_jpeg_tables(quality, None, 0, C.byref(n)), "tm_jpeg_tables")
    buf = (C.c_uint8 * n.value)()
    _lib.check(L.tm_jpeg_tables(quality, buf, n.value, C.byref(n)), "tm_jpeg_tables")
    return bytes(buf)


# SOI, SOF0 (8 bits, 256 x 256, one component 1, sampling 1 x 1, table 0), SOS (component 1, DC / AC table 0, 0 .. 63)
_TILE_HEAD = (b"\xff\xd8" + b"\xff\xc0" + struct.pack(">HBHHBBBB", 11, 8, TILE, TILE, 1, 1, 0x11, 0) +
              b"\xff\xda" + struct.pack(">HBBBBBB", 8, 1, 1, 0x00, 0, 63, 0))
_TILE_TAIL = b"\xff\xd9"


def jpeg_tile_stream(scan: bytes) -> bytes:
    """The abbreviated JPEG stream of one tile around its entropy-coded segment."""
    return _TILE_HEAD + scan + _TILE_TAIL


def jpeg_tables_rgb(quality: int) -> bytes:
    """SOI DQT(0) DQT(1) DHT(DC 0) DHT(AC 0) DHT(DC 1) DHT(AC 1) EOI for `quality`: the tables of the colour tiles (host only)."""
    n = C.c_size_t(0)
    L = _lib.lib()
    _lib.check(L.tm_jpeg_tables_rgb(quality, None, 0, C.byref(n)), "tm_jpeg_tables_rgb")
    buf = (C.c_uint8 * n.value)()
    _lib.check(L.tm_jpeg_tables_rgb(quality, buf, n.value, C.byref(n)), "tm_jpeg_tables_rgb")
    return bytes(buf)


# SOI, SOF0 (8 bits, 256 x 256, components 1 2 3 all sampled 1 x 1, quantisers 0 1 1), SOS (1 on DC / AC tables 0 / 0, 2 and 3
# on 1 / 1, 0 .. 63)
_TILE_HEAD_RGB = (b"\xff\xd8" + b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, TILE, TILE, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]) +
                  b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11]) + bytes([0, 63, 0]))


def jpeg_tile_stream_rgb(scan: bytes) -> bytes:
    """The abbreviated JPEG stream of one colour tile (three components, 4:4:4, one interleaved scan)."""
    return _TILE_HEAD_RGB + scan + _TILE_TAIL


# ---- BigTIFF container -------------------------------------------------------------------------------------------------
_SHORT, _LONG, _ASCII, _UNDEFINED, _LONG8 = 3, 4, 2, 7, 16
_FMT = {_SHORT: "<%dH", _LONG: "<%dI", _LONG8: "<%dQ"}


def encode_ifd(entries: Sequence[Tuple[int, int, object]], offset: int, next_ifd: int) -> bytes:
    """One BigTIFF IFD placed at file offset `offset`, with its out-of-line values right behind it.
    entries: (tag, type, value) in ascending tag order; value is bytes (ASCII / UNDEFINED) or a sequence of ints."""
    body = 8 + 20 * len(entries) + 8
    recs, extra = [], b""
    for tag, typ, val in entries:
        data = bytes(val) if typ in (_ASCII, _UNDEFINED) else struct.pack(_FMT[typ] % len(val), *val)
        count = len(data) if typ in (_ASCII, _UNDEFINED) else len(val)
        if len(data) <= 8:
            field = data.ljust(8, b"\0")
        else:
            field = struct.pack("<Q", offset + body + len(extra))
            extra += data + (b"\0" if len(data) & 1 else b"")      # values start on even offsets
        recs.append(struct.pack("<HHQ", tag, typ, count) + field)
    return struct.pack("<Q", len(entries)) + b"".join(recs) + struct.pack("<Q", next_ifd) + extra


def write_tiles(path, H: int, W: int, level_tiles: Callable[[int, int, int], Iterable[bytes]], compression: str = "jpeg",
                tables: Optional[bytes] = None, samples: int = 1) -> None:
    """Write the container around ready tile payloads.  level_tiles(level, h, w) yields the payload of every tile of that
    level, row-major: abbreviated JPEG streams (compression 'jpeg', with `tables`) or raw 256 x 256 tiles ('none').
    samples = 3: colour pages of YCbCr JPEG tiles (BitsPerSample 8 8 8, Photometric 6, SamplesPerPixel 3,
    PlanarConfiguration 1, YCbCrSubSampling 1 1), which libtiff hands back as RGB; JPEG only."""
    if compression not in ("jpeg", "none"):
        raise ValueError(f"compression must be 'jpeg' or 'none', got {compression!r}")
    if compression == "jpeg" and not tables:
        raise ValueError("JPEG tiles need their JPEGTables datastream")
    if samples not in (1, 3):
        raise ValueError(f"samples must be 1 or 3, got {samples}")
    if samples == 3 and compression != "jpeg":
        raise ValueError("colour pages (samples = 3) are written as YCbCr JPEG tiles only, not with compression 'none'")
    sizes = pyramid_sizes(H, W)
    with open(str(path), "wb") as f:
        f.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 0))                   # the first IFD's offset is patched below
        pos, levels = 16, []
        for lv, (h, w) in enumerate(sizes):
            offs, cnts = [], []
            for data in level_tiles(lv, h, w):
                if pos & 1:
                    f.write(b"\0")
                    pos += 1
                f.write(data)
                offs.append(pos)
                cnts.append(len(data))
                pos += len(data)
            want = ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
            if len(offs) != want:
                raise RuntimeError(f"level {lv} ({h} x {w}) has {want} tiles, got {len(offs)}")
            levels.append((offs, cnts))
        pos += f.write(b"\0" * (-pos % 8))
        first = pos
        for lv, ((h, w), (offs, cnts)) in enumerate(zip(sizes, levels)):
            e = [(254, _LONG, [1 if lv else 0]), (256, _LONG, [w]), (257, _LONG, [h]), (258, _SHORT, [8] * samples),
                 (259, _SHORT, [7 if compression == "jpeg" else 1]), (262, _SHORT, [6 if samples == 3 else 1])]
            if lv == 0:
                e.append((270, _ASCII, ome_xml(w, h, samples).encode() + b"\0"))
            e.append((277, _SHORT, [samples]))
            if samples == 3:
                e.append((284, _SHORT, [1]))
            e += [(322, _LONG, [TILE]), (323, _LONG, [TILE]), (324, _LONG8, offs), (325, _LONG8, cnts)]
            if compression == "jpeg":
                e.append((347, _UNDEFINED, tables))
            if samples == 3:
                e.append((530, _SHORT, [1, 1]))
            ifd = encode_ifd(e, pos, 0)
            ifd += b"\0" * (-len(ifd) % 8)
            if lv + 1 < len(sizes):                                          # the next IFD follows this one's values
                ifd = encode_ifd(e, pos, pos + len(ifd)).ljust(len(ifd), b"\0")
            f.write(ifd)
            pos += len(ifd)
        f.seek(8)
        f.write(struct.pack("<Q", first))


# ---- device side -------------------------------------------------------------------------------------------------------
def _check_plane(p: torch.Tensor) -> None:
    if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.uint8 and p.dim() == 2 and p.stride(1) == 1):
        raise ValueError("expected a 2-D uint8 device tensor with unit column stride")


def shrink2(src: torch.Tensor) -> torch.Tensor:
    """One pyramid level from the one above (tm_u8_shrink2)."""
    _check_plane(src)
    H, W = src.shape
    dst = torch.empty(((H + 1) // 2, (W + 1) // 2), dtype=torch.uint8, device=src.device)
    _lib.check(_lib.lib().tm_u8_shrink2(C.c_void_p(src.data_ptr()), H, W, src.stride(0), _lib.ptr(dst), dst.stride(0),
                                        _lib.current_stream_ptr()), "tm_u8_shrink2")
    return dst


def build_pyramid(plane: torch.Tensor) -> List[torch.Tensor]:
    """[plane, its 2 x 2 reduction, ...] at pyramid_sizes(H, W); about a third of the plane in extra device memory."""
    levels = [plane]
    for _ in pyramid_sizes(*plane.shape)[1:]:
        levels.append(shrink2(levels[-1]))
    return levels


class JpegBatches:
    """The buffers of one export: tile slots, need, packed bytes and offsets on the device, two pinned host landing areas."""

    def __init__(self, device, batch_tiles: int, slot_bytes: int):
        self.n, self.slot = batch_tiles, slot_bytes
        self.slots = torch.empty(batch_tiles * slot_bytes, dtype=torch.uint8, device=device)
        self.packed = torch.empty(batch_tiles * slot_bytes, dtype=torch.uint8, device=device)
        self.need = torch.empty(batch_tiles, dtype=torch.int32, device=device)
        self.offsets = torch.empty(batch_tiles + 1, dtype=torch.int64, device=device)
        self.host = torch.empty(batch_tiles * slot_bytes, dtype=torch.uint8).pin_memory()
        self.host_need = torch.empty(batch_tiles, dtype=torch.int32).pin_memory()
        self.host_off = torch.empty(batch_tiles + 1, dtype=torch.int64).pin_memory()

    def encode(self, plane: torch.Tensor, quality: int, tile0: int, n: int) -> List[bytes]:
        """Scans of tiles [tile0, tile0 + n) of `plane`: one encode + compaction call, one copy of the packed bytes."""
        H, W = plane.shape
        return self._encode("tm_jpeg_encode_tiles", (C.c_void_p(plane.data_ptr()), H, W, plane.stride(0)), plane.device,
                            quality, tile0, n)

    def encode_rgb(self, comp: "Composite", quality: int, tile0: int, n: int) -> List[bytes]:
        """Colour scans of tiles [tile0, tile0 + n) of the composite `comp` (one level), the same way."""
        return self._encode("tm_jpeg_encode_tiles_rgb", comp.args(), comp.device, quality, tile0, n)

    def _encode(self, name: str, src: tuple, device, quality: int, tile0: int, n: int) -> List[bytes]:
        """`src`: the leading arguments of entry point `name` that describe the source."""
        _lib.check(getattr(_lib.lib(), name)(*src, quality, tile0, n, _lib.ptr(self.slots), self.slot, _lib.ptr(self.need),
                                             _lib.ptr(self.packed), _lib.ptr(self.offsets), _lib.current_stream_ptr()), name)
        self.host_need[:n].copy_(self.need[:n], non_blocking=True)
        self.host_off[:n + 1].copy_(self.offsets[:n + 1], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        need, off = self.host_need[:n].tolist(), self.host_off[:n + 1].tolist()
        self.host[:off[n]].copy_(self.packed[:off[n]], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        buf = self.host.numpy()
        out = []
        for k in range(n):
            if need[k] <= self.slot:
                out.append(buf[off[k]:off[k] + need[k]].tobytes())
            else:
                out.append(self._oversize(name, src, device, quality, tile0 + k, need[k]))
        return out

    def _oversize(self, name: str, src: tuple, device, quality: int, tile: int, need: int) -> bytes:
        """A tile whose scan did not fit its slot, encoded again into a slot sized from `need`."""
        slot = torch.empty(need, dtype=torch.uint8, device=device)
        nd = torch.empty(1, dtype=torch.int32, device=device)
        _lib.check(getattr(_lib.lib(), name)(*src, quality, tile, 1, _lib.ptr(slot), need, _lib.ptr(nd), None, None,
                                             _lib.current_stream_ptr()), name)
        if int(nd.item()) != need:
            raise RuntimeError(f"tile {tile}: the scan took {int(nd.item())} bytes, the size query said {need}")
        return slot.cpu().numpy().tobytes()


def _raw_tiles(plane: torch.Tensor, tile0: int, n: int) -> List[bytes]:
    """Uncompressed 256 x 256 tiles [tile0, tile0 + n) of the plane's grid, the edge repeated (compression 'none': plumbing,
    not a hot path)."""
    H, W = plane.shape
    gx = (W + TILE - 1) // TILE
    ar = torch.arange(TILE, device=plane.device)
    out = []
    for t in range(tile0, tile0 + n):
        ys = (ar + (t // gx) * TILE).clamp_(max=H - 1)
        xs = (ar + (t % gx) * TILE).clamp_(max=W - 1)
        out.append(plane[ys][:, xs].cpu().numpy().tobytes())
    return out


def write_pyramid(path, plane, quality: int = 75, compression: str = "jpeg", batch_tiles: int = BATCH_TILES,
                  slot_bytes: int = SLOT_BYTES, buffers: Optional[JpegBatches] = None) -> List[torch.Tensor]:
    """Write uint8 device plane [H, W] (or the levels build_pyramid returned for it) as a tiled pyramidal BigTIFF.
    Returns the pyramid levels (device tensors)."""
    if compression not in ("jpeg", "none"):
        raise ValueError(f"compression must be 'jpeg' or 'none', got {compression!r}")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be 1 .. 100, got {quality}")
    levels = list(plane) if isinstance(plane, (list, tuple)) else None
    if levels is None:
        _check_plane(plane)
        levels = build_pyramid(plane)
    for p in levels:
        _check_plane(p)
    H, W = levels[0].shape
    if [tuple(p.shape) for p in levels] != pyramid_sizes(H, W):
        raise ValueError("the levels are not the pyramid of their first plane")
    bufs = None
    if compression == "jpeg":
        bufs = buffers or JpegBatches(levels[0].device, batch_tiles, slot_bytes)

    def level_tiles(lv, h, w):
        total = ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
        step = bufs.n if bufs else batch_tiles
        for t0 in range(0, total, step):
            n = min(step, total - t0)
            if bufs:
                for scan in bufs.encode(levels[lv], int(quality), t0, n):
                    yield jpeg_tile_stream(scan)
            else:
                yield from _raw_tiles(levels[lv], t0, n)

    write_tiles(path, H, W, level_tiles, compression, jpeg_tables(int(quality)) if compression == "jpeg" else None)
    return levels


# ---- colour composite --------------------------------------------------------------------------------------------------
class Composite:
    """The colour source of one level: (r, g, b) uint8 device planes of one size (entries may be None: all zeros, but not all
    three), brightness, and an optional uint8 [oh, ow, 3] device overlay blended with `alpha` / 255 where it is not black.
    The pixel rule is the library's (include/teramind_hip.h); nothing is computed here."""

    def __init__(self, planes: Sequence[Optional[torch.Tensor]], bright: float = 1.0, overlay: Optional[torch.Tensor] = None,
                 alpha: int = 100):
        planes = tuple(planes)
        given = [p for p in planes if p is not None]
        if len(planes) != 3 or not given:
            raise ValueError("a composite takes three planes (r, g, b), at least one of them given")
        for p in given:
            _check_plane(p)
            if p.shape != given[0].shape or p.device != given[0].device:
                raise ValueError("the planes of a composite have one size and one device")
        if overlay is not None and not (isinstance(overlay, torch.Tensor) and overlay.device == given[0].device and
                                        overlay.dtype == torch.uint8 and overlay.dim() == 3 and overlay.shape[2] == 3 and
                                        overlay.is_contiguous()):
            raise ValueError("the overlay is a contiguous uint8 [h, w, 3] tensor on the planes' device")
        self.planes, self.bright, self.overlay, self.alpha = planes, float(bright), overlay, int(alpha)
        self.H, self.W = given[0].shape
        self.device = given[0].device

    def args(self) -> tuple:
        """The source arguments of tm_rgb_compose / tm_jpeg_encode_tiles_rgb."""
        ptrs = (C.c_void_p * 3)(*[None if p is None else p.data_ptr() for p in self.planes])
        pitches = (C.c_int64 * 3)(*[0 if p is None else p.stride(0) for p in self.planes])
        ov = self.overlay
        return (ptrs, pitches, self.H, self.W, self.bright, _lib.ptr(ov), 0 if ov is None else ov.shape[0],
                0 if ov is None else ov.shape[1], self.alpha)

    def compose(self) -> torch.Tensor:
        """The composite as an interleaved uint8 [H, W, 3] device tensor (tm_rgb_compose)."""
        dst = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().tm_rgb_compose(*self.args(), _lib.ptr(dst), dst.stride(0), _lib.current_stream_ptr()),
                   "tm_rgb_compose")
        return dst


def write_pyramid_rgb(path, planes, quality: int = 75, bright: float = 1.0, overlay: Optional[torch.Tensor] = None,
                      alpha: int = 100, batch_tiles: int = BATCH_TILES, slot_bytes: int = 3 * SLOT_BYTES,
                      buffers: Optional[JpegBatches] = None) -> List[Composite]:
    """Write the composite of `planes` = (r, g, b) as a tiled pyramidal BigTIFF of colour pages.  Each entry is a uint8
    device plane [H, W], the levels build_pyramid returned for one, or None (all zeros).  Every given plane gets its own
    pyramid; a level is encoded from that level's stain planes, with brightness and overlay applied at that level (the
    overlay sampled by the level's own size), so no RGB image of a level is stored.  Returns the levels' Composite sources."""
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be 1 .. 100, got {quality}")
    pyr = []
    for p in planes:
        if p is None or isinstance(p, (list, tuple)):
            pyr.append(None if p is None else list(p))
        else:
            _check_plane(p)
            pyr.append(build_pyramid(p))
    given = [p for p in pyr if p is not None]
    if len(pyr) != 3 or not given:
        raise ValueError("a composite takes three planes (r, g, b), at least one of them given")
    H, W = given[0][0].shape
    for p in given:
        if [tuple(x.shape) for x in p] != pyramid_sizes(H, W):
            raise ValueError("the planes of a composite have one size, and levels are the pyramid of their first plane")
    levels = [Composite([None if p is None else p[lv] for p in pyr], bright, overlay, alpha) for lv in range(len(given[0]))]
    bufs = buffers or JpegBatches(levels[0].device, batch_tiles, slot_bytes)

    def level_tiles(lv, h, w):
        total = ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
        for t0 in range(0, total, bufs.n):
            for scan in bufs.encode_rgb(levels[lv], int(quality), t0, min(bufs.n, total - t0)):
                yield jpeg_tile_stream_rgb(scan)

    write_tiles(path, H, W, level_tiles, "jpeg", jpeg_tables_rgb(int(quality)), samples=3)
    return levels
