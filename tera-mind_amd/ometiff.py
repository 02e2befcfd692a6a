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


def ome_xml(W: int, H: int) -> str:
    """The image description of infer_brn.get_ome (infer_brn.py:32-48) for one band."""
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
                tables: Optional[bytes] = None) -> None:
    """Write the container around ready tile payloads.  level_tiles(level, h, w) yields the payload of every tile of that
    level, row-major: abbreviated JPEG streams (compression 'jpeg', with `tables`) or raw 256 x 256 tiles ('none')."""
    if compression not in ("jpeg", "none"):
        raise ValueError(f"compression must be 'jpeg' or 'none', got {compression!r}")
    if compression == "jpeg" and not tables:
        raise ValueError("JPEG tiles need their JPEGTables datastream")
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
            e = [(254, _LONG, [1 if lv else 0]), (256, _LONG, [w]), (257, _LONG, [h]), (258, _SHORT, [8]),
                 (259, _SHORT, [7 if compression == "jpeg" else 1]), (262, _SHORT, [1])]
            if lv == 0:
                e.append((270, _ASCII, ome_xml(w, h).encode() + b"\0"))
            e += [(277, _SHORT, [1]), (322, _LONG, [TILE]), (323, _LONG, [TILE]), (324, _LONG8, offs), (325, _LONG8, cnts)]
            if compression == "jpeg":
                e.append((347, _UNDEFINED, tables))
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
        L = _lib.lib()
        _lib.check(L.tm_jpeg_encode_tiles(C.c_void_p(plane.data_ptr()), H, W, plane.stride(0), quality, tile0, n,
                                          _lib.ptr(self.slots), self.slot, _lib.ptr(self.need), _lib.ptr(self.packed),
                                          _lib.ptr(self.offsets), _lib.current_stream_ptr()), "tm_jpeg_encode_tiles")
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
                out.append(self._oversize(plane, quality, tile0 + k, need[k]))
        return out

    def _oversize(self, plane: torch.Tensor, quality: int, tile: int, need: int) -> bytes:
        """A tile whose scan did not fit its slot, encoded again into a slot sized from `need`."""
        H, W = plane.shape
        slot = torch.empty(need, dtype=torch.uint8, device=plane.device)
        nd = torch.empty(1, dtype=torch.int32, device=plane.device)
        _lib.check(_lib.lib().tm_jpeg_encode_tiles(C.c_void_p(plane.data_ptr()), H, W, plane.stride(0), quality, tile, 1,
                                                   _lib.ptr(slot), need, _lib.ptr(nd), None, None,
                                                   _lib.current_stream_ptr()), "tm_jpeg_encode_tiles")
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
