"""On-disk formats either side of the denoising path.

The reference moves every tile through the filesystem each diffusion step:
  * gene tile  = `sparse.save_npz` COO archive named '{r0}_{r1}_{c0}_{c1}_{R0}_{R1}_{C0}_{C1}.npz'
    (inner ROI + ROI padded by 128 px; test_brn.py:51-70, utils/MBADataset_tst.py:65-79), shape
    [512, 512, 50*500];
  * state tile = `zarr.save_array('{r0}_{r1}_{c0}_{c1}.zip', out)` (test_brn.py:222-226): a zarr-v2 array
    in a ZipStore, float16 [100, 256, 256], channel order (stain, z); read back with `zarr.load`
    (utils/MBADataset_tst.py:60, infer_brn.py:76).
This build keeps the state resident (brain.TileSweep) and only touches these formats at the edges:
reading gene tiles, importing / exporting a step directory for interoperability and resume.

Neither `zarr`, `numcodecs` nor `sparse` exist in this image, so both containers are restated from
their published layouts (zarr storage spec v2; pydata/sparse 0.15.5 `save_npz`; c-blosc 1.x frames):
  * readers accept what zarr 2.14.1 writes by default (Blosc lz4 + byte shuffle, decoded by
    `tm_blosc_decompress` in the C-ABI library), zlib, or no compressor;
  * writers emit spec-conformant archives that `zarr.load` / `sparse.load_npz` open
    (state tiles: one chunk, uncompressed or zlib from the host, or a Blosc lz4 frame encoded on the GPU by
    `tm_blosc_compress_tiles` and wrapped by `write_zarr_zip_blosc`: the encoding zarr itself writes).
Only safe loaders are used (`numpy.load(allow_pickle=False)`, `zipfile`, `json`).
"""
import ctypes as C
import io
import json
import os
import zipfile
import zlib
from itertools import product
from typing import Optional, Sequence, Tuple

import numpy as np

GENES_PER_SLICE = 500


# ---- names ------------------------------------------------------------------------------------
def parse_gene_tile_name(path) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """'{r0}_{r1}_{c0}_{c1}_{R0}_{R1}_{C0}_{C1}.npz' -> (roi, roio)  (utils/MBADataset_tst.py:147-150)."""
    stem = os.path.splitext(os.path.basename(str(path)))[0]
    v = [int(p) for p in stem.split("_")]
    if len(v) != 8:
        raise ValueError(f"gene tile name needs 8 integers, got {stem!r}")
    return tuple(v[:4]), tuple(v[4:])


def parse_state_tile_name(path) -> Tuple[int, int, int, int]:
    stem = os.path.splitext(os.path.basename(str(path)))[0]
    v = [int(p) for p in stem.split("_")]
    if len(v) != 4:
        raise ValueError(f"state tile name needs 4 integers, got {stem!r}")
    return tuple(v)


# ---- gene tiles: pydata/sparse COO .npz ----------------------------------------------------------
def read_gene_npz(path):
    """-> (data [nnz], coords int64 [ndim, nnz], shape tuple).  Layout of sparse.save_npz (0.15.5):
    arrays 'data', 'coords', 'shape', 'fill_value' in a (compressed) .npz."""
    with np.load(path, allow_pickle=False) as z:
        data, coords, shape = z["data"], z["coords"], tuple(int(s) for s in z["shape"])
        if "fill_value" in z.files and float(z["fill_value"][()]) != 0.0:
            raise ValueError("gene tile with a non-zero fill value")
    if coords.ndim != 2 or coords.shape[0] != len(shape) or coords.shape[1] != data.shape[0]:
        raise ValueError(f"malformed COO archive {path}: coords {coords.shape}, data {data.shape}, shape {shape}")
    return data, coords.astype(np.int64, copy=False), shape


def write_gene_npz(path, data, coords, shape, compressed: bool = True):
    coords = np.asarray(coords)
    save = np.savez_compressed if compressed else np.savez
    with open(path, "wb") as f:                       # file object: numpy must not append '.npz'
        save(f, data=np.asarray(data), coords=coords, shape=np.asarray(shape, dtype=np.int64),
             fill_value=np.asarray(np.zeros((), dtype=np.asarray(data).dtype)))


def gene_tile_shift(roi: Sequence[int], roio: Sequence[int], gblk: int = 16, pad: int = 32) -> Tuple[int, int]:
    """Cell shift `psz - (roi[2i] - roio[2i]) // gblk` of _pad_gn (utils/MBADataset_tst.py:84-86)."""
    psz = pad // gblk
    return psz - (roi[0] - roio[0]) // gblk, psz - (roi[2] - roio[2]) // gblk


# ---- state tiles: zarr v2 array in a zip ------------------------------------------------------------
def _blosc_decode(buf: bytes) -> bytes:
    from . import _lib
    L = _lib.lib()
    n = C.c_size_t(0)
    src = (C.c_char * len(buf)).from_buffer_copy(buf)
    _lib.check(L.tm_blosc_decompress(src, len(buf), None, 0, C.byref(n)), "tm_blosc_decompress(size)")
    out = (C.c_char * max(1, n.value))()
    _lib.check(L.tm_blosc_decompress(src, len(buf), out, n.value, C.byref(n)), "tm_blosc_decompress")
    return bytes(out[:n.value])


def _decode_chunk(buf: bytes, compressor: Optional[dict]) -> bytes:
    if compressor is None:
        return buf
    cid = compressor.get("id")
    if cid == "blosc":
        return _blosc_decode(buf)
    if cid in ("zlib", "gzip"):
        return zlib.decompress(buf, 15 + 32)
    raise NotImplementedError(f"zarr compressor {cid!r} (supported: blosc-lz4, zlib, gzip, none)")


def read_zarr_zip(path) -> np.ndarray:
    """What `zarr.load(path)` returns for a single-array zarr-v2 ZipStore."""
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
        if ".zarray" not in names:
            raise ValueError(f"{path}: no .zarray at the archive root (not a zarr-v2 array store)")
        meta = json.loads(z.read(".zarray"))
        if meta.get("zarr_format") != 2:
            raise ValueError(f"{path}: zarr_format {meta.get('zarr_format')!r}, expected 2")
        if meta.get("filters"):
            raise NotImplementedError("zarr filters")
        shape, chunks = tuple(meta["shape"]), tuple(meta["chunks"])
        dtype, order = np.dtype(meta["dtype"]), meta.get("order", "C")
        sep = meta.get("dimension_separator", ".")
        fill = meta.get("fill_value")
        out = np.empty(shape, dtype=dtype)
        out[...] = 0 if fill is None else (np.nan if fill == "NaN" else fill)
        grid = [range((s + c - 1) // c) for s, c in zip(shape, chunks)]
        for idx in product(*grid):
            key = sep.join(str(i) for i in idx) if idx else "0"
            if key not in names:
                continue                                  # absent chunk = fill value
            raw = _decode_chunk(z.read(key), meta.get("compressor"))
            blk = np.frombuffer(raw, dtype=dtype, count=int(np.prod(chunks))).reshape(chunks, order=order)
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
            out[sl] = blk[tuple(slice(0, s.stop - s.start) for s in sl)]       # edge chunks are stored full size
    return out


def write_zarr_zip(path, arr: np.ndarray, compressor: Optional[str] = None, level: int = 1, date_time=None):
    """A single-chunk zarr-v2 array in a ZIP_STORED ZipStore (the layout zarr.save_array produces, with the
    chunk either raw or zlib-compressed: this writer runs on the host alone; frames of the GPU Blosc encoder go through
    write_zarr_zip_blosc).  date_time: a fixed
    (y, m, d, H, M, S) for the members instead of the clock, for files that must be reproducible byte for byte."""
    arr = np.ascontiguousarray(arr)
    if compressor not in (None, "zlib"):
        raise NotImplementedError("writer supports compressor None or 'zlib'")
    meta = {"chunks": list(arr.shape), "compressor": None if compressor is None else {"id": "zlib", "level": level},
            "dtype": arr.dtype.str, "fill_value": 0.0 if arr.dtype.kind == "f" else 0, "filters": None, "order": "C",
            "shape": list(arr.shape), "zarr_format": 2}
    payload = arr.tobytes()
    if compressor == "zlib":
        payload = zlib.compress(payload, level)
    tmp = str(path) + ".tmp"
    def member(name):
        if date_time is None:
            return name
        zi = zipfile.ZipInfo(name, date_time=tuple(date_time))
        zi.compress_type, zi.external_attr = zipfile.ZIP_STORED, 0o600 << 16
        return zi

    with zipfile.ZipFile(tmp, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as z:
        z.writestr(member(".zarray"), json.dumps(meta, indent=4, sort_keys=True))
        z.writestr(member(".".join("0" for _ in arr.shape) if arr.ndim else "0"), payload)
    os.replace(tmp, path)                                  # a reader never sees a half-written tile


BLOSC_COMPRESSOR = {"blocksize": 0, "clevel": 5, "cname": "lz4", "id": "blosc", "shuffle": 1}     # numcodecs.Blosc(): zarr's default


def write_zarr_zip_blosc(path, shape: Sequence[int], dtype: str, frame, date_time=None):
    """A single-chunk zarr-v2 array in a ZIP_STORED ZipStore whose chunk is `frame`: one Blosc-1 lz4 frame of the array's
    C-order bytes, already encoded (tm_blosc_compress / tm_blosc_compress_tiles).  The metadata is what zarr.save_array
    writes; members and date_time as in write_zarr_zip."""
    shape, dt = [int(s) for s in shape], np.dtype(dtype)
    frame = bytes(frame)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    if len(frame) < 16 or int.from_bytes(frame[4:8], "little") != nbytes or int.from_bytes(frame[12:16], "little") != len(frame):
        raise ValueError(f"{path}: not a Blosc frame of the {nbytes} bytes of a {dt.str} array of shape {tuple(shape)}")
    meta = {"chunks": shape, "compressor": dict(BLOSC_COMPRESSOR), "dtype": dt.str, "fill_value": 0.0 if dt.kind == "f" else 0,
            "filters": None, "order": "C", "shape": shape, "zarr_format": 2}
    tmp = str(path) + ".tmp"
    def member(name):
        if date_time is None:
            return name
        zi = zipfile.ZipInfo(name, date_time=tuple(date_time))
        zi.compress_type, zi.external_attr = zipfile.ZIP_STORED, 0o600 << 16
        return zi

    with zipfile.ZipFile(tmp, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as z:
        z.writestr(member(".zarray"), json.dumps(meta, indent=4, sort_keys=True))
        z.writestr(member(".".join("0" for _ in shape) if shape else "0"), frame)
    os.replace(tmp, path)                                  # a reader never sees a half-written tile


def read_state_tile(path) -> np.ndarray:
    """float16 [(stain z), 256, 256] as written by test_brn.py:222-226."""
    a = read_zarr_zip(path)
    if a.ndim != 3:
        raise ValueError(f"{path}: state tile must be 3-D, got {a.shape}")
    return a


# ---- state tiles decoded on the GPU (tm_blosc_decompress_tiles) ------------------------------------------------------
def read_zarr_zip_frames(path):
    """-> (the .zarray metadata, {chunk key: the member's raw bytes}): the container opened as read_zarr_zip opens it, nothing
    decoded.  Chunks that are absent from the archive (fill value) are absent from the dict."""
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
        if ".zarray" not in names:
            raise ValueError(f"{path}: no .zarray at the archive root (not a zarr-v2 array store)")
        meta = json.loads(z.read(".zarray"))
        if meta.get("zarr_format") != 2:
            raise ValueError(f"{path}: zarr_format {meta.get('zarr_format')!r}, expected 2")
        if meta.get("filters"):
            raise NotImplementedError("zarr filters")
        shape, chunks = tuple(meta["shape"]), tuple(meta["chunks"])
        sep = meta.get("dimension_separator", ".")
        members = {}
        for idx in product(*[range((s + c - 1) // c) for s, c in zip(shape, chunks)]):
            key = sep.join(str(i) for i in idx) if idx else "0"
            if key in names:
                members[key] = z.read(key)
    return meta, members


def blosc_frame_info(buf: bytes, what="frame"):
    """tm_blosc_frame_info of one frame -> _lib.TmBloscFrame (.gpu: the GPU decoder takes it); ValueError for a frame whose
    ranges leave it."""
    from . import _lib
    L = _lib.lib()
    info = _lib.TmBloscFrame()
    if L.tm_blosc_frame_info(buf, len(buf), C.byref(info)) != 0:
        raise ValueError(f"{what}: {L.tm_last_error().decode(errors='replace')}")
    return info


def gpu_chunk_jobs(path, meta, members, origin: int, chan_stride: int, pitch: int):
    """The chunks of one float16 [C, H, W] array as jobs of decode_chunks_dev: [(frame, origin element, chunk shape, clipped
    shape)] with element (c, y, x) of the array at origin + c * chan_stride + y * pitch + x -- or None where the GPU decoder
    does not take the array (not Blosc, not float16 in C order, a chunk absent, a "host only" frame): the host route's."""
    comp = meta.get("compressor")
    shape, chunks = tuple(meta["shape"]), tuple(meta["chunks"])
    if not comp or comp.get("id") != "blosc" or np.dtype(meta["dtype"]) != np.dtype("<f2") or meta.get("order", "C") != "C" or len(shape) != 3:
        return None
    sep = meta.get("dimension_separator", ".")
    jobs = []
    for idx in product(*[range((s + c - 1) // c) for s, c in zip(shape, chunks)]):
        frame = members.get(sep.join(str(i) for i in idx))
        if frame is None:
            return None
        info = blosc_frame_info(frame, f"{path}, chunk {idx}")
        if not info.gpu:
            return None
        if info.typesize != 2 or info.nbytes != 2 * int(np.prod(chunks)):
            raise ValueError(f"{path}, chunk {idx}: a frame of {info.nbytes} bytes at typesize {info.typesize}, not a float16 chunk {chunks}")
        clip = tuple(min(c, s - i * c) for i, c, s in zip(idx, chunks, shape))
        at = origin + idx[0] * chunks[0] * chan_stride + idx[1] * chunks[1] * pitch + idx[2] * chunks[2]
        jobs.append((frame, at, chunks, clip))
    return jobs


decode_timings = None            # a list: decode_chunks_dev appends (ms of the decoder call by hipEvents, frames, frame bytes); tools/bench_load_step.py


def decode_chunks_dev(canvas, jobs):
    """One host buffer of the jobs' frames, one copy to canvas.device, one tm_blosc_decompress_tiles into `canvas` (a contiguous
    float16 / float32 [C, H, W] device tensor) -> the per-frame status as a list (0: decoded; see teramind_hip.h)."""
    import torch
    from . import _lib
    L = _lib.lib()
    assert canvas.is_cuda and canvas.is_contiguous() and canvas.dim() == 3
    n = len(jobs)
    offs = np.zeros(n + 1, np.int64)
    for k, job in enumerate(jobs):
        offs[k + 1] = offs[k] + ((len(job[0]) + 15) & ~15)              # frames start at multiples of 16
    host = np.zeros(int(offs[n]), np.uint8)
    boxes = (_lib.TmBloscBox * n)()
    for k, (frame, at, chunks, clip) in enumerate(jobs):
        host[offs[k]:offs[k] + len(frame)] = np.frombuffer(frame, np.uint8)
        boxes[k].origin = at
        boxes[k].chunk[:], boxes[k].clip[:] = chunks, clip
    with torch.cuda.device(canvas.device):
        dev = torch.from_numpy(host).to(canvas.device)
        status = torch.empty(n, dtype=torch.int32, device=canvas.device)
        dtype = {torch.float32: 0, torch.float16: 2}[canvas.dtype]                       # TM_DTYPE_F32 / TM_DTYPE_F16
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if decode_timings is not None else None
        if ev:
            ev[0].record()
        _lib.check(L.tm_blosc_decompress_tiles(_lib.ptr(dev), host.ctypes.data, offs.ctypes.data, n, _lib.ptr(canvas), dtype, canvas.numel(),
                                               canvas.stride(0), canvas.stride(1), C.cast(boxes, C.c_void_p), _lib.ptr(status),
                                               _lib.current_stream_ptr()), "tm_blosc_decompress_tiles")
        if ev:
            ev[1].record()
        out = status.cpu().tolist()                                     # waits for the stream: `dev` and `host` may go
        if ev:
            decode_timings.append((ev[0].elapsed_time(ev[1]), n, int(offs[n])))
        return out


def read_zarr_zip_dev(path, device):
    """read_zarr_zip as a tensor on `device`: a float16 [C, H, W] array of Blosc-lz4 chunks is decoded there (-> (tensor, True)),
    anything else is read on the host and copied (-> (tensor, False))."""
    import torch
    meta, members = read_zarr_zip_frames(path)
    shape = tuple(meta["shape"])
    jobs = gpu_chunk_jobs(path, meta, members, 0, shape[1] * shape[2], shape[2]) if len(shape) == 3 else None
    if jobs is None:
        return torch.from_numpy(read_zarr_zip(path)).to(device), False
    out = torch.empty(shape, dtype=torch.float16, device=device)
    status = decode_chunks_dev(out, jobs)
    if any(status):
        raise ValueError(f"{path}: corrupt Blosc-lz4 stream (decoder status {max(status)})")
    return out, True


def read_state_tile_dev(path, device):
    """read_state_tile as a float16 tensor on `device`, decoded there where the file holds Blosc-lz4 chunks."""
    a = read_zarr_zip_dev(path, device)[0]
    if a.dim() != 3:
        raise ValueError(f"{path}: state tile must be 3-D, got {tuple(a.shape)}")
    return a


def write_state_tile(path, tile, compressor: Optional[str] = None):
    write_zarr_zip(path, np.asarray(tile, dtype=np.float16), compressor)
