"""Stitcher: per-step state tiles -> whole-ROI slice images.

Restates the gather of the reference's infer_brn.py:57-105 (`gen_col`: load every tile of a tile column,
reorder channels '(c s) h w -> (s c) h w', map [-1, 1] -> uint8 with `((g + 1) * 127.5).astype(uint8)` in
float16, stack the tiles of the column; `gen_mba`: join the columns) without pyvips: the mosaic is one
tensor.  `save_slices` writes it with PIL as plain TIFF / JPEG (small ROIs); `save_slices_pyramid` writes the
reference's product, one tiled pyramidal OME-TIFF (BigTIFF, 256 x 256 JPEG tiles) per slice, with the level
reductions and the JPEG tile scans computed on the GPU (ometiff.py).  Pinned there: the JPEG bytes equal
libjpeg's and Pillow / libtiff reads the container back; not pinned: byte equality with a libvips-written file,
libvips' level sizes at odd dimensions, QuPath / Bio-Formats (never run).  `save_composites_pyramid` writes the two stains
of a slice as one colour pyramid (PolyT green, DAPI blue, utils/vis_mba.py:193-195), optionally brightened and with an
ontology overlay as onto_overlay does; the composite is formed inside the colour JPEG kernel.  `save_attn_heatmaps_pyramid`
writes a slice of the attention read-out mosaic as a colour-mapped pyramid of its smoothed field (heatmap.py), on its own or
blended over that composite.  Output index `sl = s * n_stain + c` (slice-major, stain-minor), as the reference's
per-slice directories are numbered.
"""
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import formats, heatmap, ometiff, tiles


def to_uint8(g: torch.Tensor) -> torch.Tensor:
    """infer_brn.py:83: `((g + 1) * 127.5).astype(np.uint8)` on the float16 tile (arithmetic in float16)."""
    return ((g.half() + 1) * 127.5).to(torch.uint8)


def reorder_slices(tile: torch.Tensor, slc: int) -> torch.Tensor:
    """'(c s) h w -> (s c) h w' with s = slc (infer_brn.py:81)."""
    cs, h, w = tile.shape[-3:]
    c = cs // slc
    return tile.reshape(*tile.shape[:-3], c, slc, h, w).transpose(-4, -3).reshape(*tile.shape[:-3], cs, h, w)


def stitch_state(state: torch.Tensor, slc: int = 50, slices: Optional[Sequence[int]] = None) -> torch.Tensor:
    """[(c s), H, W] resident state (TileSweep.local_state(), already tile-contiguous) -> uint8 [(s c), H, W]."""
    out = reorder_slices(to_uint8(state), slc)
    return out if slices is None else out[list(slices)]


def _decoder_device(decoder: str, device):
    if decoder not in ("host", "gpu"):
        raise ValueError(f"decoder must be 'host' or 'gpu', got {decoder!r}")
    return None if decoder == "host" else torch.device("cuda" if device is None else device)


def stitch_dir(step_dir, hst: int, wst: int, hnm: int, wnm: int, slc: int = 50,
               slices: Optional[Sequence[int]] = None, size: int = tiles.TILE, decoder: str = "host", device=None):
    """Mosaic of a reference-format step directory ('{r0}_{r1}_{c0}_{c1}.zip' tiles; infer_brn.py:70-76 with
    is_gen=True) -> uint8 [n_slices, hnm*size, wnm*size].  decoder="gpu": the tiles are decoded on `device`
    (formats.read_state_tile_dev), `to_uint8` / `reorder_slices` run there and the mosaic is a uint8 tensor on it, equal to
    the host route's array."""
    dev = _decoder_device(decoder, device)
    out = None
    for pw in range(wnm):
        for ph in range(hnm):
            r0, c0 = hst + ph * size, wst + pw * size
            path = os.path.join(str(step_dir), f"{r0}_{r0 + size}_{c0}_{c0 + size}.zip")
            if dev is not None:
                t = stitch_state(formats.read_state_tile_dev(path, dev), slc, slices)
                if out is None:
                    out = torch.zeros((t.shape[0], hnm * size, wnm * size), dtype=torch.uint8, device=dev)
                out[:, ph * size:(ph + 1) * size, pw * size:(pw + 1) * size] = t
                continue
            a = formats.read_state_tile(path)
            t = stitch_state(torch.from_numpy(a), slc, slices).numpy()
            if out is None:
                out = np.zeros((t.shape[0], hnm * size, wnm * size), dtype=np.uint8)
            out[:, ph * size:(ph + 1) * size, pw * size:(pw + 1) * size] = t
    return out


def stitch_real_dir(rdir, hst: int, wst: int, hnm: int, wnm: int, slc: int = 50,
                    slices: Optional[Sequence[int]] = None, size: int = tiles.TILE, decoder: str = "host", device=None):
    """Mosaic of a directory of real tiles (infer_brn.py:67-77 with is_gen=False, test_brn.py:93-99): eight-number names
    '{r0}_{r1}_{c0}_{c1}_{r0-p}_{r1+p}_{c0-p}_{c1+p}.zip' with the frame p = size // 2, arrays [(c s), size + 2p, size + 2p]
    in image units.  The centre is cut, '(c s) -> (s c)', `.astype(uint8)` -> uint8 [n_slices, hnm*size, wnm*size].
    decoder="gpu": as in stitch_dir (float16 Blosc-lz4 tiles are decoded on `device`, others read on the host and copied)."""
    dev = _decoder_device(decoder, device)
    out, p = None, size // 2
    for pw in range(wnm):
        for ph in range(hnm):
            r0, c0 = hst + ph * size, wst + pw * size
            name = f"{r0}_{r0 + size}_{c0}_{c0 + size}_{r0 - p}_{r0 + size + p}_{c0 - p}_{c0 + size + p}.zip"
            if dev is not None:
                a = formats.read_zarr_zip_dev(os.path.join(str(rdir), name), dev)[0]
                if a.dim() != 3 or a.shape[1] < size + p or a.shape[2] < size + p:
                    raise ValueError(f"{name}: a real tile is [(c s), {size + 2 * p}, {size + 2 * p}], got {tuple(a.shape)}")
                if a.shape[0] % slc:
                    raise ValueError(f"{name}: {a.shape[0]} planes are no multiple of slc = {slc}")
                t = reorder_slices(a[:, p:p + size, p:p + size], slc).to(torch.uint8)
                if slices is not None:
                    t = t[list(slices)]
                if out is None:
                    out = torch.zeros((t.shape[0], hnm * size, wnm * size), dtype=torch.uint8, device=dev)
                out[:, ph * size:(ph + 1) * size, pw * size:(pw + 1) * size] = t
                continue
            a = formats.read_zarr_zip(os.path.join(str(rdir), name))
            if a.ndim != 3 or a.shape[1] < size + p or a.shape[2] < size + p:
                raise ValueError(f"{name}: a real tile is [(c s), {size + 2 * p}, {size + 2 * p}], got {a.shape}")
            if a.shape[0] % slc:
                raise ValueError(f"{name}: {a.shape[0]} planes are no multiple of slc = {slc}")
            t = reorder_slices(torch.from_numpy(np.ascontiguousarray(a[:, p:p + size, p:p + size])), slc).numpy().astype(np.uint8)
            if slices is not None:
                t = t[list(slices)]
            if out is None:
                out = np.zeros((t.shape[0], hnm * size, wnm * size), dtype=np.uint8)
            out[:, ph * size:(ph + 1) * size, pw * size:(pw + 1) * size] = t
    return out


def save_slices(mosaic, odir, names: Optional[Sequence[int]] = None, jpeg: bool = True):
    """'{odir}/all_{sl}.tif' (+ '.jpg'), the file names of infer_brn.py:96-101 (flat, non-pyramidal)."""
    from PIL import Image
    os.makedirs(str(odir), exist_ok=True)
    arr = mosaic.cpu().numpy() if isinstance(mosaic, torch.Tensor) else np.asarray(mosaic)
    for k in range(arr.shape[0]):
        sl = k if names is None else names[k]
        im = Image.fromarray(arr[k], mode="L")
        im.save(os.path.join(str(odir), f"all_{sl}.tif"))
        if jpeg:
            im.save(os.path.join(str(odir), f"all_{sl}.jpg"))


def save_slices_pyramid(state, odir, slc: int = 50, slices: Optional[Sequence[int]] = None,
                        names: Optional[Sequence[int]] = None, quality: int = 75, page: Optional[int] = None,
                        compression: str = "jpeg", device=None):
    """'{odir}/all_{sl}.tif' as tiled pyramidal OME-TIFF (infer_brn.py:50-54,100), one plane at a time so that the uint8
    copy of a whole canvas never exists.  state: the resident float [(c s), H, W] state (plane k of the '(s c)' order is
    converted with `to_uint8` on its device), or a host / device uint8 mosaic [(s c), H, W] as `stitch_dir` returns
    (uploaded plane by plane).  slices: indices into the '(s c)' order (default all); names as in `save_slices`.
    page: also write that pyramid level as 'all_{sl}.jpg', as gen_mba does (infer_brn.py:101-103)."""
    os.makedirs(str(odir), exist_ok=True)
    if isinstance(state, np.ndarray):
        state = torch.from_numpy(state)
    is_u8 = state.dtype == torch.uint8
    dev = torch.device(device) if device is not None else (state.device if state.is_cuda else torch.device("cuda"))
    cs = state.shape[0]
    if not is_u8 and cs % slc:
        raise ValueError(f"{cs} state planes are no multiple of slc = {slc}")
    picks = list(range(cs)) if slices is None else list(slices)
    bufs = ometiff.JpegBatches(dev, ometiff.BATCH_TILES, ometiff.SLOT_BYTES) if compression == "jpeg" else None
    for k, idx in enumerate(picks):
        sl = idx if names is None else names[k]
        if is_u8:
            plane = state[idx].to(dev).contiguous()
        else:
            s_, c_ = divmod(idx, cs // slc)                        # '(s c)' index -> plane c * slc + s of '(c s)'
            plane = to_uint8(state[c_ * slc + s_].to(dev)).contiguous()
        levels = ometiff.write_pyramid(os.path.join(str(odir), f"all_{sl}.tif"), plane, quality, compression, buffers=bufs)
        if page is not None:
            from PIL import Image
            Image.fromarray(levels[page].cpu().numpy(), mode="L").save(os.path.join(str(odir), f"all_{sl}.jpg"))


REGIONS = ("all", "half", "rhalf", "thalf", "bhalf", "quarter", "3quarter")


def overlay_region(overlay: np.ndarray, region: str = "all") -> np.ndarray:
    """The part of an [h, w, 3] overlay that `region` keeps, the rest black (= not blended), as onto_overlay selects it
    (utils/vis_mba.py:142-161): half / rhalf = left / right, thalf / bhalf = top / bottom, quarter = top left, 3quarter = all
    but top right."""
    if region not in REGIONS:
        raise ValueError(f"region must be one of {', '.join(REGIONS)}, got {region!r}")
    ov = np.ascontiguousarray(overlay)
    if ov.dtype != np.uint8 or ov.ndim != 3 or ov.shape[2] != 3:
        raise ValueError(f"the overlay is a uint8 [h, w, 3] image, got {ov.dtype} {ov.shape}")
    h, w = ov.shape[:2]
    keep = np.zeros((h, w), dtype=bool)
    if region == "all":
        keep[:] = True
    elif region == "half":
        keep[:, :w // 2] = True
    elif region == "rhalf":
        keep[:, w // 2:] = True
    elif region == "thalf":
        keep[:h // 2] = True
    elif region == "bhalf":
        keep[h // 2:] = True
    elif region == "quarter":
        keep[:h // 2, :w // 2] = True
    else:
        keep[:] = True
        keep[:h // 2, w // 2:] = False
    return ov * keep[:, :, None].astype(np.uint8)


def save_composites_pyramid(state, odir, slc: int = 50, slices: Optional[Sequence[int]] = None, quality: int = 75,
                            page: Optional[int] = None, bright: float = 1.0, overlay=None, alpha: int = 100,
                            region: str = "all", device=None):
    """'{odir}/rgb_{s}.tif' per slice s: the two stains of the slice as one colour image, R = 0, G = PolyT (c = 1),
    B = DAPI (c = 0) (utils/vis_mba.py:193-195), as a tiled pyramidal OME-TIFF of YCbCr JPEG pages (ometiff.write_pyramid_rgb).
    state: the resident float [(c s), H, W] state or a uint8 [(s c), H, W] mosaic of all `slc` slices; only the two planes of
    one slice are converted / uploaded at a time.  slices: slice indices (default all).  bright, overlay ([h, w, 3] uint8 array
    or an image path), alpha, region: onto_overlay's brightening and ontology overlay (overlay_region keeps `region` of it);
    they are applied per level on the GPU.  page: also write that level's composite as 'rgb_{s}.jpg' through Pillow."""
    os.makedirs(str(odir), exist_ok=True)
    if isinstance(state, np.ndarray):
        state = torch.from_numpy(state)
    is_u8 = state.dtype == torch.uint8
    dev = torch.device(device) if device is not None else (state.device if state.is_cuda else torch.device("cuda"))
    cs = state.shape[0]
    if cs % slc:
        raise ValueError(f"{cs} state planes are no multiple of slc = {slc}")
    n_stain = cs // slc
    if n_stain < 2:
        raise ValueError(f"a composite shows two stains (PolyT green, DAPI blue); this state has {n_stain} per slice "
                         f"({cs} planes, slc = {slc}): use save_slices_pyramid for grey pages")
    if region not in REGIONS:
        raise ValueError(f"region must be one of {', '.join(REGIONS)}, got {region!r}")
    ov = None
    if overlay is not None:
        if isinstance(overlay, torch.Tensor):
            overlay = overlay.cpu().numpy()
        elif not isinstance(overlay, np.ndarray):
            from PIL import Image
            with Image.open(str(overlay)) as im:
                overlay = np.asarray(im.convert("RGB"))
        ov = torch.from_numpy(overlay_region(overlay, region)).to(dev)
    picks = list(range(slc)) if slices is None else list(slices)
    if any(not 0 <= s < slc for s in picks):
        raise ValueError(f"slices are indices 0 .. {slc - 1}, got {picks}")
    bufs = ometiff.JpegBatches(dev, ometiff.BATCH_TILES, 3 * ometiff.SLOT_BYTES)
    for s in picks:
        pair = []
        for c in (1, 0):                                           # green = PolyT, blue = DAPI
            if is_u8:
                pair.append(state[s * n_stain + c].to(dev).contiguous())
            else:
                pair.append(to_uint8(state[c * slc + s].to(dev)).contiguous())
        levels = ometiff.write_pyramid_rgb(os.path.join(str(odir), f"rgb_{s}.tif"), (None, pair[0], pair[1]), quality, bright, ov,
                                           alpha, buffers=bufs)
        if page is not None:
            from PIL import Image
            Image.fromarray(levels[page].compose().cpu().numpy(), mode="RGB").save(os.path.join(str(odir), f"rgb_{s}.jpg"))


# ---- attention read-out tiles (infer_attn.py:9-39) -----------------------------------------------------------
def stitch_attn_dir(adir, hst: int, wst: int, hnm: int, wnm: int, size: int = tiles.TILE) -> np.ndarray:
    """Mosaic of a directory of attention read-out tiles ('{r0}_{r1}_{c0}_{c1}.zip', float16 [50, 4K, 16, 16] each) ->
    float16 [50, 4K, hnm*16, wnm*16]: `gen_col` concatenates the tiles of a tile column on axis -2, `gen_mba` joins the
    columns on axis -1."""
    cols = []
    for pw in range(wnm):
        col = []
        for ph in range(hnm):
            r0, c0 = hst + ph * size, wst + pw * size
            col.append(formats.read_zarr_zip(os.path.join(str(adir), f"{r0}_{r0 + size}_{c0}_{c0 + size}.zip")))
        cols.append(np.concatenate(col, -2))
    return np.concatenate(cols, -1)


def save_attn_slices(mosaic, odir, names: Optional[Sequence[int]] = None):
    """'{odir}/all_{sl}.zip' per slice (zarr v2), the files infer_attn.gen_mba leaves (infer_attn.py:36-38)."""
    os.makedirs(str(odir), exist_ok=True)
    arr = mosaic.cpu().numpy() if isinstance(mosaic, torch.Tensor) else np.asarray(mosaic)
    for k in range(arr.shape[0]):
        sl = k if names is None else names[k]
        formats.write_zarr_zip(os.path.join(str(odir), f"all_{sl}.zip"), arr[k])


def save_attn_heatmaps_pyramid(mosaic, odir, K: int, mode: str = "att_all", gene: Optional[int] = None,
                               slices: Optional[Sequence[int]] = None, lut=None, vmax: Optional[float] = None, sigma: float = 2.0,
                               scale: int = 4, quality: int = 90, under=None, slc: int = 50, alpha: int = 160, floor: int = 1,
                               page: Optional[int] = None, wei: float = 229, path: Optional[str] = None, device=None):
    """Heat maps of the attention read-out mosaic float16 [S, 4K, H, W] (stitch_attn_dir's array or a device tensor; a host
    mosaic is uploaded one slice at a time) as tiled pyramidal OME-TIFFs of colour JPEG pages, what test_attn.gen_img draws with
    matplotlib (test_attn.py:145-250).  Per chosen slice sl (indices into S, default all): heatmap.field (mode, gene, wei,
    sigma) -> heatmap.render (lut, 0 .. vmax, scale, floor) -> the colour pyramid writer.
      under=None    '{odir}/heat_{mode}_{sl}.tif': the three rendered planes through ometiff.write_pyramid_rgb
      under=state   '{odir}/heat_over_{mode}_{sl}.tif': the PolyT-green / DAPI-blue composite of slice sl of the resident
                    [(c s), H, W] two-stain state (or uint8 '(s c)' mosaic; `slc` slices, as save_composites_pyramid takes)
                    with the interleaved heat map as the encoder's overlay at `alpha`; the encoder samples the overlay by
                    each level's own size, so the map is rendered once, at `scale`
    lut, vmax: the table and the value painted with its last entry.  With path = 'GLUT' | 'DOPA' | 'BLOD' they default to the
    reference's (test_attn.py:173-180): INFERNO and PATHWAY_VMAX[path]['att_all'] for att_all, the gene's two-colour palette
    and PATHWAY_VMAX[path]['expr'][gene] for expr; lut alone defaults to INFERNO; without them vmax is required.
    floor: table entries below it stay black (= transparent in the blend).  page: also write that level as '.jpg' through Pillow."""
    os.makedirs(str(odir), exist_ok=True)
    if path is not None and path not in heatmap.PATHWAY_VMAX:
        raise ValueError(f"path must be one of {', '.join(heatmap.PATHWAY_VMAX)}, got {path!r}")
    heatmap.mode_ranges(K, mode, gene)                             # refuses an unknown mode / a missing gene before any work
    if path is not None and mode == "expr":
        if lut is None:
            lut = heatmap.two_colour(heatmap.PATHWAY_COLOURS[path][gene])
        if vmax is None:
            vmax = heatmap.PATHWAY_VMAX[path]["expr"][gene]
    elif path is not None and mode == "att_all" and vmax is None:
        vmax = heatmap.PATHWAY_VMAX[path]["att_all"]
    if lut is None:
        lut = heatmap.INFERNO
    if vmax is None:
        raise ValueError(f"vmax is required for mode {mode!r} without a pathway that states it")
    if isinstance(mosaic, np.ndarray):
        mosaic = torch.from_numpy(mosaic)
    if mosaic.dim() != 4 or mosaic.dtype != torch.float16 or mosaic.shape[1] != 4 * K:
        raise ValueError(f"the mosaic is float16 [S, 4K = {4 * K}, H, W], got {mosaic.dtype} {tuple(mosaic.shape)}")
    dev = torch.device(device) if device is not None else (mosaic.device if mosaic.is_cuda else torch.device("cuda"))
    picks = list(range(mosaic.shape[0])) if slices is None else list(slices)
    if any(not 0 <= s < mosaic.shape[0] for s in picks):
        raise ValueError(f"slices are indices 0 .. {mosaic.shape[0] - 1}, got {picks}")
    n_stain, is_u8 = 0, False
    if under is not None:
        if isinstance(under, np.ndarray):
            under = torch.from_numpy(under)
        is_u8 = under.dtype == torch.uint8
        if under.shape[0] % slc or under.shape[0] // slc < 2:
            raise ValueError(f"the state under a heat map has two stains per slice; got {under.shape[0]} planes, slc = {slc}")
        n_stain = under.shape[0] // slc
        if any(s >= slc for s in picks):
            raise ValueError(f"slices are indices 0 .. {slc - 1} of the state, got {picks}")
    bufs = ometiff.JpegBatches(dev, ometiff.BATCH_TILES, 3 * ometiff.SLOT_BYTES)
    for sl in picks:
        fld = heatmap.field(mosaic[sl].to(dev), K, mode, wei, sigma, gene)
        if under is None:
            name = f"heat_{mode}_{sl}"
            planes = heatmap.render(fld, lut, 0.0, vmax, scale, floor)
            levels = ometiff.write_pyramid_rgb(os.path.join(str(odir), name + ".tif"), planes, quality, buffers=bufs)
        else:
            name = f"heat_over_{mode}_{sl}"
            ov = heatmap.render(fld, lut, 0.0, vmax, scale, floor, interleaved=True)
            pair = []
            for c in (1, 0):                                       # green = PolyT, blue = DAPI
                if is_u8:
                    pair.append(under[sl * n_stain + c].to(dev).contiguous())
                else:
                    pair.append(to_uint8(under[c * slc + sl].to(dev)).contiguous())
            levels = ometiff.write_pyramid_rgb(os.path.join(str(odir), name + ".tif"), (None, pair[0], pair[1]), quality, 1.0, ov,
                                               alpha, buffers=bufs)
        if page is not None:
            from PIL import Image
            Image.fromarray(levels[page].compose().cpu().numpy(), mode="RGB").save(os.path.join(str(odir), name + ".jpg"))
