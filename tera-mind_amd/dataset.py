"""Training batches from tile files (reference utils/MBADataset.py:17-170, `sparse_batch_collate` :213-236).

The reference's training dataset opens one gene `.npz` and one image `.zip` per item, crops, block-sums and transposes a COO
on the CPU, and the step densifies the collated COO on the GPU (experiment.py:129).  Here every tile is uploaded once
(`TrainTileSet`: images as they are stored, the COO entries ordered by pixel row with a row-start table) and a batch is two
kernels, `tm_train_batch_images` and `tm_train_batch_genes` (csrc/tm_io.hip): crop, z window, rot90 / hflip, scaling, block
sum, padding and densification on the device, with no COO round trip.

What is drawn per sample -- the tile, the crop corner, the first slice `snm`, `rot`, `flip` -- has the reference's ranges
(MBADataset.py:71-72,136,156,163) but not its random stream: the reference draws from the process-global `random` /
`torch.rand` state of each DataLoader worker, which cannot be reproduced.  `TileSampler` is counter based instead: a draw is
a pure function of (seed, epoch, step, micro, rank), so a resumed run needs no generator state.
"""
import itertools
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .config import GENES_PER_SLICE, Z_PAD, PathConfig

STAIN_CODE = {"all": 0, "DAPI": 1, "PolyT": 2}
# streams of the keyed generator: one Philox key per purpose, so that no two purposes share numbers
STREAM_PERM, STREAM_SAMPLE, STREAM_STEP = 0, 1, 2


def keyed_rng(seed: int, stream: int, epoch: int = 0, step: int = 0, micro: int = 0, rank: int = 0) -> np.random.Generator:
    """numpy Philox-4x64 with key (seed, stream) and counter (epoch, step, micro, rank): a pure function of its arguments."""
    m = (1 << 64) - 1
    bg = np.random.Philox(key=np.array([int(seed) & m, int(stream) & m], dtype=np.uint64),
                          counter=np.array([int(epoch) & m, int(step) & m, int(micro) & m, int(rank) & m], dtype=np.uint64))
    return np.random.Generator(bg)


def image_path(gene_path: str) -> str:
    """The image archive of a gene tile (MBADataset.py:101)."""
    return str(gene_path).replace("gene", "img").replace(".npz", ".zip")


def mouse_file_list(mouse: str, lists: Dict[str, Sequence[str]], repeat: int = 10) -> List[str]:
    """The gene-tile list of MBADataset.__init__ (:50-60) from the `pth` columns of the reference's two csv files, given as
    {'609882': [...], '609889': [...]} (no csv is shipped): each of the two single mice trains on the OTHER mouse's list, as
    the reference has it, 638850 on both; the list is then repeated `repeat` times.  Not shuffled here: the per-epoch
    permutation of TileSampler does that."""
    if mouse == "609882":
        pth = list(lists["609889"])
    elif mouse == "609889":
        pth = list(lists["609882"])
    elif mouse == "638850":
        pth = list(lists["609882"]) + list(lists["609889"])
    else:
        raise ValueError(f"unknown mouse {mouse!r}")
    if repeat > 1:
        pth = list(itertools.chain(*itertools.repeat(pth, repeat)))
    return pth


@dataclass(frozen=True)
class TrainGeometry:
    """MBADataset's constructor arguments as config.make_dataset derives them (config.py:237-251)."""
    sdim: int          # crop edge in pixels
    gblk: int          # pixels per gene cell
    pdim: int          # gene cells of zero padding each side
    snum: int          # gene slices per sample (rna_slc)
    stain: str = "all"

    def __post_init__(self):
        if self.snum not in Z_PAD:
            raise ValueError(f"snum {self.snum} not in {sorted(Z_PAD)}")
        if self.stain not in STAIN_CODE:
            raise ValueError(f"stain {self.stain!r}")
        if self.sdim % self.gblk:
            raise ValueError(f"sdim {self.sdim} is not a multiple of gblk {self.gblk}")

    @classmethod
    def from_config(cls, cfg: PathConfig, sdim: Optional[int] = None) -> "TrainGeometry":
        coef = 2 if cfg.patch_size == 128 else 4
        return cls(sdim=sdim or coef * cfg.patch_size, gblk=cfg.patch_size // cfg.gn_sz, pdim=cfg.gn_sz // 2, snum=cfg.rna_slc,
                   stain=cfg.stain)

    @property
    def spad(self) -> int:
        return Z_PAD[self.snum]

    @property
    def shf(self) -> int:
        return self.snum // 4 if self.snum > 1 else 0

    @property
    def img_channels(self) -> int:
        return (2 if self.stain == "all" else 1) * (self.snum - 2 * self.shf)

    @property
    def gs(self) -> int:
        return self.sdim // self.gblk


class TileSampler:
    """Host half of a draw: which tile, crop, slice window and transform each sample of a batch gets.

    `entries` = for every position of the (repeated) file list the index of its resident tile.  One seeded permutation of
    the list per epoch; rank r of `world` takes positions r, r + world, ... of it (disjoint shares of equal length, the
    remainder dropped), and the share is cut into batches with `drop_last`.  The global micro-batch index step *
    accum_batches + micro selects epoch and batch."""

    def __init__(self, entries: Sequence[int], H: int, W: int, geo: TrainGeometry, seed: int = 0, gmax: int = 50,
                 accum_batches: int = 1):
        self.entries = np.asarray(entries, dtype=np.int64)
        if self.entries.ndim != 1 or self.entries.size == 0:
            raise ValueError("TileSampler: empty tile list")
        if geo.sdim > H or geo.sdim > W:
            raise ValueError(f"crop {geo.sdim} larger than the {H} x {W} tiles")
        self.H, self.W, self.geo, self.seed, self.gmax, self.accum = int(H), int(W), geo, int(seed), int(gmax), int(accum_batches)
        self.snm_max = self.gmax + 2 * geo.spad - geo.snum
        if self.snm_max < 0:
            raise ValueError(f"{gmax} slices are fewer than snum {geo.snum}")

    def batches_per_epoch(self, batch: int, world: int = 1) -> int:
        n = (len(self.entries) // world) // batch
        if n < 1:
            raise ValueError(f"{len(self.entries)} list entries over {world} ranks do not fill one batch of {batch}")
        return n

    def position(self, batch: int, step: int, micro: int = 0, world: int = 1) -> Tuple[int, int]:
        """(epoch, batch index inside the epoch) of micro-batch `micro` of optimizer step `step`."""
        return divmod(int(step) * self.accum + int(micro), self.batches_per_epoch(batch, world))

    def epoch_share(self, epoch: int, rank: int = 0, world: int = 1) -> np.ndarray:
        """List positions rank `rank` visits in `epoch`, in order."""
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside [0, {world})")
        perm = keyed_rng(self.seed, STREAM_PERM, epoch).permutation(len(self.entries))
        return perm[rank::world][:len(self.entries) // world]

    def params(self, batch: int, step: int, micro: int = 0, rank: int = 0, world: int = 1) -> np.ndarray:
        """int32 [batch, 6]: (tile, top, left, snm, rot, flip) per sample."""
        epoch, k = self.position(batch, step, micro, world)
        pos = self.epoch_share(epoch, rank, world)[k * batch:(k + 1) * batch]
        rng = keyed_rng(self.seed, STREAM_SAMPLE, epoch, step, micro, rank)
        g = self.geo
        out = np.empty((batch, 6), dtype=np.int32)
        out[:, 0] = self.entries[pos]
        out[:, 1] = rng.integers(0, self.H - g.sdim + 1, batch)           # random.randint(0, H - sdim), both ends included
        out[:, 2] = rng.integers(0, self.W - g.sdim + 1, batch)
        out[:, 3] = rng.integers(0, self.snm_max + 1, batch)
        out[:, 4] = rng.integers(0, 4, batch)
        out[:, 5] = rng.random(batch) < 0.5
        return out


def sort_by_row(data, coords, H: int):
    """Order one tile's COO entries by pixel row (stable) and build its row-start table.
    -> (crd int32 [3, n], dat fp32 [n], row_start int32 [H + 1]); entries outside rows [0, H) are dropped."""
    coords = np.asarray(coords)
    data = np.asarray(data)
    ok = (coords[0] >= 0) & (coords[0] < H)
    if not ok.all():
        coords, data = coords[:, ok], data[ok]
    order = np.argsort(coords[0], kind="stable")
    crd = np.ascontiguousarray(coords[:, order].astype(np.int32))
    dat = np.ascontiguousarray(data[order].astype(float).astype(np.float32))
    row_start = np.searchsorted(crd[0], np.arange(H + 1), side="left").astype(np.int32)
    return crd, dat, row_start


class TrainBatch:
    """img fp32 [B, C, sdim, sdim] in [-1, 1]; rna fp32 dense [B, gs + 2 pdim, gs + 2 pdim, snum * 500]; params the int32
    [B, 6] host array the batch was cut with."""

    def __init__(self, img, rna, params: np.ndarray):
        self.img, self.rna, self.params = img, rna, params

    def as_coo(self):
        """(im, dat, crd, ssz, lab) as `sparse_batch_collate` returns it (MBADataset.py:213-236): crd int64 [4, nnz] =
        (sample, h, w, channel) in row-major order of the dense tensor."""
        import torch
        crd = self.rna.nonzero().t().contiguous()
        dat = self.rna[tuple(crd)]
        return self.img, dat, crd, torch.Size(self.rna.shape), torch.zeros(self.img.shape[0], dtype=torch.long)


class TrainTileSet:
    """Resident training tiles + the batch draw.  `paths_or_dir`: a directory of gene `.npz` tiles or a list of their paths
    (a path may repeat: it is loaded once); each tile's image is `image_path(gene_path)`."""

    def __init__(self, paths_or_dir, cfg: PathConfig, device="cuda:0", seed: int = 0, repeat: int = 1, accum_batches: int = 1,
                 sdim: Optional[int] = None):
        from . import formats
        if isinstance(paths_or_dir, (str, os.PathLike)):
            d = str(paths_or_dir)
            paths = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".npz"))
        else:
            paths = [str(p) for p in paths_or_dir]
        if not paths:
            raise ValueError(f"no gene tiles in {paths_or_dir!r}")
        uniq = list(dict.fromkeys(paths))
        images = [formats.read_zarr_zip(image_path(p)) for p in uniq]
        genes = [formats.read_gene_npz(p) for p in uniq]
        index = {p: i for i, p in enumerate(uniq)}
        self._init(images, genes, TrainGeometry.from_config(cfg, sdim), device, seed, [index[p] for p in paths], repeat, accum_batches)
        self.paths = uniq

    @classmethod
    def from_arrays(cls, images, genes, geo: TrainGeometry, device="cuda:0", seed: int = 0, entries=None, repeat: int = 1,
                    accum_batches: int = 1) -> "TrainTileSet":
        """images: per tile an array [(s z) = 2 Zt, H, W], uint8 or float16; genes: per tile (data [nnz], coords [3, nnz],
        shape (H, W, Zt * 500)); entries: the file list as tile indices (default: each tile once)."""
        self = cls.__new__(cls)
        self._init(list(images), list(genes), geo, device, seed, entries, repeat, accum_batches)
        self.paths = None
        return self

    def _init(self, images, genes, geo, device, seed, entries, repeat, accum_batches):
        import torch
        if len(images) != len(genes) or not images:
            raise ValueError("TrainTileSet: one image array per gene tile")
        shp = images[0].shape
        if len(shp) != 3 or shp[0] % 2:
            raise ValueError(f"image tile must be [(s z), H, W] with two stains, got {shp}")
        self.zt, self.H, self.W = shp[0] // 2, shp[1], shp[2]
        dt = np.dtype(images[0].dtype)
        if dt not in (np.dtype(np.uint8), np.dtype(np.float16)):
            raise ValueError(f"image tiles must be uint8 or float16, got {dt}")
        crds, dats, rows, base = [], [], [], [0]
        for i, (im, (data, coords, shape)) in enumerate(zip(images, genes)):
            if im.shape != shp or np.dtype(im.dtype) != dt:
                raise ValueError(f"tile {i}: image {im.shape} {im.dtype}, expected {shp} {dt}")
            if tuple(shape) != (self.H, self.W, self.zt * GENES_PER_SLICE):
                raise ValueError(f"tile {i}: gene shape {tuple(shape)}, expected {(self.H, self.W, self.zt * GENES_PER_SLICE)}")
            c, d, r = sort_by_row(data, coords, self.H)
            if r[-1] >= 2 ** 31 - 1:
                raise ValueError(f"tile {i}: too many entries for an int32 row table")
            crds.append(c), dats.append(d), rows.append(r), base.append(base[-1] + d.shape[0])
        self.geo, self.dev, self.n_tiles = geo, torch.device(device), len(images)
        self.img_dtype = 0 if dt == np.dtype(np.uint8) else 1
        self.nnz = base[-1]
        self.img = torch.from_numpy(np.ascontiguousarray(np.stack(images))).to(self.dev)
        crd = np.concatenate(crds, axis=1) if self.nnz else np.zeros((3, 0), np.int32)
        self.crd = torch.from_numpy(np.ascontiguousarray(crd)).to(self.dev)
        self.dat = torch.from_numpy(np.concatenate(dats) if self.nnz else np.zeros(0, np.float32)).to(self.dev)
        self.tile_base = torch.tensor(base, dtype=torch.int64).to(self.dev)
        self.row_start = torch.from_numpy(np.stack(rows)).to(self.dev)
        ent = list(range(self.n_tiles)) if entries is None else list(entries)
        if repeat > 1:
            ent = list(itertools.chain(*itertools.repeat(ent, repeat)))
        self.sampler = TileSampler(ent, self.H, self.W, geo, seed, gmax=self.zt, accum_batches=accum_batches)

    def gather(self, params: np.ndarray, img=None, rna=None) -> TrainBatch:
        """The batch of the given int32 [B, 6] descriptors (img / rna: preallocated outputs, optional).  Queues one small upload and two kernels on the current stream and
        returns without waiting for them (no host synchronisation): the descriptors go up from pinned memory, the outputs
        come from torch's caching allocator."""
        import torch
        from . import _lib
        params = np.ascontiguousarray(params, dtype=np.int32)
        if params.ndim != 2 or params.shape[1] != 6:
            raise ValueError(f"descriptors must be [B, 6], got {params.shape}")
        B, g = params.shape[0], self.geo
        host = torch.from_numpy(params).pin_memory()
        desc = host.to(self.dev, non_blocking=True)
        gp = g.gs + 2 * g.pdim
        shp_i, shp_r = (B, g.img_channels, g.sdim, g.sdim), (B, gp, gp, g.snum * GENES_PER_SLICE)
        img = torch.empty(shp_i, dtype=torch.float32, device=self.dev) if img is None else img
        rna = torch.empty(shp_r, dtype=torch.float32, device=self.dev) if rna is None else rna
        for t, shp in ((img, shp_i), (rna, shp_r)):
            if tuple(t.shape) != shp or t.dtype != torch.float32 or t.device != self.dev or not t.is_contiguous():
                raise ValueError(f"output must be a contiguous fp32 {shp} tensor on {self.dev}")
        L, st = _lib.lib(), _lib.current_stream_ptr()
        with torch.cuda.device(self.dev):
            _lib.check(L.tm_train_batch_images(_lib.ptr(self.img), self.img_dtype, self.n_tiles, self.zt, self.H, self.W, _lib.ptr(desc),
                                               _lib.ptr(host), B, g.sdim, g.snum, STAIN_CODE[g.stain], _lib.ptr(img), st),
                       "tm_train_batch_images")
            _lib.check(L.tm_train_batch_genes(_lib.ptr(self.crd), _lib.ptr(self.dat), self.nnz, _lib.ptr(self.tile_base),
                                              _lib.ptr(self.row_start), self.n_tiles, self.zt, self.H, self.W, _lib.ptr(desc),
                                              _lib.ptr(host), B, g.sdim, g.gblk, g.pdim, g.snum, _lib.ptr(rna), st),
                       "tm_train_batch_genes")
        return TrainBatch(img, rna, params)

    def draw(self, batch: int, step: int, micro: int = 0, rank: int = 0, world: int = 1) -> TrainBatch:
        return self.gather(self.sampler.params(batch, step, micro, rank, world))
