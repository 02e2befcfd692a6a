"""Gene-gene attention read-out of the attention driver (reference test_attn.py:359-431, `--calc_attn`).

`run_attn_batch` is `Tester._run_batch` of test_attn re-stated over the HIP attention-map model:
z-chunk the gene tile into 25 windows of 4 slices, cut the 20x20 gene grid into 5x5 patches of 4x4
cells, get the four softmax maps per patch (tm_gene_attn), contract the maps of the selected pathway
genes `glst` with their counts, reassemble per tile and crop the half-patch frame.
The contractions are 2x2 / 4x2 matrices times 2x16 count blocks per patch -- host glue on device
tensors, not a kernel.

`run_attn_batch(..., fused=True)` takes the same read-out from tm_gene_attn_readout instead (one kernel per
batch, no G x G map is formed), and `AttnSweep` is the loop of test_attn.Tester.test / main
(test_attn.py:433-497) around it: the tile grid of an ROI, shared out over ranks by rows, one
'{r0}_{r1}_{c0}_{c1}.zip' float16 file per tile.
"""
import os
import queue
import threading
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import formats, tiles

PATHWAYS = {"GLUT": (75, 191), "DOPA": (5, 154), "BLOD": (94, 145)}      # gene indices, SURVEY.md section 2


def pathway_readout(attn: torch.Tensor, rna_mid: torch.Tensor, glst: Sequence[int]) -> torch.Tensor:
    """attn [4, B, G, G] (3 slice-pair maps + ensemble), rna_mid [B, G, 2, gh, gw] (middle slices) ->
    [B, 4 + 2 + 2, 2*gh*gw]: slice-pair products, ensemble product, raw counts (test_attn.py:404-423)."""
    g = list(glst)
    B = attn.shape[1]
    sub = attn[:, :, g][..., g]                                  # [4, B, 2, 2]
    rna = rna_mid[:, g]                                          # [B, 2, 2, gh, gw]
    rna0, rna1 = rna[:, :, 0].reshape(B, len(g), -1), rna[:, :, 1].reshape(B, len(g), -1)
    att0 = sub[:2].permute(1, 0, 2, 3).reshape(B, 2 * len(g), len(g))       # 'd b c g -> b (d c) g'
    att1 = sub[1:3].permute(1, 0, 2, 3).reshape(B, 2 * len(g), len(g))
    out = torch.cat([att0 @ rna0, att1 @ rna1], -1)              # [B, 4, 2*gh*gw]
    rna2 = rna.reshape(B, len(g), -1)
    return torch.cat([out, sub[3] @ rna2, rna2], 1)


def assemble_readout(out: torch.Tensor, b: int, p1: int, p2: int, gn: int) -> torch.Tensor:
    """'(n_z b p1 p2) g (z h w) -> b (n_z z) g (p1 h) (p2 w)' then crop gn//2 cells (test_attn.py:424-427)."""
    n, g, zhw = out.shape
    z = zhw // (gn * gn)
    nz = n // (b * p1 * p2)
    t = out.reshape(nz, b, p1, p2, g, z, gn, gn).permute(1, 0, 5, 4, 2, 6, 3, 7)
    t = t.reshape(b, nz * z, g, p1 * gn, p2 * gn)
    pad = gn // 2
    return t[:, :, :, pad:-pad, pad:-pad]


def run_attn_batch(model, rna_tile: torch.Tensor, glst: Sequence[int], z_size: int = 4, gn: int = 4,
                   fused: bool = False) -> torch.Tensor:
    """rna_tile dense [b, 20, 20, (50+2)*500] -> fp16 [b, 50, 4K, 16, 16] (what the reference saves per tile).
    fused: the read-out comes from model.readout (tm_gene_attn_readout) instead of the four maps."""
    b = rna_tile.shape[0]
    rna = tiles.zchunk_rna(rna_tile, z_size)
    p1, p2 = rna.shape[1] // gn, rna.shape[2] // gn
    rna = tiles.patchify_hwc(rna, gn, False)
    if fused:
        out = model.readout(rna, glst)
    else:
        attn, mid = model.forward(x=None, t=None, rna=rna, imgs=None)
        out = pathway_readout(attn, mid, glst)
    return assemble_readout(out, b, p1, p2, gn).half()


# ---- ROI arithmetic of test_attn.main (test_attn.py:465-478) as data ------------------------------------------
# utils/__init__.py:73-89 `MROI` per mouse: (slst = the slices shown, size, pos = the four regions' [row, col]); the gene
# NAMES of a region need the reference's gene csv and are not restated: callers pass gene indices.
REGIONS = {
    "609882": (list(range(21, 29)), 128, [[160, 1440], [160, 1888], [544, 1152], [512, 2048]]),
    "609889": (list(range(15, 23)), 128, [[160, 1440], [160, 1888], [576, 1208], [560, 1960]]),
    "638850": (list(range(16, 24)), 128, [[672, 920], [672, 2296], [176, 1320], [216, 2096]]),
}


def region_args(mouse: str, region: int) -> dict:
    """`--region r` of test_attn: hst / wst = pos * 32, hnm = wnm = size // 8 tiles, slst = the mouse's slice list."""
    slst, size, pos = REGIONS[mouse]
    return {"hst": pos[region][0] * 32, "wst": pos[region][1] * 32, "hnm": size // 8, "wnm": size // 8, "slst": list(slst)}


def pathway_args(path: str) -> dict:
    """`--path GLUT|DOPA|BLOD` of test_attn (region -1): the whole brain, all 50 slices, the pathway's gene pair."""
    return {"hst": 256, "wst": 256, "hnm": 286, "wnm": 414, "slst": list(range(50)), "glst": list(PATHWAYS[path])}


ZIP_DATE = (1980, 1, 1, 0, 0, 0)        # member time stamp of the tile files: a tile's bytes depend on its values alone


def attn_tile_name(hst: int, wst: int, r: int, c: int, size: int = tiles.TILE) -> str:
    """'{r0}_{r1}_{c0}_{c1}' of the tile at ROI grid position (r, c): the first four numbers of its gene tile's name
    (test_attn.py:428-431 saves under the dataset's `roi`)."""
    r0, c0 = hst + r * size, wst + c * size
    return f"{r0}_{r0 + size}_{c0}_{c0 + size}"


class AttnSweep:
    """test_attn.Tester.test over an hnm x wnm tile ROI.  Tile rows are shared out with tiles.row_block_partition; tiles are
    independent, so ranks neither exchange nor reduce anything.  `gene_provider(row, col)` (absolute grid position, what
    TileSweep takes) returns the dense [20, 20, 52*500] gene tile.  Every tile's [50, 4K, 16, 16] float16 result is written
    as '{r0}_{r1}_{c0}_{c1}.zip' (zarr v2, fixed member time stamp: the same tile gives the same bytes) into out_dir.

    Write-back: a batch's result is copied to a pinned host buffer on a side stream (the compute stream only records an event
    and goes on with the next batch), and a writer thread waits for that copy and writes the zip files; two buffers rotate, so
    the GPU waits for the writer only when it is two batches behind."""

    def __init__(self, conf, model, gene_provider: Optional[Callable[[int, int], torch.Tensor]], glst: Sequence[int],
                 hst: int, wst: int, hnm: int, wnm: int, out_dir=None, rank: int = 0, world: int = 1, batch_tiles: int = 4,
                 fused: bool = True, device=None):
        if conf.rna_slc != 4:
            raise NotImplementedError("the attention read-out is defined for rna_slc = 4")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside [0, {world})")
        self.conf, self.model, self.gene, self.glst = conf, model, gene_provider, [int(g) for g in glst]
        self.hst, self.wst, self.hnm, self.wnm = hst, wst, hnm, wnm
        self.row0, self.col0 = hst // tiles.TILE, wst // tiles.TILE
        self.out_dir, self.rank, self.world = out_dir, rank, world
        self.batch_tiles, self.fused = max(1, int(batch_tiles)), fused
        self.dev = torch.device(device) if device is not None else (model.device if model is not None else None)
        self.r0, self.r1 = tiles.row_block_partition(hnm, world)[rank]
        self.bytes_written, self.tiles_done = 0, 0

    def tile_list(self) -> List[Tuple[int, int]]:
        """(r, c) ROI grid positions of this rank's tiles, row-major."""
        return [(r, c) for r in range(self.r0, self.r1) for c in range(self.wnm)]

    def tile_path(self, r: int, c: int) -> str:
        return os.path.join(str(self.out_dir), attn_tile_name(self.hst, self.wst, r, c) + ".zip")

    def run_batch(self, batch: Sequence[Tuple[int, int]]) -> torch.Tensor:
        """fp16 [len(batch), 50, 4K, 16, 16] on the device."""
        rna = torch.stack([self.gene(self.row0 + r, self.col0 + c).to(self.dev) for r, c in batch])
        return run_attn_batch(self.model, rna, self.glst, self.conf.rna_slc, self.conf.gn_sz, fused=self.fused)

    def _writer(self, q, errs):
        while True:
            item = q.get()
            if item is None:
                return
            ev, host, batch, free = item
            try:
                ev.synchronize()
                arr = host.numpy()
                for i, (r, c) in enumerate(batch):
                    p = self.tile_path(r, c)
                    formats.write_zarr_zip(p, arr[i], date_time=ZIP_DATE)
                    self.bytes_written += os.path.getsize(p)
            except Exception as e:                      # surfaced by run()
                errs.append(e)
            finally:
                free.set()

    def run(self, write: bool = True) -> dict:
        """Sweep this rank's tiles.  write=False computes every tile and drops the result (measurement)."""
        todo = self.tile_list()
        write = write and self.out_dir is not None
        if write:
            os.makedirs(str(self.out_dir), exist_ok=True)
        side = torch.cuda.Stream(self.dev) if write else None
        K = len(self.glst)
        bufs, frees, q, errs, th = [], [], queue.Queue(), [], None
        if write:
            for _ in range(2):
                bufs.append(torch.empty((self.batch_tiles, 50, 4 * K, 16, 16), dtype=torch.float16).pin_memory())
                f = threading.Event()
                f.set()
                frees.append(f)
            th = threading.Thread(target=self._writer, args=(q, errs), daemon=True)
            th.start()
        try:
            for k, i0 in enumerate(range(0, len(todo), self.batch_tiles)):
                batch = todo[i0:i0 + self.batch_tiles]
                out = self.run_batch(batch)
                self.tiles_done += len(batch)
                if not write:
                    continue
                host, free = bufs[k % 2][:len(batch)], frees[k % 2]
                free.wait()
                free.clear()
                side.wait_stream(torch.cuda.current_stream(self.dev))
                with torch.cuda.stream(side):
                    host.copy_(out, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(side)
                out.record_stream(side)
                q.put((ev, host, batch, free))
        finally:
            if th is not None:
                q.put(None)
                th.join()
        torch.cuda.synchronize(self.dev)
        if errs:
            raise errs[0]
        return {"tiles": self.tiles_done, "bytes_written": self.bytes_written, "rows": (self.r0, self.r1)}
