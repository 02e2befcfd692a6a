#!/usr/bin/env python3
"""End-to-end run of the `test_attn --calc_attn` + `infer_attn` flow: gene tiles of an hnm x wnm ROI (a directory of the
reference's COO '.npz' gene tiles through brain.GeneTileDir, or --synthetic device-resident tiles) -> attn_maps.AttnSweep
(fused read-out kernel, one float16 '{r0}_{r1}_{c0}_{c1}.zip' per tile) -> stitch.stitch_attn_dir -> 'all_{sl}.zip' per
slice (test_attn.py:433-497, infer_attn.py:9-39).  Hashed weights unless the caller loads a checkpoint into the model.
`--gpus N` starts N rank processes through launch.spawn_ranks (one per GPU; tile rows are split over them, no exchange);
the calling process never opens a GPU itself in that case.  `--heatmap MODE` also writes every slice of the mosaic as a
colour-mapped pyramid (stitch.save_attn_heatmaps_pyramid) into 'heat_{path}_{mode}' next to 'attn_{path}_all' ('expr': one
directory per gene, 'heat_{path}_expr_g{k}').  Prints one JSON line (measured at the stated ROI size)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(args):
    import torch
    import teramind_amd  # noqa: F401
    from teramind_amd import attn_maps, heatmap, launch, stitch
    from teramind_amd.brain import GeneTileDir, device_gene_provider
    from teramind_amd.config import PathConfig
    from teramind_amd.unet import GeneAttnModel
    from teramind_amd.weights import hashed_state_dict

    rank, local_rank, world = launch.dist_env()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        launch.init_distributed("gloo", None)                    # only the final barrier: tiles are independent
    cfg = PathConfig()
    model = GeneAttnModel(cfg, dev).load_state_dict(hashed_state_dict(cfg, 0, vis_only=True), strict=False)
    glst = [int(v) for v in args.glst.split(",")] if args.glst else list(attn_maps.PATHWAYS[args.path])
    if args.synthetic or not args.gene_dir:
        genes = device_gene_provider(cfg, dev, density=args.density)
    else:
        genes = GeneTileDir(args.gene_dir, cfg, dev, total_slc=50, keep_resident=True)
    out_dir = args.out_dir or tempfile.mkdtemp(prefix="attn_roi_")
    tdir = os.path.join(out_dir, f"attn_{args.path}")
    sw = attn_maps.AttnSweep(cfg, model, genes, glst, args.hst, args.wst, args.hnm, args.wnm, tdir, rank=rank, world=world,
                             batch_tiles=args.batch_tiles, fused=not args.unfused)
    if args.prefetch:                                            # gene tiles resident before the timed region
        for r, c in sw.tile_list():
            genes(sw.row0 + r, sw.col0 + c)
    sw.run_batch(sw.tile_list()[:1])                             # warm-up: code objects, workspace
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = sw.run(write=not args.no_tile_files)
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    total = time.perf_counter() - t0
    if rank == 0:
        stitch_s, shape = None, None
        if not args.no_tile_files:
            t1 = time.perf_counter()
            mosaic = stitch.stitch_attn_dir(tdir, args.hst, args.wst, args.hnm, args.wnm)
            stitch.save_attn_slices(mosaic, os.path.join(out_dir, f"attn_{args.path}_all"))
            stitch_s, shape = round(time.perf_counter() - t1, 3), list(mosaic.shape)
        heat = {}
        if args.heatmap:
            t2 = time.perf_counter()
            path = None if args.glst else args.path              # the reference's palettes and scales belong to its gene pairs
            kw = dict(K=len(glst), mode=args.heatmap, vmax=args.heat_vmax, sigma=args.heat_sigma, scale=args.heat_scale,
                      wei=heatmap.gene_weight(cfg.rna_num), path=path, device=dev)
            dirs = []
            if args.heatmap == "expr":
                for k in range(len(glst)):
                    dirs.append(os.path.join(out_dir, f"heat_{args.path}_expr_g{k}"))
                    stitch.save_attn_heatmaps_pyramid(mosaic, dirs[-1], gene=k, **kw)
            else:
                dirs.append(os.path.join(out_dir, f"heat_{args.path}_{args.heatmap}"))
                stitch.save_attn_heatmaps_pyramid(mosaic, dirs[-1], **kw)
            torch.cuda.synchronize(dev)
            heat = {"heatmap": args.heatmap, "heatmap_s": round(time.perf_counter() - t2, 3),
                    "heatmap_files": sum(len(os.listdir(d)) for d in dirs)}
        tiles = args.hnm * args.wnm
        print(json.dumps({"what": "attention read-out sweep, measured", "tiles": tiles, "rank0_tiles": res["tiles"], "n_gpus": world,
                          "glst": glst, "fused": not args.unfused, "batch_tiles": args.batch_tiles,
                          "genes": "synthetic, device resident" if (args.synthetic or not args.gene_dir) else "GeneTileDir",
                          "prefetched": bool(args.prefetch), "tile_files_written": not args.no_tile_files,
                          "seconds": round(total, 4), "rank0_sweep_s": round(dt, 4), "tiles_per_s": round(tiles / total, 2),
                          "bytes_written_rank0": res["bytes_written"], "stitch_s": stitch_s, "mosaic_shape": shape,
                          "out_dir": out_dir, **heat}), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--hst", type=int, default=256)
    ap.add_argument("--wst", type=int, default=256)
    ap.add_argument("--hnm", type=int, default=2)
    ap.add_argument("--wnm", type=int, default=8)
    ap.add_argument("--path", choices=["GLUT", "DOPA", "BLOD"], default="GLUT")
    ap.add_argument("--glst", default=None, help="comma-separated gene indices (1..8 of them) instead of --path's pair")
    ap.add_argument("--gene_dir", default=None)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--batch_tiles", type=int, default=4)
    ap.add_argument("--prefetch", type=int, default=1, help="1: make every gene tile resident before the timed sweep")
    ap.add_argument("--unfused", action="store_true", help="the four-map path (tm_gene_attn + torch gather), for comparison")
    ap.add_argument("--no_tile_files", action="store_true", help="compute every tile, write nothing")
    ap.add_argument("--out_dir", default=None)
    ap.add_argument("--heatmap", choices=["att_all", "att_up", "att_dn", "expr"], default=None,
                    help="also write the slices as colour-mapped pyramids of this field (test_attn.gen_img)")
    ap.add_argument("--heat_scale", type=int, default=4, choices=[1, 2, 4, 8, 16], help="pixels per mosaic cell")
    ap.add_argument("--heat_sigma", type=float, default=2.0)
    ap.add_argument("--heat_vmax", type=float, default=None,
                    help="upper end of the colour scale (default: the reference's for --path; required for att_up / att_dn and with --glst)")
    args = ap.parse_args()
    if args.heatmap and args.no_tile_files:
        ap.error("--heatmap draws the stitched mosaic: it needs the tile files (drop --no_tile_files)")
    from teramind_amd import launch
    if args.gpus > 1 and not launch.launched_as_rank():
        sys.exit(launch.spawn_ranks(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))
    worker(args)


if __name__ == "__main__":
    main()
