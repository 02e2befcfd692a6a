#!/usr/bin/env python3
"""How good is a generated ROI: PSNR, SSIM and MS-SSIM of every slice against the real tiles.

Reads what the reference's `test_brn.gen_img(gdir, rdir, ...)` (test_brn.py:73-121) reads: a generated step directory
('{r0}_{r1}_{c0}_{c1}.zip' state tiles) and a directory of real tiles (eight-number names, 128-px frame), stitches both
(`stitch.stitch_dir`, `stitch.stitch_real_dir`) and compares them plane by plane on the GPU (`metrics.compare_mosaics`: one
plane pair resident at a time, as `stitch.save_slices_pyramid` uploads).  Writes a JSON report: one row per '(s c)' plane
(slice-major, stain-minor) and the means per stain.  A PSNR of equal planes is Infinity in the report.  The side-by-side JPEGs
of gen_img are not written.

--volume adds "volumes": one row per stain with the measures of the 3-D window over the stain's whole slice stack
(`metrics.compare_volumes`: psnr3d, ssim3d, ms_ssim3d), which see what no single plane shows: neighbouring slices that do not
match, a seam between z-chunks, slices out of order.  It needs every slice, so it is refused together with --slices."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def evaluate(gen_dir, real_dir, hst, wst, hnm, wnm, slc=50, slices=None, n_stain=2, ms=True, size=256, tile_decoder="host",
             volume=False):
    if volume and slices is not None:
        raise ValueError("--volume measures every slice of a stain: it cannot be combined with --slices")
    import teramind_amd  # noqa: F401
    from teramind_amd import metrics, stitch
    gen = stitch.stitch_dir(gen_dir, hst, wst, hnm, wnm, slc=slc, slices=slices, size=size, decoder=tile_decoder)
    real = stitch.stitch_real_dir(real_dir, hst, wst, hnm, wnm, slc=slc, slices=slices, size=size, decoder=tile_decoder)
    if gen.shape != real.shape:
        raise SystemExit(f"generated mosaic {gen.shape} and real mosaic {real.shape} differ")
    rows = metrics.compare_mosaics(gen, real, ms=ms)
    picks = list(range(gen.shape[0])) if slices is None else list(slices)
    planes = []
    for k, idx in enumerate(picks):
        s, c = divmod(idx, n_stain)
        planes.append(dict({"plane": idx, "slice": s, "stain": c}, **{m: v[k] for m, v in rows.items()}))
    means = []
    for c in sorted({p["stain"] for p in planes}):
        sel = [p for p in planes if p["stain"] == c]
        means.append(dict({"stain": c, "planes": len(sel)}, **{m: sum(p[m] for p in sel) / len(sel) for m in rows}))
    rep = {"gen_dir": str(gen_dir), "real_dir": str(real_dir), "roi": [hst, wst, hnm, wnm], "shape": list(gen.shape[1:]),
           "measures": sorted(rows), "planes": planes, "mean_per_stain": means}
    if volume:
        vols = metrics.compare_volumes(gen, real, n_stain=n_stain, ms=ms)
        rep["volumes"] = [dict({"stain": c, "slices": gen.shape[0] // n_stain}, **{m: v[c] for m, v in vols.items()})
                          for c in range(n_stain)]
    return rep


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gen_dir", required=True, help="generated step directory ('{r0}_{r1}_{c0}_{c1}.zip')")
    ap.add_argument("--real_dir", required=True, help="real tiles (eight-number names, [(c s), 512, 512])")
    ap.add_argument("--hst", type=int, required=True)
    ap.add_argument("--wst", type=int, required=True)
    ap.add_argument("--hnm", type=int, required=True)
    ap.add_argument("--wnm", type=int, required=True)
    ap.add_argument("--slc", type=int, default=50, help="slices per stain in a tile")
    ap.add_argument("--slices", type=int, nargs="*", default=None, help="indices into the '(s c)' order (default all)")
    ap.add_argument("--n_stain", type=int, default=2, help="stains per slice, for the slice / stain columns of the report")
    ap.add_argument("--no_ms", action="store_true", help="skip MS-SSIM")
    ap.add_argument("--tile_decoder", choices=["host", "gpu"], default="host",
                    help="decode the tile files on the host, or their Blosc-lz4 chunks on the GPU (the mosaics then never leave it)")
    ap.add_argument("--volume", action="store_true",
                    help="add the 3-D-window measures of every stain's slice stack ('volumes' in the report); not with --slices")
    ap.add_argument("--out", required=True, help="report.json")
    a = ap.parse_args()
    try:
        rep = evaluate(a.gen_dir, a.real_dir, a.hst, a.wst, a.hnm, a.wnm, a.slc, a.slices, a.n_stain, not a.no_ms,
                       tile_decoder=a.tile_decoder, volume=a.volume)
    except ValueError as e:                                 # the one refusal evaluate() makes of its arguments
        ap.error(str(e))
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({"out": a.out, "planes": len(rep["planes"]), "mean_per_stain": rep["mean_per_stain"]}))
