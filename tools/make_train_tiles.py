#!/usr/bin/env python3
"""Writes a small synthetic training tile directory in the reference's file layout (utils/MBADataset.py:70,101:
`<out>/gene/tile_XXXX.npz` COO archives + `<out>/img/tile_XXXX.zip` zarr arrays), for the tests and for a first run of
tools/train.py.  Run:  python tools/make_train_tiles.py --out /tmp/tiles --tiles 2"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import teramind_amd  # noqa: E402,F401
from teramind_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--tiles", type=int, default=2)
    ap.add_argument("--size", type=int, default=512, help="tile edge in pixels")
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--nnz", type=int, default=200000, help="transcript entries per tile")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    for p in synth.write_train_tile_dir(a.out, a.tiles, a.size, a.size, a.slices, a.nnz, a.seed):
        print(p)


if __name__ == "__main__":
    main()
