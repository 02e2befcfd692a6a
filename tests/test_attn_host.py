"""Host logic of the attention sweep (no GPU): the stitcher of the read-out tiles against a numpy restatement of
infer_attn.gen_col + gen_mba, the ROI arithmetic of test_attn.main against the reference's literal numbers, and the rank
shares of AttnSweep."""
import os

import numpy as np
import pytest

from teramind_amd import attn_maps, formats, stitch
from teramind_amd.config import PathConfig

# utils/__init__.py:73-89 (slices, size, positions) and test_attn.py:465-478, copied as data
MROI_NUMBERS = {
    "609882": (list(range(21, 29)), 128, [[160, 1440], [160, 1888], [544, 1152], [512, 2048]]),
    "609889": (list(range(15, 23)), 128, [[160, 1440], [160, 1888], [576, 1208], [560, 1960]]),
    "638850": (list(range(16, 24)), 128, [[672, 920], [672, 2296], [176, 1320], [216, 2096]]),
}


def _tiles(tmp, hst, wst, hnm, wnm, K=2, size=256):
    rng = np.random.default_rng(7)
    d = os.path.join(str(tmp), "tiles")
    os.makedirs(d)
    made = {}
    for ph in range(hnm):
        for pw in range(wnm):
            a = rng.standard_normal((50, 4 * K, 16, 16)).astype(np.float16)
            r0, c0 = hst + ph * size, wst + pw * size
            formats.write_zarr_zip(os.path.join(d, f"{r0}_{r0 + size}_{c0}_{c0 + size}.zip"), a)
            made[(ph, pw)] = a
    return d, made


@pytest.mark.parametrize("hst,wst,hnm,wnm", [(256, 256, 3, 2), (5120, 46080, 1, 4)])
def test_stitch_attn_dir_is_gen_col_then_gen_mba(tmp_path, hst, wst, hnm, wnm):
    d, made = _tiles(tmp_path, hst, wst, hnm, wnm)
    # infer_attn.py:9-39: gen_col concatenates a tile column on axis -2 (and files it per slice), gen_mba joins the columns on -1
    cols = [np.concatenate([made[(ph, pw)] for ph in range(hnm)], -2) for pw in range(wnm)]
    per_slice = [np.concatenate([col[sl] for col in cols], -1) for sl in range(50)]
    mosaic = stitch.stitch_attn_dir(d, hst, wst, hnm, wnm)
    assert mosaic.dtype == np.float16 and mosaic.shape == (50, 8, hnm * 16, wnm * 16)
    for sl in range(50):
        assert np.array_equal(mosaic[sl].view(np.uint16), per_slice[sl].view(np.uint16))
    odir = os.path.join(str(tmp_path), "all")
    stitch.save_attn_slices(mosaic, odir)
    assert sorted(os.listdir(odir)) == sorted(f"all_{sl}.zip" for sl in range(50))
    for sl in (0, 17, 49):
        back = formats.read_zarr_zip(os.path.join(odir, f"all_{sl}.zip"))
        assert back.dtype == np.float16 and np.array_equal(back.view(np.uint16), per_slice[sl].view(np.uint16))
    stitch.save_attn_slices(mosaic[[3, 4]], os.path.join(str(tmp_path), "two"), names=[21, 22])
    assert sorted(os.listdir(os.path.join(str(tmp_path), "two"))) == ["all_21.zip", "all_22.zip"]


def test_stitch_attn_dir_missing_tile_fails(tmp_path):
    d, _ = _tiles(tmp_path, 256, 256, 2, 2)
    os.remove(os.path.join(d, "512_768_256_512.zip"))
    with pytest.raises(Exception):
        stitch.stitch_attn_dir(d, 256, 256, 2, 2)


def test_region_args_match_the_reference_numbers():
    for mouse, (slst, size, pos) in MROI_NUMBERS.items():
        for region in range(4):
            a = attn_maps.region_args(mouse, region)
            assert a == {"hst": pos[region][0] * 32, "wst": pos[region][1] * 32, "hnm": size // 8, "wnm": size // 8, "slst": slst}
            assert a["hst"] % 256 == 0 and a["wst"] % 256 == 0          # whole tiles: the gene tile names exist
    assert attn_maps.region_args("638850", 0) == {"hst": 21504, "wst": 29440, "hnm": 16, "wnm": 16, "slst": list(range(16, 24))}


def test_pathway_args_match_the_reference_numbers():
    for path, glst in (("GLUT", [75, 191]), ("DOPA", [5, 154]), ("BLOD", [94, 145])):
        assert attn_maps.pathway_args(path) == {"hst": 256, "wst": 256, "hnm": 286, "wnm": 414, "slst": list(range(50)),
                                                "glst": glst}


def test_attn_tile_name_is_the_gene_tile_prefix():
    from teramind_amd import tiles
    names = tiles.gene_tile_names(hst=512, wst=768, hnm=2, wnm=3)
    got = {attn_maps.attn_tile_name(512, 768, r, c) for r in range(2) for c in range(3)}
    assert got == {"_".join(n.split("_")[:4]) for n in names}


@pytest.mark.parametrize("rows", [8, 286])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_rank_shares_cover_the_grid_once(rows, world):
    wnm = 5
    seen = []
    for rank in range(world):
        sw = attn_maps.AttnSweep(PathConfig(), None, None, (75, 191), 256, 256, rows, wnm, None, rank=rank, world=world)
        mine = sw.tile_list()
        assert mine == sorted(mine) and len({r for r, _ in mine}) in (rows // world, rows // world + 1)
        seen += mine
    assert sorted(seen) == [(r, c) for r in range(rows) for c in range(wnm)] and len(set(seen)) == len(seen)


def test_attn_sweep_rejects_bad_rank_and_config():
    with pytest.raises(ValueError):
        attn_maps.AttnSweep(PathConfig(), None, None, (75, 191), 256, 256, 4, 4, None, rank=2, world=2)
    with pytest.raises(NotImplementedError):
        attn_maps.AttnSweep(PathConfig(rna_slc=8), None, None, (75, 191), 256, 256, 4, 4, None)
