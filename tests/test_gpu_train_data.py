"""GPU: tm_train_batch_images / tm_train_batch_genes (csrc/tm_io.hip) through dataset.TrainTileSet, bit for bit against
  * a torch restatement of MBADataset._getimg / _trans / `im / 127.5 - 1` (utils/MBADataset.py:100-118,143,154-166),
  * the reference's OWN _getimg / _trans output (tests/golden/train_data_ref.npz, tools/make_train_data_golden.py),
  * a dense numpy restatement of the gene path: densify, crop, reshape(...).sum((1, 3)), channel pad + window, rot90 / flip on
    the [g, h, w] view, pad by pdim -- the identity the reference asserts about its own COO code in _gene_test /
    _trans_test_sp (:172-199).  The gene half of the reference itself needs the `sparse` package, which is absent.
Every output is filled with NaN before the call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import train_data_cases as tc
from teramind_amd import _lib, synth
from teramind_amd.dataset import TrainGeometry, TrainTileSet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAD = {1: 0, 4: 1, 8: 1, 16: 3}
ZT, H, W, SDIM = 12, 80, 72, 64


def gather_nan(ts, params):
    g, B = ts.geo, len(params)
    gp = g.gs + 2 * g.pdim
    img = torch.full((B, g.img_channels, g.sdim, g.sdim), float("nan"), device=DEV)
    rna = torch.full((B, gp, gp, g.snum * 500), float("nan"), device=DEV)
    bt = ts.gather(np.asarray(params, dtype=np.int32), img=img, rna=rna)
    torch.cuda.synchronize()
    return bt


def ref_image(tile, geo, top, left, snm, rot, flip):
    """MBADataset._getimg + the image half of _trans + scaling, restated with the same numpy / torch calls."""
    sd, snum = geo.sdim, geo.snum
    im = tile[:, top:top + sd, left:left + sd]
    im = im.reshape(2, -1, sd, sd)
    if geo.stain == "DAPI":
        im = im[[0]]
    elif geo.stain == "PolyT":
        im = im[[1]]
    shf = snum // 4 if snum > 1 else 0
    if snum > 1:
        pd = np.zeros((im.shape[0], SPAD[snum], sd, sd))
        im = np.concatenate((pd, im, pd), 1)
    im = im[:, snm + shf:snm + snum - shf]
    im = torch.from_numpy(np.ascontiguousarray(im.reshape(-1, sd, sd))).float()
    im = torch.rot90(im, rot, [1, 2])
    if flip:
        im = im.flip(-1)
    return im / 127.5 - 1


def ref_genes(gene, geo, top, left, snm, rot, flip):
    """Dense restatement of _getgene + the gene half of _trans + _to_sparse(pad) + to_dense().  Only the crop window of the
    tile is densified (the whole tile would be H * W * zt * 500 floats); entries outside it cannot reach the result."""
    data, crd, shape = gene
    sd, gb, snum = geo.sdim, geo.gblk, geo.snum
    inside = (crd[0] >= top) & (crd[0] < top + sd) & (crd[1] >= left) & (crd[1] < left + sd)
    crop = np.zeros((sd, sd, shape[2]), dtype=np.float64)
    np.add.at(crop, (crd[0][inside] - top, crd[1][inside] - left, crd[2][inside]), np.asarray(data)[inside].astype(np.float64))
    gs = sd // gb
    gn = crop.reshape(gs, gb, gs, gb, -1).sum((1, 3))
    if snum > 1:
        z = np.zeros((gs, gs, SPAD[snum] * 500))
        gn = np.concatenate((z, gn, z), -1)
    gn = gn[:, :, snm * 500:(snm + snum) * 500]
    v = torch.from_numpy(np.ascontiguousarray(gn.transpose(2, 0, 1)))
    v = torch.rot90(v, rot, [1, 2])
    if flip:
        v = v.flip(-1)
    out = torch.zeros((gs + 2 * geo.pdim, gs + 2 * geo.pdim, snum * 500), dtype=torch.float64)
    out[geo.pdim:geo.pdim + gs, geo.pdim:geo.pdim + gs] = v.permute(1, 2, 0)
    return out.float()


def small_set(geo, dtype=np.uint8, nnz=6000, n_tiles=2, seed=0):
    tiles = [synth.image_tile(f"td/img{i}", (2 * ZT, H, W), seed, np.uint8) for i in range(n_tiles)]
    if dtype == np.float16:
        tiles = [(t.astype(np.float32) * 0.5).astype(np.float16) for t in tiles]      # halves: exact in fp16
    genes = [synth.train_gene_tile(f"td/gene{i}", H, W, ZT, nnz, seed) for i in range(n_tiles)]
    return TrainTileSet.from_arrays(tiles, genes, geo, DEV), tiles, genes


def border_params(snum):
    """Crops touching all four borders, snm at both ends, every rot x flip."""
    smax = ZT + 2 * SPAD[snum] - snum
    corners = [(0, 0), (0, W - SDIM), (H - SDIM, 0), (H - SDIM, W - SDIM), (7, 3)]
    p = []
    for k, (rot, flip) in enumerate((r, f) for r in range(4) for f in (0, 1)):
        top, left = corners[k % len(corners)]
        p.append((k % 2, top, left, (0, smax, smax // 2)[k % 3], rot, flip))
    p += [(1, H - SDIM, W - SDIM, 0, 1, 1), (0, 0, 0, smax, 3, 0), (1, 0, W - SDIM, smax, 2, 1), (0, H - SDIM, 0, 0, 0, 1)]
    return p


@pytest.mark.parametrize("dtype", [np.uint8, np.float16], ids=["u8", "f16"])
@pytest.mark.parametrize("snum", [1, 4, 8, 16])
@pytest.mark.parametrize("stain", ["all", "DAPI", "PolyT"])
def test_images_equal_torch_restatement(stain, snum, dtype):
    geo = TrainGeometry(sdim=SDIM, gblk=16, pdim=2, snum=snum, stain=stain)
    ts, tiles, _ = small_set(geo, dtype, nnz=100)
    params = border_params(snum)
    bt = gather_nan(ts, params)
    assert bt.img.shape == (len(params), geo.img_channels, SDIM, SDIM)
    got = bt.img.cpu()
    for b, (tile, top, left, snm, rot, flip) in enumerate(params):
        ref = ref_image(tiles[tile], geo, top, left, snm, rot, flip)
        assert torch.equal(got[b], ref), (b, params[b], float((got[b] - ref).abs().max()))


def test_images_equal_the_reference_dataset():
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_data_ref.npz"))
    tile = synth.image_tile(tc.REF_TAG, tc.REF_SHAPE, tc.REF_SEED)
    empty = (np.zeros(0, np.uint16), np.zeros((3, 0), np.int64), (tc.REF_H, tc.REF_W, tc.REF_ZT * 500))
    n = 0
    for stain in tc.STAINS:
        for snum in tc.SNUMS:
            geo = TrainGeometry(sdim=tc.REF_SDIM, gblk=16, pdim=0, snum=snum, stain=stain)
            ts = TrainTileSet.from_arrays([tile], [empty], geo, DEV)
            draws = gold[f"img/{stain}/{snum}/draws"]
            assert [tuple(d) for d in draws] == tc.ref_draws(snum)
            params = [(0, int(t), int(l), int(s), 0, 0) for t, l, s in draws]
            got = gather_nan(ts, params).img.cpu()
            ref = torch.from_numpy(gold[f"img/{stain}/{snum}/out"])
            assert got.shape == ref.shape and torch.equal(got, ref), (stain, snum)
            n += len(params)
            if (stain, snum) == (tc.TRANS_STAIN, tc.TRANS_SNUM):
                t, l, s = (int(v) for v in gold["trans/draw"])
                for rot in range(4):
                    for flip in (0, 1):
                        got = gather_nan(ts, [(0, t, l, s, rot, flip)]).img.cpu()[0]
                        assert torch.equal(got, torch.from_numpy(gold[f"trans/{rot}/{flip}"])), (rot, flip)
                        n += 1
    assert n == 3 * 4 * 3 + 8


@pytest.mark.parametrize("gblk", [8, 16, 32])
@pytest.mark.parametrize("snum", [1, 4, 8, 16])
def test_genes_equal_dense_restatement(snum, gblk):
    geo = TrainGeometry(sdim=SDIM, gblk=gblk, pdim=2, snum=snum)
    ts, _, genes = small_set(geo, nnz=20000)
    params = border_params(snum)
    bt = gather_nan(ts, params)
    got = bt.rna.cpu()
    assert not torch.isnan(got).any()
    for b, (tile, top, left, snm, rot, flip) in enumerate(params):
        ref = ref_genes(genes[tile], geo, top, left, snm, rot, flip)
        assert torch.equal(got[b], ref), (b, params[b], float((got[b] - ref).abs().sum()))
    assert float(got.sum()) > 0
    # the reference's tuple, rebuilt through torch.sparse_coo_tensor(...).to_dense() (experiment.py:129)
    im, dat, crd, ssz, lab = bt.as_coo()
    assert crd.dtype == torch.int64 and crd.shape[0] == 4 and lab.shape == (len(params),) and im is bt.img
    assert torch.equal(torch.sparse_coo_tensor(crd, dat, ssz).to_dense(), bt.rna)
    lin = ((crd[0] * ssz[1] + crd[1]) * ssz[2] + crd[2]) * ssz[3] + crd[3]
    assert bool((lin[1:] > lin[:-1]).all())                        # row-major order


def test_genes_on_and_beside_the_crop_border():
    geo = TrainGeometry(sdim=SDIM, gblk=16, pdim=2, snum=4)
    top, left, snm = 9, 5, 3
    edge_h = [top - 1, top, top + SDIM - 1, top + SDIM]
    edge_w = [left - 1, left, left + SDIM - 1, left + SDIM]
    # channels: first / last inside the slice window [snm, snm + 4) of the padded stack (= slices snm - 1 .. snm + 2), one beside each
    chans = [(snm - 1) * 500 - 1, (snm - 1) * 500, (snm + 3) * 500 - 1, (snm + 3) * 500]
    crd = np.array([(h, w, c) for h in edge_h for w in edge_w for c in chans], dtype=np.int64).T
    base_in = np.isin(crd[0], edge_h[1:3]) & np.isin(crd[1], edge_w[1:3]) & np.isin(crd[2], chans[1:3])
    crd = np.concatenate([crd, crd[:, base_in][:, :4], crd[:, :4]], axis=1)      # repeated coordinates, inside and outside
    data = (np.arange(crd.shape[1]) % 3 + 1).astype(np.uint16)
    gene = (data, crd, (H, W, ZT * 500))
    img = synth.image_tile("td/b", (2 * ZT, H, W), 0)
    ts = TrainTileSet.from_arrays([img], [gene], geo, DEV)
    params = [(0, top, left, snm, r, f) for r in range(4) for f in (0, 1)]
    got = gather_nan(ts, params).rna.cpu()
    inside = np.isin(crd[0], edge_h[1:3]) & np.isin(crd[1], edge_w[1:3]) & np.isin(crd[2], chans[1:3])
    assert inside.sum() == 8 + 4                                   # 2 x 2 x 2 border entries + the repeats among them
    for b, p in enumerate(params):
        assert torch.equal(got[b], ref_genes(gene, geo, *p[1:])), p
        assert float(got[b].sum()) == float(data[inside].sum())
        assert float(got[b][:2].sum() + got[b][-2:].sum() + got[b][:, :2].sum() + got[b][:, -2:].sum()) == 0.0     # the pdim frame


def test_genes_empty_tile_big_tile_and_repeated_draws():
    geo = TrainGeometry(sdim=SDIM, gblk=16, pdim=2, snum=4)
    Hb = 512
    big = synth.train_gene_tile("td/big", Hb, Hb, ZT, 1_200_000, 1)
    empty = (np.zeros(0, np.uint16), np.zeros((3, 0), np.int64), (Hb, Hb, ZT * 500))
    imgs = [synth.image_tile(f"td/bigimg{i}", (2 * ZT, Hb, Hb), 0) for i in range(2)]
    ts = TrainTileSet.from_arrays(imgs, [empty, big], geo, DEV, seed=5, repeat=40)
    assert ts.nnz >= 1_000_000
    # B = 1
    p1 = [(1, Hb - SDIM, 17, 2, 3, 1)]
    assert torch.equal(gather_nan(ts, p1).rna.cpu()[0], ref_genes(big, geo, *p1[0][1:]))
    # B = 64 from the sampler: both tiles several times each
    params = ts.sampler.params(64, 0)
    assert (params[:, 0] == 0).sum() > 3 and (params[:, 0] == 1).sum() > 3
    bt = gather_nan(ts, params)
    got = bt.rna.cpu()
    for b, p in enumerate(params.tolist()):
        if p[0] == 0:
            assert float(got[b].abs().sum()) == 0.0
        else:
            assert torch.equal(got[b], ref_genes(big, geo, *p[1:])), p
    # two identical calls give identical bits; draw() is gather(sampler.params(...))
    again = gather_nan(ts, params)
    assert torch.equal(again.rna, bt.rna) and torch.equal(again.img, bt.img)
    d = ts.draw(64, 0)
    torch.cuda.synchronize()
    assert np.array_equal(d.params, params) and torch.equal(d.rna, bt.rna) and torch.equal(d.img, bt.img)
    # a set without any entry
    ts0 = TrainTileSet.from_arrays(imgs[:1], [empty], geo, DEV)
    assert float(gather_nan(ts0, [(0, 0, 0, 0, 0, 0)]).rna.abs().sum()) == 0.0


def test_argument_errors():
    geo = TrainGeometry(sdim=SDIM, gblk=16, pdim=2, snum=4)
    ts, _, _ = small_set(geo, nnz=100)
    L = _lib.lib()
    img = torch.zeros((1, 4, SDIM, SDIM), device=DEV)
    rna = torch.zeros((1, 8, 8, 2000), device=DEV)
    st = _lib.current_stream_ptr()

    def images(desc, sdim=SDIM, snum=4, null=False, stain=0):
        host = torch.tensor([desc], dtype=torch.int32)
        dev = host.to(DEV)
        return L.tm_train_batch_images(None if null else _lib.ptr(ts.img), 0, ts.n_tiles, ZT, H, W, _lib.ptr(dev), _lib.ptr(host), 1, sdim,
                                       snum, stain, _lib.ptr(img), st)

    def genes(desc, sdim=SDIM, gblk=16, snum=4, null=False):
        host = torch.tensor([desc], dtype=torch.int32)
        dev = host.to(DEV)
        return L.tm_train_batch_genes(_lib.ptr(ts.crd), _lib.ptr(ts.dat), ts.nnz, None if null else _lib.ptr(ts.tile_base),
                                      _lib.ptr(ts.row_start), ts.n_tiles, ZT, H, W, _lib.ptr(dev), _lib.ptr(host), 1, sdim, gblk, 2, snum,
                                      _lib.ptr(rna), st)

    ok = (0, 0, 0, 0, 0, 0)
    assert images(ok) == 0 and genes(ok) == 0
    cases = [(lambda: images(ok, null=True), b"null"), (lambda: genes(ok, null=True), b"null"),
             (lambda: genes(ok, sdim=60), b"multiple"), (lambda: genes(ok, gblk=12), b"gblk"),
             (lambda: images((0, H - SDIM + 1, 0, 0, 0, 0)), b"outside"), (lambda: genes((0, 0, W - SDIM + 1, 0, 0, 0)), b"outside"),
             (lambda: images((0, -1, 0, 0, 0, 0)), b"outside"), (lambda: images((2, 0, 0, 0, 0, 0)), b"tile"),
             (lambda: images((0, 0, 0, 0, 4, 0)), b"rot"), (lambda: genes((0, 0, 0, 0, 4, 0)), b"rot"),
             (lambda: images((0, 0, 0, 0, 0, 2)), b"flip"), (lambda: images((0, 0, 0, ZT + 2 - 4 + 1, 0, 0)), b"snm"),
             (lambda: images(ok, snum=5), b"snum"), (lambda: genes(ok, snum=2), b"snum"), (lambda: images(ok, stain=3), b"stain"),
             (lambda: images(ok, sdim=H + 1), b"sdim")]
    for call, word in cases:
        assert call() == -1
        assert word in L.tm_last_error(), (word, L.tm_last_error())
    host = torch.tensor([ok], dtype=torch.int32)
    assert L.tm_train_batch_images(_lib.ptr(ts.img), 0, ts.n_tiles, ZT, H, W, None, _lib.ptr(host), 1, SDIM, 4, 0, _lib.ptr(img), st) == -1
    assert b"descriptors" in L.tm_last_error()
    torch.cuda.synchronize()
