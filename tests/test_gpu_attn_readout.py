"""-m gpu: the fused pathway read-out (tm_gene_attn_readout / GeneAttnModel.readout / run_attn_batch(fused=True)) and the
attention sweep around it (attn_maps.AttnSweep, stitch.stitch_attn_dir).

Bounds.  Against the reference's recorded results the fused path gets what the unfused path has in test_gpu_golden.py: 2e-3 on
the float16 tile (one fp16 ulp at |x| <= 4) and atol 1e-7 / rtol 1e-4 on the K x K softmax blocks `sub`.

Fused against unfused in fp32 (_check_vs_unfused).  Both sides compute, per map, q = Wq.tok + bq (64-term fp32 fma chains, the
fused kernel as per-slice chains of 16 terms added afterwards), qn = w * q * rsqrt(mean q^2 + eps), logits l = qn.qn' / 64 and
p = exp(l - max) / sum exp(l - max); they differ only in the order of these sums.  An fp32 chain of n terms has a relative
error of at most n * 2^-24 of sum |a b| (6e-8 * 64 = 3.8e-6); q, the mean of q^2 and the logit dot product are three such
chains in sequence and |l| <= max w^2 = O(1), so the two logit rows differ by delta <= about 1e-5 in absolute terms, and a
softmax whose logits move by delta moves by a factor within exp(+-2 delta): a relative 2e-5, plus the 232-term denominator sum
(1.4e-5 worst case).  That is inside the rtol 1e-4 (atol 1e-7) the project already grants the maps themselves against the
reference, so `sub` is held to exactly that.  An element of `out` is sum_g sub[row, g] * count[g, col] over the K selected
genes, with integer counts that both sides read exactly: its error is at most sum_g |d sub[row, g]| * |count[g, col]|, i.e. the
`sub` bound weighted by the counts (<= the bound times the row's sum |count|); the K-term contraction itself adds at most
K * 2^-24 relative, which rtol 1e-4 absorbs.  The raw-count rows of `out` must be equal.  Outputs are prefilled with NaN and a
second launch must reproduce every bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import config_cases as cc
import util
from teramind_amd import _lib, attn_maps, formats, stitch, synth
from teramind_amd.attn_maps import PATHWAYS, AttnSweep, pathway_readout, run_attn_batch
from teramind_amd.config import PathConfig
from teramind_amd.unet import GeneAttnModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = util.GOLDEN
ATOL, RTOL = 1e-7, 1e-4
GLST8 = [75, 191, 5, 154, 94, 145, 57, 180]
GLST_K4 = [191, 180, 67, 57]              # tools/make_attn_region_golden.py
_M, _RNA = {}, {}


def model(case=None):
    if case not in _M:
        cfg = PathConfig() if case is None else cc.path_config(case)
        _M[case] = GeneAttnModel(cfg, DEV).load_state_dict(util.state_dict(cfg, vis_only=True), strict=False)
    return _M[case]


def _raw_readout(m, rna, glst, want_sub=True):
    """tm_gene_attn_readout into NaN-prefilled buffers, twice; returns (out, sub) of the first launch."""
    B, gn = rna.shape[0], m.conf.gn_sz
    K = len(glst)
    L = _lib.lib()
    nws = L.tm_gene_attn_readout_workspace_bytes(m._h, B, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    gl = (C.c_int * K)(*glst)
    res = []
    for _ in range(2):
        out = torch.full((B, 4 * K, 2 * gn * gn), float("nan"), dtype=torch.float32, device=DEV)
        sub = torch.full((4, B, K, K), float("nan"), dtype=torch.float32, device=DEV) if want_sub else None
        _lib.check(L.tm_gene_attn_readout(m._h, _lib.ptr(rna), B, gl, K, _lib.ptr(out), _lib.ptr(sub), _lib.ptr(ws), nws,
                                          _lib.current_stream_ptr()), "tm_gene_attn_readout")
        res.append((out, sub))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(res[0][0]).any()), "out has unwritten elements"
    assert torch.equal(res[0][0], res[1][0]), "two launches differ in out"
    if want_sub:
        assert not bool(torch.isnan(res[0][1]).any()), "sub has unwritten elements"
        assert torch.equal(res[0][1], res[1][1]), "two launches differ in sub"
    return res[0]


def _check_vs_unfused(m, rna, glst, tag):
    K, B = len(glst), rna.shape[0]
    out, sub = _raw_readout(m, rna, glst)
    attn, mid = m(rna=rna)
    g = list(glst)
    sub_u = attn[:, :, g][..., g]
    out_u = pathway_readout(attn, mid, g)
    del attn
    assert out.shape == out_u.shape and sub.shape == sub_u.shape
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(sub).all())
    ds = (sub - sub_u).abs()
    tol_s = ATOL + RTOL * sub_u.abs()
    print(f"{tag}: sub max|d| {ds.max().item():.3e} (worst ratio to bound {(ds / tol_s).max().item():.3f})")
    assert bool((ds <= tol_s).all()), f"{tag}: sub outside atol {ATOL} / rtol {RTOL}"
    # bound of out: the sub bound weighted by the counts each product row multiplies (see the module docstring)
    cnt = mid[:, g].abs()                                                     # [B, K, 2, gh, gw]
    c0, c1 = cnt[:, :, 0].reshape(B, K, -1), cnt[:, :, 1].reshape(B, K, -1)
    t0 = tol_s[:2].permute(1, 0, 2, 3).reshape(B, 2 * K, K)
    t1 = tol_s[1:3].permute(1, 0, 2, 3).reshape(B, 2 * K, K)
    tol_o = torch.cat([torch.cat([t0 @ c0, t1 @ c1], -1), tol_s[3] @ cnt.reshape(B, K, -1)], 1)
    do = (out - out_u).abs()
    print(f"{tag}: out max|d| {do[:, :3 * K].max().item():.3e}, bound min {tol_o.min().item():.3e} max {tol_o.max().item():.3e}")
    assert bool((do[:, :3 * K] <= tol_o).all()), f"{tag}: out outside the count-weighted sub bound"
    assert torch.equal(out[:, 3 * K:], out_u[:, 3 * K:]), f"{tag}: the raw-count rows differ"
    return out, sub


# ---- 1. against the reference -------------------------------------------------------------------------------
def test_fused_driver_readout_vs_reference():
    gold = torch.from_numpy(np.load(os.path.join(G, "attn_readout.npz"))["out"].astype(np.float32))
    tile = synth.gene_counts("attn/tile", (1, 20, 20, 26000), 0, density=0.05)
    out = run_attn_batch(model(), tile.to(DEV), PATHWAYS["GLUT"], fused=True)
    assert out.dtype == torch.float16 and out.shape == (1, 50, 8, 16, 16)
    d = (out[0].float().cpu() - gold).abs().max().item()
    print(f"fused tile vs reference: max|d| {d:.3e}")
    assert d <= 2e-3


def test_fused_sub_vs_reference():
    gold = np.load(os.path.join(G, "attn_maps.npz"))
    rna = synth.gene_counts("rna_vis", (2, 4, 4, 2000), 1, density=0.05)
    out, sub = model().readout(rna.to(DEV), [75, 191], want_sub=True)
    ref = torch.from_numpy(gold["attn_glst"])
    assert sub.shape == ref.shape and sub.dtype == torch.float32
    print(f"fused sub vs reference: max|d| {(sub.cpu() - ref).abs().max().item():.3e}")
    assert torch.allclose(sub.cpu(), ref, atol=1e-7, rtol=1e-4)


# ---- 2. K = 4, reference-minted -----------------------------------------------------------------------------
def test_fused_driver_readout_k4_vs_reference():
    gold = torch.from_numpy(np.load(os.path.join(G, "attn_readout_k4.npz"))["out"].astype(np.float32))
    tile = synth.gene_counts("attn/tile_k4", (1, 20, 20, 26000), 0, density=0.05)
    out = run_attn_batch(model(), tile.to(DEV), GLST_K4, fused=True)
    assert out.dtype == torch.float16 and out.shape == (1, 50, 16, 16, 16)
    d = (out[0].float().cpu() - gold).abs().max().item()
    print(f"fused K=4 tile vs reference: max|d| {d:.3e}")
    assert d <= 2e-3


# ---- 3. against the unfused path in fp32 --------------------------------------------------------------------
def _dense_rna(B):
    if B not in _RNA:
        rna = synth.gene_counts(f"readout/rna{B}", (B, 4, 4, 2000), 2, density=0.3).to(DEV)
        if B > 1:
            rna[B // 2] = 0                                   # one all-zero patch: uniform softmax, finite output
        _RNA[B] = rna
    return _RNA[B]


@pytest.mark.parametrize("B", [1, 7, 625])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_fused_vs_unfused_fp32(K, B):
    rna = _dense_rna(B)
    glst = GLST8[:K]
    sel = rna.reshape(B, 16, 4, 500)[:, :, :, glst].sum((1, 2))
    live = [n for n in range(B) if not (B > 1 and n == B // 2)]
    assert bool((sel[live] > 0).all()), "a selected gene is all-zero in a live patch: raise the density"
    out, sub = _check_vs_unfused(model(), rna, glst, f"K{K}_B{B}")
    if B > 1:
        z = B // 2
        assert torch.allclose(sub[:, z], torch.full_like(sub[:, z], 1.0 / 229), atol=ATOL, rtol=RTOL)
        assert bool((out[z] == 0).all())


def test_all_zero_single_patch():
    rna = torch.zeros((1, 4, 4, 2000), device=DEV)
    out, sub = _raw_readout(model(), rna, [75, 191])
    assert torch.allclose(sub, torch.full_like(sub, 1.0 / 229), atol=ATOL, rtol=RTOL) and bool((out == 0).all())


# ---- 4. other geometries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(64, 4, "all", 500), (128, 4, "DAPI", 229)], ids=cc.tag_of)
def test_other_geometries_fused_vs_unfused(case):
    m = model(case)
    gn = m.conf.gn_sz
    B = 11                                                    # one full chunk of 8 and a tail of 3
    rna = synth.gene_counts("readout/rna_cfg", (B, gn, gn, 2000), 3, density=0.3).to(DEV)
    glst = [75, 191, 5, 154] if case[3] == 229 else [75, 191, 305, 499]
    out, sub = _check_vs_unfused(m, rna, glst, cc.tag_of(case))
    o2, s2 = m.readout(rna, glst, want_sub=True)
    assert torch.equal(o2, out) and torch.equal(s2, sub)
    assert torch.equal(m.readout(rna, glst), out)
    bound = m._L.tm_gene_attn_readout_workspace_bytes(m._h, 8, 4)
    assert m._L.tm_gene_attn_readout_workspace_bytes(m._h, 625, 4) == bound
    assert m._L.tm_gene_attn_readout_workspace_bytes(m._h, 100000, 4) == bound


# ---- 5. workspace condition and argument errors -------------------------------------------------------------
def test_workspace_does_not_grow_with_the_maps():
    m = model()
    Gn = m.conf.rna_num
    for K in (1, 2, 4, 8):
        assert m._L.tm_gene_attn_readout_workspace_bytes(m._h, 625, K) < 625 * Gn * Gn * 4


def test_argument_errors():
    m = model()
    rna = torch.zeros((2, 4, 4, 2000), device=DEV)
    for bad in ([], list(range(9)), [75, 229], [-1, 75], [75, 191, 75]):
        with pytest.raises(RuntimeError):
            m.readout(rna, bad)
    cfg = cc.path_config((64, 8, "all", 229))
    m8 = GeneAttnModel(cfg, DEV).load_state_dict(util.state_dict(cfg, vis_only=True), strict=False)
    with pytest.raises(RuntimeError):
        m8.readout(torch.zeros((2, 4, 4, 4000), device=DEV), [75, 191])
    # too small a workspace on a geometry that needs one
    mc = model((64, 4, "all", 500))
    gl = (C.c_int * 2)(75, 191)
    out = torch.zeros((2, 8, 32), device=DEV)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    rc = mc._L.tm_gene_attn_readout(mc._h, _lib.ptr(rna), 2, gl, 2, _lib.ptr(out), None, _lib.ptr(ws), 1024,
                                    _lib.current_stream_ptr())
    assert rc != 0
    assert torch.equal(m.readout(rna, [75, 191]), m.readout(rna, (75, 191)))          # the model is still usable


# ---- 6. sweep -----------------------------------------------------------------------------------------------
def _provider():
    from teramind_amd.brain import synthetic_gene_provider
    cache = {}
    base = synthetic_gene_provider(PathConfig(), density=0.05, device=DEV)

    def provider(row, col):
        if (row, col) not in cache:
            cache[(row, col)] = base(row, col)
        return cache[(row, col)]
    return provider


def _dir_bytes(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_attn_sweep_files_ranks_and_stitch(tmp_path):
    cfg, m, genes = PathConfig(), model(), _provider()
    glst, hst, wst, hnm, wnm = PATHWAYS["GLUT"], 512, 768, 2, 3
    d1 = str(tmp_path / "w1")
    res = AttnSweep(cfg, m, genes, glst, hst, wst, hnm, wnm, d1, batch_tiles=4).run()
    assert res["tiles"] == 6 and len(os.listdir(d1)) == 6
    by_hand = np.zeros((50, 8, hnm * 16, wnm * 16), dtype=np.float16)
    for r in range(hnm):
        for c in range(wnm):
            name = f"{hst + r * 256}_{hst + (r + 1) * 256}_{wst + c * 256}_{wst + (c + 1) * 256}.zip"
            a = formats.read_zarr_zip(os.path.join(d1, name))
            assert a.dtype == np.float16 and a.shape == (50, 8, 16, 16)
            ref = run_attn_batch(m, genes(hst // 256 + r, wst // 256 + c)[None], glst, fused=True)[0].cpu().numpy()
            assert np.array_equal(a.view(np.uint16), ref.view(np.uint16)), name
            by_hand[:, :, r * 16:(r + 1) * 16, c * 16:(c + 1) * 16] = ref
    assert res["bytes_written"] == sum(len(v) for v in _dir_bytes(d1).values())
    d2 = str(tmp_path / "w2")
    shares = [AttnSweep(cfg, m, genes, glst, hst, wst, hnm, wnm, d2, rank=k, world=2, batch_tiles=2) for k in range(2)]
    assert sorted(t for s in shares for t in s.tile_list()) == [(r, c) for r in range(hnm) for c in range(wnm)]
    for s in shares:
        s.run()
    assert _dir_bytes(d1) == _dir_bytes(d2)
    mosaic = stitch.stitch_attn_dir(d1, hst, wst, hnm, wnm)
    assert mosaic.dtype == np.float16 and mosaic.shape == (50, 8, 32, 48)
    assert np.array_equal(mosaic.view(np.uint16), by_hand.view(np.uint16))
