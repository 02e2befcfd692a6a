"""-m gpu: every gene-gene attention kernel on its own (tm_attn.hip: gene_attn_mfma_kernel, gene_attn_generic_kernel,
rna_mid_kernel, gene_readout_kernel, gene_readout_gather_kernel) through the single-operator hooks tm_op_gene_attn, tm_op_rna_mid
and tm_op_gene_readout, against the float64 model of tests/gene_attn_cases.py.

Rules of every case (the house style of test_gpu_window_attn.py):
  * the outputs start as NaN: every real element must be written, and the CB8 pad slots of out_tok (genes G .. 8 ceil(G / 8) - 1)
    must still hold the prefill -- the launchers document "pad slots untouched", the model zeroes them beforehand;
  * the launch is made twice and the two results must agree in bits;
  * the result is compared element by element, |d| <= bound, with the bound gene_attn_cases derives (its docstring holds the
    derivation; tests/test_gene_attn_cases_host.py shows on the CPU what it rejects).  No constant in it comes from an observed error;
  * the worst |d| / bound of the case is printed and appended to gene_attn_bounds.txt in the suite's output directory.

Case -> kernel: form 0 is the model's rule (D = 64, G <= 232, no slot table: the fused MFMA kernels; else the generic kernel
and, for the read-out, the map kernel over chunks of 8 patches plus the gather kernel); forms 1 and 2 force one.  The tables
and what each shape is there for: gene_attn_cases.mfma_cases / generic_cases / readout_cases."""
import ctypes as C
import functools
import os

import pytest
import torch

import gene_attn_cases as GA
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _wptrs(W):
    return (C.c_void_p * 12)(*[w.data_ptr() for w in W])


def _iptr(t):
    return (C.c_int * len(t))(*[int(v) for v in t]) if t is not None else None


@functools.lru_cache(maxsize=2)
def _ref(key):
    """The float64 model of a case's data, shared by the cases that differ only in form / outs."""
    c = GA.Case(key)
    return GA.forward(c, GA.make(c))


def _log(out_dir, line):
    print(line)
    with open(os.path.join(out_dir, "gene_attn_bounds.txt"), "a") as f:
        f.write(line + "\n")


def _compare(name, got, ref, bound, where):
    d = (got - ref).abs()
    ratio = d / bound
    worst = float(ratio.max())
    line = f"{name}  worst |d|/bound = {worst:.3g}  max|d| = {float(d.max()):.3e}  min bound = {float(bound.min()):.3e}"
    if not worst <= 1.0:
        i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        idx = tuple(int(t) for t in torch.unravel_index(torch.tensor(i), ratio.shape))
        line += (f"\n  {int((~(ratio <= 1)).sum())} of {ratio.numel()} elements outside the bound; worst at {where} {idx}: "
                 f"got {float(got[idx])!r} ref {float(ref[idx])!r} bound {float(bound[idx]):.3e}")
    return worst, line


def _run_attn(c, data):
    L = _lib.lib()
    rna = data["rna"].to(DEV)
    wp, gi = _wptrs(data["W"]), _iptr(data["gidx"])
    Gb = (c.G + 7) // 8
    res = []
    for _ in range(2):
        tok = torch.full((c.B, Gb, c.zs, c.gn, c.gn, 8), NAN, device=DEV) if c.outs != "map" else None
        mp = torch.full((c.B, c.G, c.G), NAN, device=DEV) if c.outs != "tok" else None
        _lib.check(L.tm_op_gene_attn(_lib.ptr(rna), wp, gi, c.B, c.gn, c.zs, c.G, c.form, c.zlo, c.zhi, _lib.ptr(tok), _lib.ptr(mp),
                                     _lib.current_stream_ptr()), "tm_op_gene_attn")
        res.append((tok, mp))
    for a, b in zip(*res):
        if a is not None:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches on the same inputs differ in bits"
    tok, mp = res[0]
    return (tok.cpu().double().reshape(c.B, Gb, c.D, 8) if tok is not None else None), (mp.cpu().double() if mp is not None else None)


@pytest.mark.parametrize("c", GA.attn_cases(), ids=lambda c: c.id)
def test_gene_attn(c, out_dir):
    data = GA.make(c)
    ref = _ref(tuple(sorted(dict(c, form=0, outs="both").items())))
    tok, mp = _run_attn(c, data)
    kern = "gene_attn_mfma_kernel" if c.run_form == 1 else "gene_attn_generic_kernel"
    fails = []
    if mp is not None:
        assert not torch.isnan(mp).any(), f"{int(torch.isnan(mp).sum())} attn_map elements not written"
        worst, line = _compare(f"{kern:26s} {c.id:52s} map", mp, ref["map"], ref["dmap"], "(n, query, key)")
        _log(out_dir, line)
        fails += [line] if not worst <= 1.0 else []
    if tok is not None:
        want, bound = GA.to_cb8(ref["tok"]), GA.to_cb8(ref["dtok"])
        real = ~torch.isnan(want)
        assert torch.isnan(tok[~real]).all(), "a CB8 pad slot of out_tok was written"
        assert not torch.isnan(tok[real]).any(), f"{int(torch.isnan(tok[real]).sum())} out_tok elements not written"
        z = torch.zeros(())
        worst, line = _compare(f"{kern:26s} {c.id:52s} tok", torch.where(real, tok, z), torch.where(real, want, z),
                               torch.where(real, bound, z + 1), "(n, gene block, feature, gene % 8)")
        _log(out_dir, line)
        fails += [line] if not worst <= 1.0 else []
    if fails:
        pytest.fail("\n".join(fails))


# ---- rna_mid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,zs,G,B", [(4, 4, 229, 3), (4, 8, 500, 1), (2, 16, 65, 5), (4, 1, 81, 2), (8, 2, 229, 1)])
def test_rna_mid(gn, zs, G, B):
    """rna_h[:, :, 1:-1] must be equal; zs = 1 and 2 have no middle slice: success, nothing written."""
    c = GA.case(gn, zs, G, B)
    rna = GA.make(c)["rna"]
    want = GA.rna_mid(rna, c)
    out = torch.full((max(want.numel(), 64),), NAN, device=DEV)
    _lib.check(_lib.lib().tm_op_rna_mid(_lib.ptr(rna.to(DEV)), B, gn, zs, G, _lib.ptr(out), _lib.current_stream_ptr()), "tm_op_rna_mid")
    out = out.cpu()
    if zs <= 2:
        assert want.numel() == 0 and torch.isnan(out).all()
    else:
        assert torch.equal(out[:want.numel()].reshape(want.shape), want) and torch.isnan(out[want.numel():]).all()


# ---- read-out ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,glst,want_sub", GA.readout_cases(), ids=lambda v: v.id if isinstance(v, GA.Case) else None)
def test_gene_readout(c, glst, want_sub, out_dir):
    L = _lib.lib()
    data = GA.make(c)
    K, gg = len(glst), c.gn * c.gn
    rna = data["rna"].to(DEV)
    wp, gi, gl = _wptrs(data["W"]), _iptr(data["gidx"]), _iptr(glst)
    res = []
    for _ in range(2):
        out = torch.full((c.B, 4 * K, 2 * gg), NAN, device=DEV)
        sub = torch.full((4, c.B, K, K), NAN, device=DEV) if want_sub else None
        _lib.check(L.tm_op_gene_readout(_lib.ptr(rna), wp, gi, c.B, c.gn, c.zs, c.G, gl, K, c.form, _lib.ptr(out), _lib.ptr(sub),
                                        _lib.current_stream_ptr()), "tm_op_gene_readout")
        res.append((out, sub))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)), "two launches differ in out"
    out = res[0][0].cpu().double()
    assert not torch.isnan(out).any(), "out has unwritten elements"
    ref = GA.readout(c, glst, data)
    kern = "gene_readout_kernel" if c.run_form == 1 else "gene_readout_gather_kernel"
    assert torch.equal(out[:, 3 * K:], ref["out"][:, 3 * K:]), "the raw-count rows differ"
    fails = []
    worst, line = _compare(f"{kern:26s} {c.id:40s} K={K} out", out[:, :3 * K], ref["out"][:, :3 * K], ref["dout"][:, :3 * K].clamp_min(1e-300),
                           "(n, row, column)")
    _log(out_dir, line)
    fails += [line] if not worst <= 1.0 else []
    if want_sub:
        assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32)), "two launches differ in sub"
        sub = res[0][1].cpu().double()
        assert not torch.isnan(sub).any(), "sub has unwritten elements"
        worst, line = _compare(f"{kern:26s} {c.id:40s} K={K} sub", sub, ref["sub"], ref["dsub"], "(map, n, row, column)")
        _log(out_dir, line)
        fails += [line] if not worst <= 1.0 else []
    if fails:
        pytest.fail("\n".join(fails))


# ---- refusals: TM_ERR_ARG before any device call ---------------------------------------------------------------------------------
def test_refusals():
    """Every geometry the launchers refuse, and every missing pointer, comes back as TM_ERR_ARG (-1) with a text before any device
    call: the pointers handed over here are host memory and are never dereferenced."""
    L = _lib.lib()
    buf = torch.zeros(16)
    p = _lib.ptr(buf)
    wp = (C.c_void_p * 12)(*[buf.data_ptr()] * 12)
    gl = (C.c_int * 9)(0, 1, 2, 3, 4, 5, 6, 7, 8)
    tab = (C.c_int * 512)(*range(500), *range(12))

    def attn(gn, zs, G, form, word, gidx=None, zlo=0, zhi=None, tok=p, mp=p, rna=p, w=wp, B=1):
        rc = L.tm_op_gene_attn(rna, w, gidx, B, gn, zs, G, form, zlo, zs if zhi is None else zhi, tok, mp, None)
        assert rc == -1 and word.encode() in L.tm_last_error(), (gn, zs, G, form, rc, L.tm_last_error())

    attn(8, 16, 229, 0, "> 512")                  # D = 1024
    attn(8, 16, 229, 2, "> 512")
    attn(4, 4, 513, 0, "G = 513 > 512", gidx=tab)
    attn(4, 4, 233, 1, "> 232")                   # the fused kernel keeps 232 genes in LDS
    attn(4, 8, 229, 1, "!= D = 64")               # gn^2 zs != D of the fused kernel
    attn(2, 4, 229, 1, "!= D = 64")
    attn(4, 4, 81, 1, "slot table", gidx=tab)
    attn(4, 4, 501, 2, "slot table")              # slot g of 500 does not exist
    attn(4, 4, 229, 3, "form")
    attn(4, 4, 229, 0, ">= 1", B=0)
    attn(4, 4, 0, 0, ">= 1")
    attn(4, 4, 229, 0, "slice mask", zlo=3, zhi=2)
    attn(4, 4, 229, 0, "slice mask", zhi=5)
    attn(4, 4, 229, 0, "null", tok=None, mp=None)
    attn(4, 4, 229, 0, "null", rna=None)
    attn(4, 4, 229, 0, "null", w=None)
    attn(4, 4, 229, 0, "w_host[11]", w=(C.c_void_p * 12)(*[buf.data_ptr()] * 11, None))
    bad = (C.c_int * 81)(*range(80), 500)
    attn(4, 1, 81, 0, "gidx[80]", gidx=bad)

    def ro(gn, zs, G, K, form, word, out=p, glst=gl, gidx=None):
        rc = L.tm_op_gene_readout(p, wp, gidx, 1, gn, zs, G, glst, K, form, out, None, None)
        assert rc == -1 and word.encode() in L.tm_last_error(), (gn, zs, G, K, form, rc, L.tm_last_error())

    ro(4, 4, 229, 0, 0, "outside [1, 8]")
    ro(4, 4, 229, 9, 0, "outside [1, 8]")
    ro(4, 8, 229, 2, 0, "rna_slc = 4")
    ro(4, 1, 229, 2, 2, "rna_slc = 4")
    ro(4, 4, 233, 2, 1, "> 232")
    ro(8, 4, 229, 2, 1, "!= D = 64")
    ro(16, 4, 229, 2, 0, "> 512")
    ro(4, 4, 513, 2, 0, "> 512", gidx=tab)
    ro(4, 4, 8, 2, 0, "outside [0, 8)", glst=(C.c_int * 2)(0, 8))
    ro(4, 4, 229, 2, 0, "repeated", glst=(C.c_int * 2)(5, 5))
    ro(4, 4, 229, 2, 0, "null", out=None)
    ro(4, 4, 229, 2, 0, "null", glst=None)
    assert L.tm_op_rna_mid(None, 1, 4, 4, 229, p, None) == -1 and b"null" in L.tm_last_error()
    assert L.tm_op_rna_mid(p, 1, 4, 4, 501, p, None) == -1 and b"<= 500" in L.tm_last_error()
