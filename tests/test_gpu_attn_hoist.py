"""-m gpu: the step-invariant conditioning side of the AttnBlocks (SiLU(cond), the 7C adaLN tensor, k / v) kept in the RNA
pyramid buffer (tm_rna_pyramid) and read by every step (tm_unet_forward_rna), against tm_unet_forward on the dense genes,
which computes it inside each block.  Same kernels on the same inputs: every comparison is torch.equal.

Hashed weights and synth inputs, as in tests/test_gpu_unet.py.  The references (dense-gene forwards) are computed once per
shape and shared."""
import pytest
import torch

import util
from teramind_amd import synth
from teramind_amd.config import PathConfig
from teramind_amd.unet import BeatGANsUNetModel, RnaPyramid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"square": (1, 2, 2), "nonsquare": (2, 3, 2)}      # (b, p1, p2): Ne = 4, Nd = 1 (the smallest collage); Ne = 12, Nd = 4
STEPS = {"square": ([801], [12]), "nonsquare": ([640, 3], [27, 955])}     # two steps, other t each; two different t per image

_M, _CASE = {}, {}


def model(dtype="f32"):
    if dtype not in _M:
        cfg = PathConfig(compute_dtype=dtype)
        _M[dtype] = BeatGANsUNetModel(cfg, DEV).load_state_dict(util.state_dict(cfg))
    return _M[dtype]


def case(name, dtype="f32"):
    """Inputs of the two steps, the dense-gene references and the pyramid of one shape."""
    key = (name, dtype)
    if key not in _CASE:
        b, p1, p2 = SHAPES[name]
        ne = b * p1 * p2
        m = model(dtype)
        shp = torch.empty((b, 4, 64 * (p1 - 1), 64 * (p2 - 1)), device="meta")
        rna = synth.gene_counts(f"hoist/rna/{name}", (ne, 4, 4, 2000), 21).to(DEV)
        steps = []
        for k, tt in enumerate(STEPS[name]):
            x = synth.normal(f"hoist/x/{name}/{k}", (ne, 4, 64, 64), 21 + k).to(DEV)
            t = torch.tensor(tt, dtype=torch.long, device=DEV)
            ref = m(x=x, t=t, rna=rna, imgs=shp, patch_size=64).pred.clone()
            steps.append((x, t, ref))
        pyr = m.precompute_rna(rna, b, imgs=shp, patch_size=64)
        _CASE[key] = (m, shp, steps, pyr)
    return _CASE[key]


def level_bytes(cfg, ne):
    """The pyramid levels alone (what the buffer held before the AttnBlock tensors joined it): four CB8 stream tensors
    [ne][ceil(w / 8)][Z][S][S][8], S = 2 gn, 4 gn, .., and in fp32 SiLU of the first three; each starts 256-byte aligned."""
    el = 4 if cfg.compute_dtype == "f32" else 2
    sizes = [ne * ((w + 7) // 8) * cfg.z_size * (2 * cfg.gn_sz << i) ** 2 * 8 * el for i, w in enumerate(cfg.rna_widths)]
    if cfg.compute_dtype == "f32":
        sizes += sizes[:3]
    return sum((s + 255) // 256 * 256 for s in sizes)


@pytest.mark.parametrize("name", ["square", "nonsquare"])
def test_two_steps_through_one_pyramid_equal_the_dense_forward(name):
    """One precompute_rna, two forwards with different x and t: the second would show hoisted tensors that live in, or are
    overwritten through, the per-step workspace; the non-square grid shows Ne / Nd, per_image and collage indexing."""
    m, shp, steps, pyr = case(name)
    for x, t, ref in steps:
        got = m(x=x, t=t, rna=pyr, imgs=shp, patch_size=64).pred
        assert torch.equal(got, ref), util.report(name, got, ref)


def test_forward_only_reads_the_pyramid():
    m, shp, steps, pyr = case("nonsquare")
    before = pyr.buf.clone()
    for x, t, _ in steps:
        m(x=x, t=t, rna=pyr, imgs=shp, patch_size=64)
    torch.cuda.synchronize()
    assert torch.equal(pyr.buf, before)


@pytest.mark.parametrize("name", ["square", "nonsquare"])
def test_poisoned_workspace_gives_the_same_result(name):
    """0xFF bytes (NaN patterns) in the whole workspace before each step: nothing a step reads lives there from before."""
    m, shp, steps, pyr = case(name)
    for x, t, ref in steps:
        [w.fill_(0xFF) for w in m._ws.values()]
        got = m(x=x, t=t, rna=pyr, imgs=shp, patch_size=64).pred
        assert torch.equal(got, ref), util.report(name, got, ref)


def test_buffer_of_the_levels_alone_is_rejected():
    """tm_rna_pyramid_bytes covers the AttnBlock tensors, and tm_unet_forward_rna turns a smaller buffer down with an error."""
    m, shp, steps, pyr = case("nonsquare")
    b, p1, p2 = SHAPES["nonsquare"]
    old = level_bytes(m.conf, b * p1 * p2)
    need = m._L.tm_rna_pyramid_bytes(m._h, b, p1, p2)
    print(f"pyramid bytes (b, p1, p2) = {(b, p1, p2)}: levels {old}, buffer {need}")
    assert need == pyr.buf.numel() and need > old
    x, t, ref = steps[0]
    for n in (old, need - 1):
        with pytest.raises(RuntimeError, match="pyramid buffer too small"):
            m(x=x, t=t, rna=RnaPyramid(pyr.buf[:n], b, p1, p2), imgs=shp, patch_size=64)
    torch.cuda.synchronize()
    assert torch.equal(m(x=x, t=t, rna=pyr, imgs=shp, patch_size=64).pred, ref)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_two_steps_16bit(dtype):
    """The 16-bit AttnBlock keeps its 16-bit mod / kv in the pyramid the same way."""
    m, shp, steps, pyr = case("square", dtype)
    for x, t, ref in steps:
        [w.fill_(0xFF) for w in m._ws.values()]
        got = m(x=x, t=t, rna=pyr, imgs=shp, patch_size=64).pred
        assert torch.equal(got, ref), util.report(dtype, got, ref)
    _M.pop(dtype, None)
    _CASE.pop(("square", dtype), None)
