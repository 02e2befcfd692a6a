"""The flat parameter layout of the training path (train_conv.ParamLayout) and the (1,3,3) -> 3x3x3 filter embedding, on the host:
no GPU, and the module is imported without loading the HIP library."""
import importlib.util

import torch

from teramind_amd import _lib, train_conv
from teramind_amd.train_conv import ParamLayout, embed_133

SHAPES = {"a.weight": (1, 3, 1, 1), "b.weight": (4, 3, 1, 3, 3), "b.bias": (4,), "c.weight": (5, 2, 5, 3, 3)}


def _params():
    g = torch.Generator().manual_seed(11)
    return {k: torch.randn(s, generator=g) for k, s in SHAPES.items()}


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_import_does_not_load_the_library(monkeypatch):
    def loaded():
        raise AssertionError("importing train_conv loaded the HIP library")
    monkeypatch.setattr(_lib, "lib", loaded)
    spec = importlib.util.spec_from_file_location("teramind_amd._train_conv_probe", train_conv.__file__)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                            # the module body, run again with lib() forbidden
    assert mod.ParamLayout({"w": torch.zeros(2, 3)}).n == 6 and tuple(mod.embed_133(torch.zeros(1, 1, 3, 3)).shape) == (1, 1, 3, 3, 3)


def test_split_of_flatten_returns_every_tensor_bit_for_bit():
    d = _params()
    d["b.bias"][1] = -0.0                                   # a sign bit that a value comparison would not see
    lay = ParamLayout(d)
    flat = lay.flatten(d)
    assert flat.shape == (lay.n,) and flat.dtype == torch.float32
    back = lay.split(flat)
    assert list(back) == list(d)
    assert all(_same_bits(back[k], d[k]) for k in d)


def test_offsets_are_contiguous_and_in_insertion_order():
    d = _params()
    lay = ParamLayout(d)
    assert lay.keys == list(SHAPES) and lay.shape == SHAPES
    n = 0
    for k in SHAPES:
        assert lay.off[k] == n, k
        n += d[k].numel()
    assert lay.n == n == 3 + 108 + 4 + 450
    assert ParamLayout(dict(reversed(list(d.items())))).keys == list(reversed(list(SHAPES)))


def test_view_aliases_the_flat_tensor():
    d = _params()
    lay = ParamLayout(d)
    flat = lay.flatten(d)
    v = lay.view(flat, "b.weight")
    assert tuple(v.shape) == SHAPES["b.weight"]
    v[3, 2, 0, 2, 2] = 123.5
    assert flat[lay.off["b.weight"] + 108 - 1] == 123.5
    flat[lay.off["b.bias"]] = -7.25
    assert lay.view(flat, "b.bias")[0] == -7.25 and lay.split(flat)["b.bias"][0] == -7.25


def test_embedding_puts_the_filter_in_the_middle_z_plane():
    w = torch.randn((2, 3, 1, 3, 3), generator=torch.Generator().manual_seed(12))
    wf = embed_133(w[:, :, 0])
    assert tuple(wf.shape) == (2, 3, 3, 3, 3) and wf.dtype == torch.float32 and wf.device == w.device
    assert not wf[:, :, 0].any() and not wf[:, :, 2].any()
    assert _same_bits(wf[:, :, 1], w[:, :, 0])
