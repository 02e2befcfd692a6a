"""CPU: the bounds tests/test_gpu_window_attn_train_short.py holds the short-window training attention core to
(tests/train_short_cases.py) must accept a plain float32 walk of the operation on every shape and input kind, and must reject
every deliberate error of train_short_cases.WRONG in at least one element of one output."""
import pytest
import torch

import train_short_cases as L

_REF = {}


def _case(shape, kind):
    if (shape, kind) not in _REF:
        N, C, Z, S = shape
        x = L.inputs(N, C, Z, S, kind)
        ref, mag, lmax = L.reference(*x, Z, S)
        _REF[(shape, kind)] = (x, ref, L.bounds(N, C, Z, S, mag, lmax))
    return _REF[(shape, kind)]


def _bites(shape, wrong):
    """'hwz' changes nothing where a window has one plane (Z = 1) or one token per plane (S = 2): the two orders coincide"""
    return wrong != "hwz" or (shape[2] > 1 and shape[3] > 2)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("shape", L.SHORT_CASES)
def test_bound_accepts_the_float32_walk(shape, kind):
    x, ref, bound = _case(shape, kind)
    got = L.emulate_f32(*x, shape[2], shape[3])
    for name in L.OUTPUTS:
        d = (got[name] - ref[name]).abs()
        worst = float((d / bound[name].clamp_min(1e-300)).max())
        assert bool((d <= bound[name]).all()), f"{name}: float32 walk outside the bound, worst |d|/bound = {worst:.3g}"
        assert bool((bound[name] >= 0).all())


@pytest.mark.parametrize("wrong", L.WRONG)
@pytest.mark.parametrize("shape", L.SHORT_CASES)
def test_bound_rejects_every_wrong_variant(shape, wrong):
    """'hwz' reads the QUERY tokens in (h, w, z) order while everything is written back (z, h, w): attention is equivariant
    under one common permutation of a window's tokens, so a wrong order only shows where read and write disagree."""
    if not _bites(shape, wrong):
        x, _, _ = _case(shape, "plain")
        a, b = L.emulate_f32(*x, shape[2], shape[3]), L.emulate_f32(*x, shape[2], shape[3], wrong=wrong)
        assert all(torch.equal(a[n], b[n]) for n in L.OUTPUTS)          # the variant is the operation itself at this shape
        return
    x, ref, bound = _case(shape, "plain")
    bad = L.emulate_f32(*x, shape[2], shape[3], wrong=wrong)
    out = [name for name in L.OUTPUTS if bool(((bad[name] - ref[name]).abs() > bound[name]).any())]
    assert out, f"{wrong}: inside the bound everywhere"


def test_every_wrong_variant_bites_somewhere():
    assert all(any(_bites(s, w) for s in L.SHORT_CASES) for w in L.WRONG)


def test_emulation_matches_the_reference_closely():
    """The float32 walk is the operation: relative L2 against float64 autograd below 1e-4 for every output."""
    for shape in L.SHORT_CASES:
        x, ref, _ = _case(shape, "plain")
        got = L.emulate_f32(*x, shape[2], shape[3])
        for name in L.OUTPUTS:
            assert float((got[name] - ref[name]).norm() / ref[name].norm()) < 1e-4, (shape, name)
