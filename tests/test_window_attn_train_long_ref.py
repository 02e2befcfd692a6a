"""CPU: the bounds tests/test_gpu_window_attn_train_long.py holds the long-window training attention core to
(tests/train_long_cases.py) must accept a plain float32 walk of the operation, key-blocked as the kernels walk it, on every
input kind, and must reject every deliberate error of train_long_cases.WRONG in at least one element of one output."""
import pytest
import torch

import train_long_cases as L

# T = 256 at the fixture's width and off the CB8 block with two patches, T = 512: every error shows at each of them
BITE_CASES = [(1, 64, 4, 16), (2, 13, 4, 16), (1, 40, 8, 16)]
_REF = {}


def _case(shape, kind):
    if (shape, kind) not in _REF:
        N, C, Z, S = shape
        x = L.inputs(N, C, Z, S, kind)
        ref, mag, lmax = L.reference(*x, Z, S)
        _REF[(shape, kind)] = (x, ref, L.bounds(N, C, Z, S, mag, lmax))
    return _REF[(shape, kind)]


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("shape", BITE_CASES)
def test_bound_accepts_the_float32_walk(shape, kind):
    x, ref, bound = _case(shape, kind)
    got = L.emulate_f32(*x, shape[2], shape[3])
    for name in L.OUTPUTS:
        d = (got[name] - ref[name]).abs()
        worst = float((d / bound[name].clamp_min(1e-300)).max())
        assert bool((d <= bound[name]).all()), f"{name}: float32 walk outside the bound, worst |d|/bound = {worst:.3g}"
        assert bool((bound[name] >= 0).all())


@pytest.mark.parametrize("wrong", L.WRONG)
@pytest.mark.parametrize("shape", BITE_CASES)
def test_bound_rejects_every_wrong_variant(shape, wrong):
    """'hwz' reads the QUERY tokens in (h, w, z) order while everything is written back (z, h, w): attention is equivariant
    under one common permutation of a window's tokens, so a wrong order only shows where read and write disagree."""
    x, ref, bound = _case(shape, "plain")
    bad = L.emulate_f32(*x, shape[2], shape[3], wrong=wrong)
    out = [name for name in L.OUTPUTS if bool(((bad[name] - ref[name]).abs() > bound[name]).any())]
    assert out, f"{wrong}: inside the bound everywhere"


def test_emulation_matches_the_reference_closely():
    """The float32 walk is the operation: relative L2 against float64 autograd below 1e-4 for every output."""
    shape = BITE_CASES[0]
    x, ref, _ = _case(shape, "plain")
    got = L.emulate_f32(*x, shape[2], shape[3])
    for name in L.OUTPUTS:
        assert float((got[name] - ref[name]).norm() / ref[name].norm()) < 1e-4, name
