"""CPU: the ResBlock dropout keep-mask rule of DESIGN.md §8 as tests/dropout_rng.py states it (the HIP kernels draw by the same
rule, tests/test_gpu_train_dropout.py), and the reference-minted train-mode fixture tests/golden/train_grad_dropout_ref.npz."""
import os

import numpy as np
import pytest

from dropout_rng import drop_scale, keep_mask, keep_words, philox4x32_10, threshold

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in philox4x32_10(ctr, key)) == want


def test_threshold_and_scale():
    assert threshold(0.0) == 0
    assert threshold(0.5) == 1 << 31
    assert threshold(np.float32(0.1)) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))
    assert threshold(0.9999999999) == 2 ** 32 - 1           # float32(p) rounds to 1.0: clamped
    assert drop_scale(0.1) == np.float32(1.0) / np.float32(0.9)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction(p):
    m = keep_mask(0x1234_5678_9ABC_DEF0, 3, p, (4, 64, 1, 128, 128))          # 2^22 elements
    n = m.size
    sd = np.sqrt(n * p * (1 - p))
    assert abs(int(m.sum()) - (1 - p) * n) < 6 * sd


def test_two_sites_are_independent():
    p = 0.1
    a = keep_mask(99, 0, p, (2, 32, 2, 128, 128))                             # 2^21 elements
    b = keep_mask(99, 1, p, (2, 32, 2, 128, 128))
    n = a.size
    q = (1 - p) ** 2 + p ** 2
    assert abs(int((a == b).sum()) - q * n) < 6 * np.sqrt(n * q * (1 - q))
    c = keep_mask(100, 0, p, (2, 32, 2, 128, 128))                           # another key
    assert abs(int((a == c).sum()) - q * n) < 6 * np.sqrt(n * q * (1 - q))


def test_mask_independent_of_enumeration_order():
    """Element (n, c, z, y, x) depends on its coordinates only: drawn one at a time in a shuffled order, or as a slice of a larger
    batch (the first N' images of N), it is the same."""
    key, site, p, shape = 0xDEADBEEF_0000_0001, 17, 0.5, (3, 13, 2, 8, 8)
    m = keep_mask(key, site, p, shape)
    N, C, Z, S, _ = shape
    rng = np.random.default_rng(0)
    idx = np.stack(np.unravel_index(rng.permutation(m.size), shape), axis=1)
    n, c, z, y, x = idx.T
    v = ((n * Z + z) * S + y) * S + x
    words = keep_words(key, site, v.astype(np.uint64), c)
    assert np.array_equal(words >= np.uint32(threshold(p)), m[n, c, z, y, x])
    big = keep_mask(key, site, p, (N + 2,) + shape[1:])
    assert np.array_equal(big[:N], m)
    # C >= 8 channels of one voxel come from two Philox calls (c >> 2): a channel slice is the same mask too
    assert np.array_equal(keep_mask(key, site, p, (N, 5, Z, S, S)), m[:, :5])


def test_fixture_pins_dropout():
    """train_grad_dropout_ref.npz (reference model in .train(), p = 0.1 with the mask of this rule) differs from the eval-mode
    train_grad_ref.npz, for most of the 403 tensors, by far more than the GPU test's bound (2e-3 of the gradient's norm)."""
    d = np.load(os.path.join(GOLDEN, "train_grad_dropout_ref.npz"))
    e = np.load(os.path.join(GOLDEN, "train_grad_ref.npz"))
    assert float(d["p"]) == pytest.approx(0.1) and int(d["sites"]) > 0 and int(d["key"]) > 0
    name = "mse_seed3"
    keys = sorted(k[len(name) + 6:] for k in d.files if k.startswith(f"{name}/norm/"))
    assert len(keys) == 403 and keys == sorted(k[len(name) + 6:] for k in e.files if k.startswith(f"{name}/norm/"))
    assert abs(float(d[f"{name}/loss"]) - float(e[f"{name}/loss"])) > 100 * 2e-5 * abs(float(e[f"{name}/loss"]))
    far = 0
    for k in keys:
        nref = float(d[f"{name}/norm/{k}"])
        if nref == 0.0:
            continue
        dn = abs(float(e[f"{name}/norm/{k}"]) - nref) / nref
        dp = float(np.abs(d[f"{name}/proj/{k}"] - e[f"{name}/proj/{k}"]).max()) / nref
        df = 0.0
        if f"{name}/full/{k}" in d.files:
            df = float(np.linalg.norm(d[f"{name}/full/{k}"].astype(np.float64) - e[f"{name}/full/{k}"]) / nref)
        far += max(dn, dp, df) > 10 * 2e-3
    assert far > 0.5 * len(keys), (far, len(keys))
