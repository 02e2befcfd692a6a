"""CPU: the pure host pieces of data-parallel training -- the shard layout of the gradient exchange (train_dist.shard_layout)
and the rank term of the dropout key (train_model.derive_dropout_key)."""
import itertools

import pytest

from teramind_amd.train_dist import shard_layout
from teramind_amd.train_model import derive_dropout_key


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4100])
def test_shard_layout(n, world):
    shard, padded = shard_layout(n, world)
    assert padded >= n and shard % 4 == 0 and padded == world * shard and padded - n < 4 * world
    assert shard >= 4 and (world - 1) * shard < n + 4 * world            # no shard lies wholly beyond what rounding needs


def test_shard_layout_rejects_nonsense():
    for n, world in ((0, 2), (-1, 2), (8, 0)):
        with pytest.raises(ValueError):
            shard_layout(n, world)


def test_dropout_key_rank_zero_is_the_single_device_key():
    for seed, step, micro in itertools.product((0, 7, 123456), (0, 1, 99), (0, 1, 31)):
        assert derive_dropout_key(seed, step, micro, 0) == derive_dropout_key(seed, step, micro)
        assert derive_dropout_key(seed, step, micro, rank=0) == derive_dropout_key(seed, step, micro)


def test_dropout_keys_distinct_over_seed_step_micro_rank():
    grid = list(itertools.product(range(3), repeat=4))
    keys = {derive_dropout_key(*g) for g in grid}
    assert len(keys) == len(grid) == 81
    assert all(0 <= k < 2 ** 64 for k in keys)
