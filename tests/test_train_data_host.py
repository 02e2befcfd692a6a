"""CPU: the host half of the training data path (teramind_amd.dataset.TileSampler, the file rules) and the checkpoint
dictionary of teramind_amd.trainer."""
import os

import numpy as np
import torch

from teramind_amd import dataset, trainer
from teramind_amd.config import PathConfig
from teramind_amd.weights import hashed_state_dict, param_spec, strip_lightning_state_dict

GEO = dataset.TrainGeometry(sdim=256, gblk=16, pdim=2, snum=4)


def sampler(n=7, seed=3, accum=2, geo=GEO):
    return dataset.TileSampler(list(range(n)) * 10, 512, 512, geo, seed=seed, gmax=50, accum_batches=accum)


def test_draw_is_a_pure_function_of_its_key():
    a, b = sampler(), sampler()
    p = a.params(8, 5, 1, 0, 2)
    a.params(8, 9, 0, 1, 2)                                        # another draw in between leaves no state behind
    assert np.array_equal(p, b.params(8, 5, 1, 0, 2)) and np.array_equal(p, a.params(8, 5, 1, 0, 2))
    assert p.dtype == np.int32 and p.shape == (8, 6)
    for other in (sampler(seed=4).params(8, 5, 1, 0, 2), a.params(8, 6, 1, 0, 2), a.params(8, 5, 0, 0, 2), a.params(8, 5, 1, 1, 2)):
        assert not np.array_equal(p[:, 1:], other[:, 1:])
    # the epoch enters the key: the same batch slot of two epochs differs
    bpe = a.batches_per_epoch(8, 2)
    assert a.position(8, bpe // 2, 0, 2) == (1, 0) and not np.array_equal(a.params(8, 0, 0, 0, 2), a.params(8, bpe // 2, 0, 0, 2))


def test_ranges_of_the_reference_and_both_ends_occur():
    for snum in (1, 4, 8, 16):
        geo = dataset.TrainGeometry(sdim=256, gblk=16, pdim=2, snum=snum)
        s = dataset.TileSampler(list(range(100)), 300, 280, geo, seed=snum, gmax=50)
        p = np.concatenate([s.params(100, step) for step in range(100)])            # 10 000 draws
        smax = 50 + 2 * {1: 0, 4: 1, 8: 1, 16: 3}[snum] - snum
        for col, lo, hi in ((0, 0, 99), (1, 0, 300 - 256), (2, 0, 280 - 256), (3, 0, smax), (4, 0, 3), (5, 0, 1)):
            assert p[:, col].min() == lo and p[:, col].max() == hi, (snum, col, p[:, col].min(), p[:, col].max())
        assert 0.45 < p[:, 5].mean() < 0.55


def test_epoch_permutation_and_rank_shares():
    s = sampler(n=7)                                                # 70 list entries
    for epoch in (0, 1):
        assert sorted(s.epoch_share(epoch)) == list(range(70))     # every list entry once
    assert not np.array_equal(s.epoch_share(0), s.epoch_share(1))
    for world in (2, 3):
        shares = [s.epoch_share(0, r, world) for r in range(world)]
        flat = np.concatenate(shares)
        assert len(set(flat.tolist())) == len(flat) == (70 // world) * world       # disjoint, complete up to the remainder
        assert all(len(x) == 70 // world for x in shares)
        if 70 % world == 0:
            assert sorted(flat.tolist()) == list(range(70))
    # batches of one epoch are consecutive slices of the share: together they visit it once (drop_last)
    share = s.epoch_share(0, 1, 2)
    s1 = dataset.TileSampler(list(range(70)), 512, 512, GEO, seed=3, accum_batches=1)
    got = np.concatenate([s1.params(8, k, 0, 1, 2)[:, 0] for k in range(s1.batches_per_epoch(8, 2))])
    assert np.array_equal(got, share[:len(got)]) and len(got) == (35 // 8) * 8


def test_file_rules():
    assert dataset.image_path("Data/gene_609882/12_7.npz") == "Data/img_609882/12_7.zip"
    lists = {"609882": ["a", "b"], "609889": ["c"]}
    assert dataset.mouse_file_list("609882", lists, repeat=1) == ["c"]            # MBADataset.py:50-53: the other mouse's list
    assert dataset.mouse_file_list("609889", lists, repeat=2) == ["a", "b", "a", "b"]
    assert dataset.mouse_file_list("638850", lists, repeat=10) == ["a", "b", "c"] * 10
    geo = dataset.TrainGeometry.from_config(PathConfig())
    assert (geo.sdim, geo.gblk, geo.pdim, geo.snum, geo.img_channels) == (256, 16, 2, 4, 4)
    assert dataset.TrainGeometry.from_config(PathConfig(patch_size=128, rna_slc=16)).sdim == 256
    assert dataset.TrainGeometry.from_config(PathConfig(patch_size=32, rna_slc=1, stain="DAPI")).img_channels == 1


def test_row_table():
    rng = np.random.default_rng(0)
    crd = np.stack([rng.integers(-2, 42, 500), rng.integers(0, 40, 500), rng.integers(0, 1000, 500)])
    dat = rng.integers(1, 4, 500).astype(np.uint16)
    c, d, rs = dataset.sort_by_row(dat, crd, 40)
    assert rs.shape == (41,) and rs[0] == 0 and rs[-1] == c.shape[1] == ((crd[0] >= 0) & (crd[0] < 40)).sum()
    assert (np.diff(c[0]) >= 0).all()
    for r in (0, 17, 39):
        assert (c[0, rs[r]:rs[r + 1]] == r).all() and rs[r + 1] - rs[r] == (crd[0] == r).sum()
    dense = np.zeros((40, 40, 1000)); np.add.at(dense, tuple(crd[:, (crd[0] >= 0) & (crd[0] < 40)]), dat[(crd[0] >= 0) & (crd[0] < 40)])
    again = np.zeros_like(dense); np.add.at(again, tuple(c), d)
    assert np.array_equal(dense, again)


def test_checkpoint_round_trip(tmp_path):
    cfg = PathConfig(net_ch=16, rna_num=37)
    sd = hashed_state_dict(cfg, 0)
    m = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    ck = trainer.make_checkpoint(cfg, sd, global_step=7, adam_m=m, adam_v=m, adam_t=7, seed=5, epoch=1, epoch_batch=2,
                                 hparams={"batch_size": 2, "accum_batches": 1, "dropout_p": 0.1, "lr": 2e-5, "grad_clip": 1.0, "loss_type": "mse"})
    p = os.path.join(tmp_path, "last.ckpt")
    torch.save(ck, p)
    back = trainer.load_checkpoint(p)                               # weights_only=True
    assert back["global_step"] == 7 and back["config_name"] == cfg.name and back["seed"] == 5 and back["adam_step"] == 7
    assert all(k.startswith("model.") for k in back["state_dict"])
    stripped = strip_lightning_state_dict(back)
    spec = param_spec(cfg)
    assert list(stripped) == [k for k, _ in spec]
    for k, shape in spec:
        assert tuple(stripped[k].shape) == tuple(shape) and torch.equal(stripped[k], sd[k].float())
        assert torch.equal(back["adam_m"][k], m[k].float())
    assert trainer.config_from_dict(back["config"]) == cfg


def test_header_declares_the_training_entry_points():
    from teramind_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "teramind_hip.h")).read()
    L = _lib.lib()
    for name in ("tm_train_batch_images", "tm_train_batch_genes"):
        assert name + "(" in src and name in _lib.SIGNATURES and hasattr(L, name)
    # argument checks that never touch the device
    assert L.tm_train_batch_images(None, 0, 1, 5, 8, 8, None, None, 1, 8, 4, 0, None, None) == -1
    assert b"null" in L.tm_last_error()
