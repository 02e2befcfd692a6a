"""No GPU: the bounds of tests/prep_form_cases.py admit an honest float32 evaluation in the kernel's own order on every case of
the GPU test (its own inputs), and reject every deliberately wrong pass of prep_form_cases.WRONG; tm_op_prep_form refuses what
launch_prep must never be handed, before any device call."""
import ctypes as C

import pytest
import torch

import prep_form_cases as pc
from teramind_amd import _lib

ALL = [c for f in pc.CASES.values() for c in f]


def _by_id(cid):
    return next(c for c in ALL if pc.case_id(c) == cid)


def test_case_ids_are_unique_and_cover_the_table():
    ids = [pc.case_id(c) for c in ALL]
    assert len(set(ids)) == len(ids)
    for form, blocks in (("a", (1, 2, 5, 8, 9, 16, 17, 29, 32)), ("b", (1, 2, 5, 8, 9, 16, 17, 29, 32)),
                         ("c", (1, 2, 5, 8, 9, 16, 17, 29, 32)), ("d", (1, 2, 5, 8, 9, 16, 17, 29, 32)),
                         ("h", (1, 2, 5, 8, 9, 16, 17, 29, 32))):
        have = {pc.len_blocks(c["size"]) for c in pc.CASES[form]}
        assert set(blocks) <= have, (form, sorted(have))
    assert {len(c["cins"]) for c in pc.CASES["a"]} == {1, 2, 3}
    assert all(c["N"] * c["Z"] * c["S"] ** 2 <= 144 for c in ALL)
    assert all(len({t for t in (c["src"], c["out"], c["raw"], c["mod_dt"]) if t}) <= 1 for c in ALL), "bf16 and f16 in one case"


@pytest.mark.parametrize("form", list(pc.CASES))
def test_float32_emulation_inside_every_bound(form):
    worst = 0.0
    for c in pc.CASES[form]:
        d = pc.make(c)
        ok, ratio, _ = pc.check(c, pc.reference(c, d), pc.emulate_f32(c, d))
        assert ok, (pc.case_id(c), ratio)
        worst = max(worst, ratio)
    print(f"form {form}: {len(pc.CASES[form])} cases, worst emulation |d| / bound = {worst:.3f}")


# wrong model -> the cases it is shown on (each has what the error needs: a collage, four sub-voxels, pad channels, ...)
WRONG_ON = {
    "pick_odd_row": [c for c in pc.CASES["c"] if c["size"] in ("cb1", "cb9_2", "cb32_2")],
    "collage_out_coords": [c for c in pc.CASES["c"] if any(c["flags"]) and c["size"] in ("cb1p", "cb5_3", "cb17_3", "cb5_2")],
    "swap_ij": [c for f in "ach" for c in pc.CASES[f] if any(c["flags"]) and c["size"] in ("cb1", "cb5_3", "cb9_2", "cb16_2")],
    "one_stat": [c for c in pc.CASES["b"] if c["size"] in ("cb1", "cb1p", "cb5", "cb32")],
    "no_quarter": [c for c in pc.CASES["b"] if c["size"] in ("cb1", "cb9", "cb29")],
    "mean_padded_c": [c for f in "abd" for c in pc.CASES[f] if c["norm"] and c["size"] in ("cb1p", "cb2_2", "cb29")],
    "scale_plain": [c for f in "adh" for c in pc.CASES[f] if c["mod"] and c["size"] in ("cb1", "cb1p", "cb5_3", "cb32_3", "cb32_2")],
    "pad_copied": [c for f in "cdh" for c in pc.CASES[f] if c["pad"] and c["size"] in ("cb1", "cb1p", "cb9", "cb17_3", "cb29")],
}


@pytest.mark.parametrize("wrong", pc.WRONG)
def test_every_wrong_model_lands_outside(wrong):
    cases = WRONG_ON[wrong]
    assert len(cases) >= 3, wrong
    for c in cases:
        d = pc.make(c)
        ok, ratio, _ = pc.check(c, pc.reference(c, d), pc.wrong_model(c, d, wrong))
        assert not ok and ratio > 1.0, (wrong, pc.case_id(c), ratio)


def test_wrong_model_without_an_error_is_the_reference():
    """wrong_model's own arithmetic, with no error switched on, is the reference: what the test above rejects is the error"""
    for cid in ("a-cb1p-image_3-Z2S4N3-rs0-f32>f32", "b-cb5-norm_silu-Z2S4N3-rs2-f32>f32-rawf32"):
        c = _by_id(cid)
        d = pc.make(c)
        vs = [pc._wrong_one(c, d, xc) for xc in d["subs"]]
        ref = pc.cb8(sum(vs) / len(vs), c["cins"], c["pad"])
        assert torch.allclose(ref, pc.reference(c, d)["out"][0], rtol=1e-13, atol=1e-300)


def test_refusals_need_no_device():
    """TM_ERR_ARG with a text before any device call: the pointers are host memory the kernels could not read."""
    L = _lib.lib()
    buf = torch.zeros(8)
    p = _lib.ptr(buf)
    ptrs = (C.c_void_p * 3)(*[buf.data_ptr()] * 3)
    c8 = (C.c_int * 3)(8, 8, 8)
    col0, col1 = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(1, 0, 0)

    def call(nsrc=1, col=col0, N=2, S=4, rs=0, src=0, out=0, mod=0, mod_dt=0, mod_half=0, variant=0, pad=0, raw=None, raw_dt=0):
        return L.tm_op_prep_form(ptrs, c8, col, nsrc, N, 2, S, 3, 2, rs, src, out, p, 8 * nsrc, mod, mod_dt, p if mod else None,
                                 p if mod else None, 8, mod_half, 1, 1, variant, pad, p, raw, raw_dt, 1, None, None)

    for kw, text in [(dict(rs=2, col=col1), b"downsample"), (dict(rs=2, mod=1), b"downsample"), (dict(rs=2, nsrc=2), b"downsample"),
                     (dict(rs=3, S=5), b"pick2"), (dict(rs=1, S=5), b"up2"), (dict(rs=1, col=col1), b"up2"),
                     (dict(src=1, out=2), b"mixed"), (dict(src=1, out=1, mod=2, mod_dt=2), b"mixed"),
                     (dict(out=1, raw=p, raw_dt=2), b"mixed"), (dict(pad=1), b"pad_blocks"), (dict(out=3), b"dtype"),
                     (dict(mod=2, mod_half=1, S=5), b"mod_half"), (dict(mod=1, mod_half=1), b"mod_half"),
                     (dict(mod=1, mod_dt=1), b"per-image"), (dict(rs=4), b"resample"), (dict(variant=4), b"variant"),
                     (dict(variant=2), b"variant 2"), (dict(variant=3), b"variant 3"), (dict(variant=3, src=1, out=1, rs=2), b"variant 3"),
                     (dict(col=col1, N=3), b"collage")]:
        rc = call(**kw)
        assert rc == -1 and text in L.tm_last_error(), (kw, rc, L.tm_last_error())
