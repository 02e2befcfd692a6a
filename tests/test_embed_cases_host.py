"""No GPU: the bounds of tests/embed_cases.py admit a float32 evaluation in the kernels' own order on the GPU test's inputs and
reject every deliberately wrong kernel of TE_WRONG / EA_WRONG; tm_op_time_embed / tm_op_emb_all refuse what the kernels do not
take before any device call."""
import pytest
import torch

import embed_cases as ec
from prep_form_cases import F32, check_tensor
from teramind_amd import _lib


def _te_check(ref, bounds, got):
    res = [check_tensor(g.float(), r, b, F32) for g, r, b in zip(got, ref, bounds)]
    return all(r[0] for r in res), max(r[1] for r in res)


def test_cases_cover_the_request():
    assert {tuple(ec.te_make(c)[0].tolist()) for c in ec.TE_CASES} == {(999,), (0, 1, 137)}
    assert sorted(set(ec.T_VALUES)) == [0, 1, 137, 999]
    assert {c[:2] for c in ec.TE_CASES} == {(64, 256), (128, 512), (320, 1024)}
    assert {c[:3] for c in ec.EA_CASES if c[3] == "int"} == {(E, tot, b) for E in (64, 256, 1024) for tot in (1, 5, 130) for b in (1, 3)}


@pytest.mark.parametrize("c", ec.TE_CASES, ids=ec.te_id)
def test_time_embed_emulation_inside_bound(c):
    args = ec.te_make(c)
    ref, bounds = ec.te_reference(c, *args)
    ok, worst = _te_check(ref, bounds, ec.te_emulate_f32(c, *args))
    print(f"{ec.te_id(c)}: emulation |d| / bound = {worst:.3f}")
    assert ok, worst


@pytest.mark.parametrize("wrong", ec.TE_WRONG)
def test_time_embed_wrong_models_land_outside(wrong):
    for c in ec.TE_CASES:
        args = ec.te_make(c)
        ref, bounds = ec.te_reference(c, *args)
        bad, _ = ec.te_reference(c, *args, wrong=wrong)
        ok, worst = _te_check(ref, bounds, bad)
        assert not ok and worst > 1.0, (wrong, ec.te_id(c), worst)


@pytest.mark.parametrize("c", ec.EA_CASES, ids=ec.ea_id)
def test_emb_all_emulation_inside_bound(c):
    args = ec.ea_make(c)
    ref, bound = ec.ea_reference(c, *args)
    ok, worst, exact = check_tensor(ec.ea_emulate_f32(c, *args), ref, bound, F32)
    assert ok and (exact or c[3] != "int"), (ec.ea_id(c), worst)


@pytest.mark.parametrize("wrong", ec.EA_WRONG)
def test_emb_all_wrong_models_land_outside(wrong):
    # each error needs a shape that shows it: more than one image and tot != E; a bias that is not all zero; per > 1
    need = {"row_stride_E": lambda c: c[2] > 1 and c[1] != c[0], "bias_per_lane": lambda c: c[1] >= 5, "lane_major": lambda c: c[0] >= 256}[wrong]
    cases = [c for c in ec.EA_CASES if need(c)]
    assert len(cases) >= 6
    for c in cases:
        args = ec.ea_make(c)
        ref, bound = ec.ea_reference(c, *args)
        bad, _ = ec.ea_reference(c, *args, wrong=wrong)
        ok, worst, _ = check_tensor(bad.float(), ref, bound, F32)
        assert not ok and worst > 1.0, (wrong, ec.ea_id(c), worst)


def test_refusals_need_no_device():
    L = _lib.lib()
    buf = torch.zeros(8)
    p = _lib.ptr(buf)
    for args, text in [((p, p, p, p, 1, 96, 5), b"multiple of 64"), ((p, p, p, p, 1, 1088, 5), b"at most 1024"),
                       ((p, p, p, p, 1, 2048, 5), b"at most 1024"), ((p, p, p, None, 1, 64, 5), b"null"), ((p, p, p, p, 1, 64, 0), b"positive")]:
        assert L.tm_op_emb_all(*args, None) == -1 and text in L.tm_last_error(), (args[4:], L.tm_last_error())
    for args, text in [((p, p, p, p, p, p, p, 1, 63, 256), b"even"), ((p, p, p, p, p, p, p, 0, 64, 256), b"positive"),
                       ((p, p, p, p, p, p, None, 1, 64, 256), b"null"), ((p, p, p, p, p, p, p, 1, 320, 16384), b"LDS")]:
        assert L.tm_op_time_embed(*args, None) == -1 and text in L.tm_last_error(), (args[7:], L.tm_last_error())
