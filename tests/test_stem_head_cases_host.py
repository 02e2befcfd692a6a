"""No GPU: the criteria of tests/stem_head_cases.py admit a float32 evaluation in the kernels' own order on the GPU test's inputs
and reject every deliberately wrong stem / head of stem_head_cases.WRONG; tm_op_stem / tm_op_head refuse what the kernels do not
take before any device call."""

import pytest
import torch

import stem_head_cases as sh
from teramind_amd import _lib


def test_cases_cover_the_request():
    ids = [sh.case_id(c) for c in sh.CASES]
    assert len(set(ids)) == len(ids)
    stem = {c[1:7] for c in sh.STEM_INT}
    assert len(stem) == 2 * 3 * 12 * 3
    for geo in sh.GEO:                                  # every geometry meets both head instantiations in every type
        have = {(c[2] in (3, 5, 8), c[6]) for c in sh.HEAD_INT if c[3:6] == geo}
        assert len(have) == 6, (geo, have)
    assert {c[1] for c in sh.HEAD_INT} == {24, 61, 64, 128} and {c[2] for c in sh.HEAD_INT} == {1, 2, 3, 4, 5, 8}


@pytest.mark.parametrize("kern", ["stem", "head"])
def test_float32_emulation_meets_every_criterion(kern):
    """the random cases and a cut of the integer ones (every type, both head forms, C = 61): the chain is 9 Cin or 72 Cb tensor
    FMAs on the CPU"""
    geos = ((2, 6, 3), (3, 4, 1), (1, 6, 1))
    cases = [c for c in sh.CASES if c[0] == kern and (c[7] == "rand" or (c[1] == 2 and c[3:6] in geos) or c[1] in (24, 61))]
    assert len(cases) >= 9
    for c in cases:
        x, w, b = sh.make(c)
        ok, worst, exact = sh.check(c, *sh.reference(c, x, w, b), sh.emulate_f32(c, x, w, b))
        assert ok, (sh.case_id(c), worst)
        print(f"{sh.case_id(c)}: emulation |d| / bound = {worst:.3f}{' exact' if exact else ''}")


@pytest.mark.parametrize("kern,wrong", [(k, w) for k, ws in sh.WRONG.items() for w in ws])
def test_every_wrong_model_lands_outside(kern, wrong):
    need = {"zs_unfold": lambda c: c[1] == 2 and c[3] >= 2, "bias_group0": lambda c: c[2] >= 64, "plane_stride": lambda c: c[3] >= 2 and c[2] >= 2}       # each is invisible where its need fails
    cases = [c for c in sh.CASES if c[0] == kern and need.get(wrong, lambda c: True)(c)]
    cases = cases[::max(1, len(cases) // 12)]
    assert len(cases) >= 6
    for c in cases:
        x, w, b = sh.make(c)
        ref, bound = sh.reference(c, x, w, b)
        bad, _ = sh.reference(c, x, w, b, wrong)
        got = bad.to(sh.TORCH[c[6]]) if kern == "stem" else bad.float()
        ok, worst, _ = sh.check(c, ref, bound, got)
        assert not ok and worst > 1.0, (wrong, sh.case_id(c), worst)


def test_refusals_need_no_device():
    L = _lib.lib()
    buf = torch.zeros(8)
    p = _lib.ptr(buf)
    for args, text in [((p, p, p, p, 1, 2, 48, 2, 4, 0), b"multiple of 32"), ((p, p, p, p, 1, 2, 64, 2, 4, 3), b"dtype"),
                       ((p, p, p, p, 1, 2, 64, 2, 4, -1), b"dtype"), ((p, None, p, p, 1, 2, 64, 2, 4, 0), b"null")]:
        assert L.tm_op_stem(*args, None) == -1 and text in L.tm_last_error(), (args[4:], L.tm_last_error())
    for args, text in [((p, p, p, p, 1, 64, 9, 2, 4, 0), b"at most 8"), ((p, p, p, p, 1, 64, 2, 2, 4, 3), b"dtype"),
                       ((p, p, p, None, 1, 64, 2, 2, 4, 0), b"null"), ((p, p, p, p, 1, 64, 0, 2, 4, 0), b"positive")]:
        assert L.tm_op_head(*args, None) == -1 and text in L.tm_last_error(), (args[4:], L.tm_last_error())
