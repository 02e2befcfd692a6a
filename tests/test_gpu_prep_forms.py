"""The block-input pass through tm_op_prep_form -> launch_prep in the forms the executor launches and no other hook expresses,
each against the float64 model and bound of tests/prep_form_cases.py (forms a, b, c, d, h there):

  * prep_kernel<1, true> at 1 .. 32 channel blocks with one, two and three sources, collaged on a 3 x 2 encoder grid, in the
    five modes of test_gpu_prep_wide; prep_kernel<4, false> (down2) with norm and SiLU; pick2 in prep_kernel and prep_h16_kernel;
    fp32 sources with a 16-bit output, per-image and 16-bit per-voxel modulation, pad_blocks;
  * all-16-bit calls also under variant 1 (prep_kernel), 2 and 3 (the two forms of prep_h16_kernel): each inside the same
    interval, and 2 == 3 in bits, pick2 included;
  * outputs start as NaN: every element, channel pads and pad blocks included, must be written; two launches agree in bits;
    every element is compared.  A gather (no norm, no SiLU) and every raw copy must equal the source bits.

N = 3, Z = 2, S = 4 is 96 voxels, the second 64-voxel workgroup half empty; Z = 1, S = 6 is 36.  The worst |d| / bound of every
case goes to prep_forms.txt in the out_dir fixture.
"""
import ctypes as C
import os

import pytest
import torch

import prep_form_cases as pc
from teramind_amd import _lib

DEV = "cuda:0"


def _dev(t, cins, dt, pad=0):
    return pc.cb8(t, cins, pad).to(pc.TORCH[dt]).to(DEV)


def _run(c, d, variant=0):
    """One tm_op_prep_form call on NaN-filled outputs -> dict(out=, raw=) of CPU CB8 tensors in their own types"""
    cins, N, Z, S = c["cins"], c["N"], c["Z"], c["S"]
    cbs = [(cn + 7) // 8 for cn in cins]
    xc = [_dev(x, (cn,), c["src"]) for x, cn in zip(d["xs"], cins)]
    nw = _dev(torch.cat(d["ws"])[None, :, None, None, None], cins, pc.F32).reshape(-1) if c["norm"] else None
    sc = sh = None
    stride = 0
    if c["mod"] == 1:                      # rows over the padded concat channel order, as the executor's emb rows are laid out
        sc, sh = [_dev(t[:, :, None, None, None], cins, pc.F32).reshape(t.shape[0], -1).contiguous() for t in (d["scale"], d["shift"])]
        stride = sc.shape[1]
    elif c["mod"] == 2:
        sc, sh = _dev(d["scale"], cins, c["mod_dt"]), _dev(d["shift"], cins, c["mod_dt"])
        stride = sc[0].numel()
    out = torch.full((N, sum(cbs) + c["pad"], Z, S, S, 8), float("nan"), dtype=pc.TORCH[c["out"]], device=DEV)
    raw = None
    if c["raw"] is not None:
        rp = c["pad"] if c["raw"] != pc.F32 else 0
        raw = torch.full((N, sum(cbs) + rp, Z, S, S, 8), float("nan"), dtype=pc.TORCH[c["raw"]], device=DEV)
    ptrs = (C.c_void_p * len(xc))(*[t.data_ptr() for t in xc])
    cin = (C.c_int * len(xc))(*cins)
    col = (C.c_int * len(xc))(*[int(f) for f in c["flags"]])
    rc = _lib.lib().tm_op_prep_form(ptrs, cin, col, len(xc), N, Z, S, pc.P1, pc.P2, c["rs"], c["src"], c["out"], _lib.ptr(nw),
                                    sum(cins), c["mod"], c["mod_dt"], _lib.ptr(sc), _lib.ptr(sh), stride, c["mod_half"],
                                    c["per_image"], c["act"], variant, c["pad"], _lib.ptr(out), _lib.ptr(raw), c["raw"] or 0,
                                    1, None, _lib.current_stream_ptr())
    assert rc == 0, (pc.case_id(c), variant, _lib.lib().tm_last_error())
    return dict(out=out.cpu(), raw=None if raw is None else raw.cpu())


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return all(a[k] is None or torch.equal(_bits(a[k]), _bits(b[k])) for k in ("out", "raw"))


def _one_case(c, log):
    d = pc.make(c)
    ref = pc.reference(c, d)
    res = _run(c, d)
    assert _same(res, _run(c, d)), f"{pc.case_id(c)}: two launches differ in bits"
    ok, worst, exact = pc.check(c, ref, res)
    line = f"{pc.case_id(c)} variant 0: worst |d| / bound = {worst:.3f}{' exact' if exact else ''}"
    print(line)
    log.append(line)
    assert ok, line
    if c["mode"] == "gather" and c["rs"] != pc.DOWN2:
        assert exact, f"{pc.case_id(c)}: a gather must copy the source bits"
    if c["src"] != pc.F32 and c["out"] != pc.F32:                  # all-16-bit: the generic kernel and both 16-bit forms
        by = {}
        for variant in (1, 2, 3):
            by[variant] = _run(c, d, variant)
            okv, wv, exv = pc.check(c, ref, by[variant])
            line = f"{pc.case_id(c)} variant {variant}: worst |d| / bound = {wv:.3f}{' exact' if exv else ''}"
            print(line)
            log.append(line)
            assert okv, line
        assert _same(by[2], by[3]), f"{pc.case_id(c)}: the one-wave and four-wave forms of prep_h16_kernel differ in bits"
        assert _same(by[2], res), f"{pc.case_id(c)}: the automatic form is neither form of prep_h16_kernel"


GROUPS = [(form, size) for form, cs in pc.CASES.items() for size in dict.fromkeys(c["size"] for c in cs)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,size", GROUPS, ids=[f"{f}-{s}" for f, s in GROUPS])
def test_prep_form(form, size, out_dir):
    log = []
    try:
        for c in pc.CASES[form]:
            if c["size"] == size:
                _one_case(c, log)
    finally:
        with open(os.path.join(out_dir, "prep_forms.txt"), "a") as f:
            f.write("".join(s + "\n" for s in log))
