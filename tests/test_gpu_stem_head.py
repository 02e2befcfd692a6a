"""stem_kernel and head_kernel<H16, CO> on their own (tm_op_stem / tm_op_head) against F.conv3d in float64, on the cases of
tests/stem_head_cases.py: integer operands must come back bit for bit in fp32, bf16 and f16; the random cases within
(9 Cin + 1) U mag / (72 Cb + 1) U mag, a 16-bit stem output inside the interval a monotone rounding reaches.  Outputs start as
NaN (every element must be written; the stem's CB8 has no channel pads, Cout % 32 == 0), two launches agree in bits, every
element is compared.  No Z S S N here is a multiple of 256: the last workgroup is partly filled in every case.  The head's
C = 61 input has zero pad channels, as the contract of CB8 says.  Worst ratios go to stem_head.txt in the out_dir fixture."""
import ctypes as C
import os

import pytest
import torch

import stem_head_cases as sh
from prep_form_cases import cb8
from teramind_amd import _lib

DEV = "cuda:0"


def _host(t):
    t = t.contiguous().float()
    return t, C.c_void_p(t.data_ptr())


def _run(c, x, w, b):
    kern, Cin, Cout, Z, S, N, dt, kind = c
    (wk, wp), (bk, bp) = _host(w), _host(b)
    if kern == "stem":
        xd = x.contiguous().to(DEV)                                            # [N][Cin Z][S][S]: '(s z) h w'
        y = torch.full((N, Cout // 8, Z, S, S, 8), float("nan"), dtype=sh.TORCH[dt], device=DEV)
        rc = _lib.lib().tm_op_stem(_lib.ptr(xd), wp, bp, _lib.ptr(y), N, Cin, Cout, Z, S, dt, _lib.current_stream_ptr())
    else:
        xd = cb8(x, (Cin,)).to(sh.TORCH[dt]).to(DEV)
        y = torch.full((N, Cout, Z, S, S), float("nan"), dtype=torch.float32, device=DEV)
        rc = _lib.lib().tm_op_head(_lib.ptr(xd), wp, bp, _lib.ptr(y), N, Cin, Cout, Z, S, dt, _lib.current_stream_ptr())
    assert rc == 0, (sh.case_id(c), _lib.lib().tm_last_error())
    return y.cpu()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


GROUPS = [(k, dt, kind) for k in ("stem", "head") for dt in (sh.F32, sh.BF16, sh.F16) for kind in ("int", "rand")]


@pytest.mark.gpu
@pytest.mark.parametrize("kern,dt,kind", GROUPS, ids=["%s-%s-%s" % (k, "f32 bf16 f16".split()[d], n) for k, d, n in GROUPS])
def test_stem_head(kern, dt, kind, out_dir):
    log = []
    try:
        for c in sh.CASES:
            if (c[0], c[6], c[7]) != (kern, dt, kind):
                continue
            x, w, b = sh.make(c)
            got = _run(c, x, w, b)
            assert torch.equal(_bits(got), _bits(_run(c, x, w, b))), f"{sh.case_id(c)}: two launches differ in bits"
            ok, worst, exact = sh.check(c, *sh.reference(c, x, w, b), got)
            log.append(f"{sh.case_id(c)}: worst |d| / bound = {worst:.3f}{' exact' if exact else ''}")
            print(log[-1])
            assert ok, log[-1]
    finally:
        with open(os.path.join(out_dir, "stem_head.txt"), "a") as f:
            f.write("".join(s + "\n" for s in log))
