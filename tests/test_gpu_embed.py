"""time_embed_kernel and emb_all_kernel on their own (tm_op_time_embed / tm_op_emb_all) against the float64 models and the bounds
of tests/embed_cases.py.  Outputs start as NaN, two launches agree in bits, every element is compared; emb_all's integer cases
must come back bit for bit.  The time_embed bound takes logf / expf / sinf / cosf as 2 ulp: an assumption.  The "probe" cases
(one sinusoid per output, identity second Linear) leave little else in the bound, so their printed ratio is the measurement of
it; a ratio above 1 fails here and is a finding about the device functions, not a reason to widen the bound.  Worst ratios go
to embed.txt in the out_dir fixture."""
import os

import pytest
import torch

import embed_cases as ec
from prep_form_cases import F32, check_tensor
from teramind_amd import _lib

DEV = "cuda:0"


def _bits(t):
    return t.view(torch.int32)


def _log(out_dir, line):
    print(line)
    with open(os.path.join(out_dir, "embed.txt"), "a") as f:
        f.write(line + "\n")


def _time_embed(c, t, w1, b1, w2, b2):
    ch, E, b, kind = c
    dev = [x.contiguous().to(DEV) for x in (t, w1, b1, w2, b2)]
    te = torch.full((b, E), float("nan"), device=DEV)
    act = torch.full((b, E), float("nan"), device=DEV)
    rc = _lib.lib().tm_op_time_embed(*[_lib.ptr(x) for x in dev], _lib.ptr(te), _lib.ptr(act), b, ch, E, _lib.current_stream_ptr())
    assert rc == 0, _lib.lib().tm_last_error()
    return te.cpu(), act.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", ec.TE_CASES, ids=ec.te_id)
def test_time_embed(c, out_dir):
    args = ec.te_make(c)
    ref, bounds = ec.te_reference(c, *args)
    got, again = _time_embed(c, *args), _time_embed(c, *args)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), "two launches differ in bits"
    res = [check_tensor(g, r, b, F32) for g, r, b in zip(got, ref, bounds)]
    _log(out_dir, f"{ec.te_id(c)}: worst |d| / bound = te {res[0][1]:.3f}, te_act {res[1][1]:.3f}")
    assert res[0][0] and res[1][0], (ec.te_id(c), res)


@pytest.mark.gpu
@pytest.mark.parametrize("c", ec.EA_CASES, ids=ec.ea_id)
def test_emb_all(c, out_dir):
    E, tot, b, kind = c
    args = ec.ea_make(c)
    ref, bound = ec.ea_reference(c, *args)

    def run():
        dev = [x.contiguous().to(DEV) for x in args]
        ss = torch.full((b, tot), float("nan"), device=DEV)
        rc = _lib.lib().tm_op_emb_all(*[_lib.ptr(x) for x in dev], _lib.ptr(ss), b, E, tot, _lib.current_stream_ptr())
        assert rc == 0, _lib.lib().tm_last_error()
        return ss.cpu()
    got = run()
    assert torch.equal(_bits(got), _bits(run())), "two launches differ in bits"
    ok, worst, exact = check_tensor(got, ref, bound, F32)
    _log(out_dir, f"{ec.ea_id(c)}: worst |d| / bound = {worst:.3f}{' exact' if exact else ''}")
    assert ok and (exact or kind != "int"), (ec.ea_id(c), worst)
