"""No GPU: the x-quad identity of tests/xquad_cases.py (pair form in z, Winograd F(4,3) along x) equals F.conv3d in float64;
on the integer cases every intermediate stays below 2^24, so a float32 evaluation -- the kernel's included, whatever its order
of sums -- is bit-equal to F.conv3d; the derived bound rejects the model with one wrong coefficient in every case; the host
packer divides exactly; and the hook refuses what the kernel does not take before any device call."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import xquad_cases as XQ
from teramind_amd import _lib


@pytest.mark.parametrize("case", XQ.CASES, ids=XQ.case_id)
def test_float64_model_equals_conv3d(case):
    c = XQ.make(case, "float")
    d = (XQ.model(c) - XQ.reference(c)).abs()
    # float64 roundings of the same expression: the bound's own count with 2^-53 in place of 2^-24
    lim = XQ.bound(c) * (2.0 ** -53 / XQ.U)
    print(f"{XQ.case_id(case)}: max|d|={float(d.max()):.3e}")
    assert bool((d <= lim).all())


@pytest.mark.parametrize("case", XQ.CASES, ids=XQ.case_id)
def test_integer_cases_stay_exact_in_float32(case):
    c = XQ.make(case, "int")
    mag = XQ.magnitude(c)
    print(f"{XQ.case_id(case)}: largest intermediate <= {float(mag.max()):.0f} = 2^{float(mag.max().log2()):.2f}")
    assert float(mag.max()) < 2.0 ** 24
    for pu in XQ.filters(c["w"].double()):           # the transformed filters are integers: multiples of 24 divide exactly
        for u in pu:
            assert torch.equal(u, u.round())
    assert torch.equal(XQ.model(c, torch.float32).double(), XQ.reference(c))


@pytest.mark.parametrize("wrong", XQ.WRONG)
@pytest.mark.parametrize("case", XQ.CASES, ids=XQ.case_id)
def test_one_wrong_coefficient_leaves_the_bound(case, wrong):
    c = XQ.make(case, "float")
    d = (XQ.model(c, torch.float64, wrong) - XQ.reference(c)).abs()
    bnd = XQ.bound(c)
    ci = XQ.make(case, "int")
    breaks = not torch.equal(XQ.model(ci, torch.float32, wrong).double(), XQ.reference(ci))
    print(f"{XQ.case_id(case)} {wrong}: worst |d|/bound={XQ.worst(d, bnd):.3g}, breaks integer equality {breaks}")
    assert not bool((d <= bnd).all()) and breaks


def test_form_switched_off_is_refused():
    """TM_CONV_XQUAD=0 is read once per process, so a fresh interpreter: the hook refuses before any device call"""
    code = ("import ctypes as C, torch\n"
            "from teramind_amd import _lib\n"
            "h = torch.zeros(64); p = C.c_void_p(h.data_ptr())\n"
            "rc = _lib.lib().tm_op_conv_xquad_f32(p, p, p, p, C.c_void_p(0), 0, 1, 8, 64, 2, 8, 0, None)\n"
            "print('rc', rc, _lib.lib().tm_last_error().decode())\n")
    env = dict(os.environ, TM_CONV_XQUAD="0", PYTHONPATH=os.pathsep.join(sys.path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("rc -1 ") and "switched off" in out.stdout, out.stdout


def test_hook_refusals_need_no_device():
    L = _lib.lib()
    h = torch.zeros(64)
    p = C.c_void_p(h.data_ptr())
    n = C.c_void_p(0)
    f = L.tm_op_conv_xquad_f32
    assert f(p, p, p, p, n, 0, 1, 8, 64, 4, 8, 0, None) == -1      # Z != 2
    assert f(p, p, p, p, n, 0, 1, 8, 64, 1, 8, 0, None) == -1
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 4, 0, None) == -1      # S = 4
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 10, 0, None) == -1     # S not a multiple of 4
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 12, 0, None) == -1     # S not a tile size
    assert f(p, p, p, p, n, 0, 1, 8, 64, 2, 8, 3, None) == -1      # tile_variant
    assert f(p, p, p, p, n, 1, 1, 8, 64, 2, 8, 0, None) == -1      # res_half without a residual
    assert f(p, p, p, n, n, 0, 1, 8, 64, 2, 8, 0, None) == -1      # no output
    assert f(p, p, p, p, n, 0, 0, 8, 64, 2, 8, 0, None) == -1      # N < 1
    assert L.tm_last_error()
    ms = (C.c_float * 2)()
    assert L.tm_op_conv_pad1_time_sched_f32(p, p, p, p, 1, 8, 64, 8, 3, 0, -1, 2, ms, None) == -1    # no such form
    assert L.tm_op_conv_pad1_time_sched_f32(p, p, p, p, 1, 8, 64, 8, 1, 0, -1, 2, ms, None) == -1    # form 1 is no form any more
