"""No GPU: the rule of the x-quad split (tm_conv_xquad_ksplit) over the ResBlock conv shapes of the model at 128, 32 and 400
patches, the knob TM_CONV_XQUAD_SPLIT=0, and the refusals of tm_op_conv_xquad_split_f32, which come before any device call (on
a machine without a GPU a device call would answer TM_ERR_HIP, not TM_ERR_ARG)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from teramind_amd import _lib

FLOOR = 4                                            # XQUAD_SPLIT_FLOOR (tm_kernels.h): cin blocks a split keeps at least
# (Cin, Cout, S) of the counted 3x3x3 ResBlock convs of the fp32 step at Z = 2 and patch size 64, as the executor lists them
# (TM_PROF_LAYERS): encoder and decoder levels, the decoder concats with the skip tensors and the gene channels
SHAPES = [(ci, co, S) for S, co, cins in ((64, 64, (64, 96, 160, 224)), (64, 128, (128,)), (32, 128, (64, 128, 192, 256, 320, 448)),
                                          (32, 256, (256,)), (16, 256, (128, 256, 384, 512, 640, 896)), (16, 512, (512,)),
                                          (8, 256, (256,)), (8, 512, (485, 512, 741, 997, 1253)))
          for ci in cins]
LAUNCHES = [(N,) + s for N in (128, 32, 400) for s in SHAPES]


def large_wgs(N, Cout, S):
    return (N * 2 * S * S // 1024) * 2 * ((Cout + 63) // 64)


@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda l: "N%d-Cin%d-Cout%d-S%d" % l)
def test_rule(launch):
    N, Cin, Cout, S = launch
    L = _lib.lib()
    k = L.tm_conv_xquad_ksplit(N, Cin, Cout, S, 0)
    assert k in (1, 2, 4)
    if large_wgs(N, Cout, S) >= 256:
        assert k == 1, "a launch that fills the chip with large workgroups is not split"
    if k > 1:
        assert (Cin + 7) // 8 // k >= FLOOR, "a split below the floor"
    assert L.tm_conv_xquad_ksplit(N, Cin, Cout, S, 1) == 1, "res_half is never split"


def test_the_deepest_decoder_level_is_split():
    L = _lib.lib()
    assert L.tm_conv_xquad_ksplit(32, 1253, 512, 8, 0) > 1 and L.tm_conv_xquad_ksplit(32, 512, 512, 8, 0) > 1
    assert L.tm_conv_xquad_ksplit(128, 512, 512, 8, 0) == 1 and L.tm_conv_xquad_ksplit(400, 1253, 512, 8, 0) == 1
    assert L.tm_conv_xquad_ksplit(32, 40, 512, 8, 0) == 1      # five cin blocks: below the floor at any factor


def test_the_factor_does_not_grow_as_the_launch_shrinks():
    """one image of a batch must sum in the batch's order: below the fill threshold the factor is the same at every patch count"""
    L = _lib.lib()
    for Cin in (1253, 997, 512):
        assert {L.tm_conv_xquad_ksplit(N, Cin, 512, 8, 0) for N in range(1, 61)} == {2}


def test_knob_off_is_the_unsplit_rule():
    """TM_CONV_XQUAD_SPLIT=0 is read once per process, so a fresh interpreter"""
    code = ("from teramind_amd import _lib\n"
            "L = _lib.lib()\n"
            "print('k', L.tm_conv_xquad_ksplit(32, 1253, 512, 8, 0), L.tm_conv_xquad_ksplit(32, 512, 512, 8, 0))\n")
    env = dict(os.environ, TM_CONV_XQUAD_SPLIT="0", PYTHONPATH=os.pathsep.join(sys.path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "k 1 1", out.stdout


def test_refusals_need_no_device():
    L = _lib.lib()
    h = torch.zeros(64)
    p = C.c_void_p(h.data_ptr())
    n = C.c_void_p(0)
    f = L.tm_op_conv_xquad_split_f32

    def refused(rc, text):
        assert rc == -1                              # TM_ERR_ARG
        assert text in L.tm_last_error().decode(), L.tm_last_error().decode()

    refused(f(p, p, p, p, n, 0, 1, 40, 37, 2, 8, 0, 0, 3, None), "ksplit must be 0")
    refused(f(p, p, p, p, n, 0, 1, 40, 37, 2, 8, 0, 0, -1, None), "ksplit must be 0")
    refused(f(p, p, p, p, n, 0, 1, 40, 37, 2, 8, 0, 0, 8, None), "ksplit must be 0")
    refused(f(p, p, p, p, n, 0, 1, 8, 37, 2, 8, 0, 0, 2, None), "above the 1 cin blocks")
    refused(f(p, p, p, p, n, 0, 1, 20, 37, 2, 8, 0, 0, 4, None), "above the 3 cin blocks")
    refused(f(p, p, p, p, p, 1, 1, 40, 37, 2, 8, 0, 0, 2, None), "res_half")
    refused(f(p, p, p, p, n, 0, 1, 40, 37, 2, 8, 0, 2, 2, None), "sched must be")
    refused(f(p, p, p, p, n, 0, 1, 40, 37, 2, 4, 0, 0, 2, None), "S must be")
    ms = (C.c_float * 2)()
    g = L.tm_op_conv_pad1_time_split_f32
    refused(g(p, p, p, p, 1, 40, 64, 8, 2, 0, 0, 3, 2, ms, None), "ksplit must be 0")
    refused(g(p, p, p, p, 1, 40, 64, 8, 0, 0, -1, 2, 2, ms, None), "needs form 2")
