"""No GPU: the LDS bank rule of tests/test_conv_frag_banks.py applied to conv3d_xquad (tm_conv_frag_addrs kernel 4), on the byte
addresses the library computes with the kernel's own address functions: every fragment read of the K loop, every wave, both
tiles and both tile widths costs four LDS cycles; the staging stores are conflict-free; every slot of the eighteen q-planes is
written exactly once and every activation fragment falls on written slots; weights stay inside the ring below 64 KiB (the
LDS-DMA destinations), activations inside the planes, the whole inside the CU's 160 KiB."""
import ctypes as C

import pytest

from test_conv_frag_banks import READ_GROUPS, WRITE_GROUPS, addrs_of, cycles
from teramind_amd import _lib

XQUAD = 4
INST = [(h, tw) for h in (0, 1) for tw in (8, 16)]


def geo(half, tw):
    nw = 4 if half else 8
    mg, gw = 16 * nw, tw // 4
    tr = min(mg // gw, tw)
    npb = mg // (tr * gw)
    return dict(nw=nw, xp=npb * (tr + 2) * gw, w_end=2 * 18 * 256 * 4)


def fragments():
    for p in range(3):
        for ky in range(3):
            for q in range(3):
                yield 0, p, ky, q
                yield 1, p, ky, q


@pytest.mark.parametrize("half,tw", INST)
def test_fragment_reads_are_conflict_free_and_inside_their_areas(half, tw):
    g = geo(half, tw)
    x_end = g["w_end"] + 18 * g["xp"] * 32
    assert g["w_end"] <= 65536 and x_end <= 160 * 1024
    n = 0
    for wave in range(g["nw"]):
        for what, p, ky, q in fragments():
            a = addrs_of(XQUAD, half, tw, what, wave, p, ky, q, 0)
            assert a is not None and min(a) >= 0
            assert cycles(a, READ_GROUPS, 64) == 4, (wave, what, p, ky, q)
            lo, hi = (0, g["w_end"]) if what == 0 else (g["w_end"], x_end)
            assert all(lo <= v and v + 16 <= hi for v in a), (wave, what, p, ky, q)
            n += 1
    assert n == g["nw"] * 2 * 27
    assert addrs_of(XQUAD, half, tw, 0, g["nw"], 0, 0, 0, 0) is None      # no such wave


@pytest.mark.parametrize("half,tw", INST)
def test_staging_stores(half, tw):
    g = geo(half, tw)
    planes = {}
    for p in range(3):
        for q in range(6):
            written = []
            for wave in range(g["nw"]):
                a = addrs_of(XQUAD, half, tw, 2, wave, p, 0, q, 0)
                assert a is not None
                act = [sum(1 for lane in grp if a[lane] >= 0) for grp in WRITE_GROUPS]
                assert cycles(a, WRITE_GROUPS, 32) == sum(1 for k in act if k), "a store group meets a bank conflict"
                written += [v for v in a if v >= 0]
            assert len(written) == len(set(written)) == 2 * g["xp"]          # every slot of the plane, once
            base = g["w_end"] + (p * 6 + q) * g["xp"] * 32
            assert set(written) == set(range(base, base + g["xp"] * 32, 16))
            planes[(p, q)] = set(written)
    assert addrs_of(XQUAD, half, tw, 2, 0, 0, 1, 0, 0) is None              # one staging item per thread
    for wave in range(g["nw"]):
        for what, p, ky, q in fragments():
            if what == 1:
                a = addrs_of(XQUAD, half, tw, 1, wave, p, ky, q, 0)
                assert set(a) <= planes[(p, 3 * (wave & 1) + q)], (wave, p, ky, q)


def test_refusals():
    out = (C.c_int * 64)()
    f = _lib.lib().tm_conv_frag_addrs
    assert f(XQUAD, 0, 32, 0, 0, 0, 0, 0, 0, out) == -1          # the x-quad stops at 16-wide tiles
    assert f(XQUAD, 1, 8, 0, 4, 0, 0, 0, 0, out) == -1           # the small tile has four waves
    assert f(XQUAD, 0, 8, 0, 8, 0, 0, 0, 0, out) == -1
    assert f(XQUAD, 0, 8, 1, 0, 3, 0, 0, 0, out) == -1           # product
    assert f(XQUAD, 0, 8, 1, 0, 0, 0, 3, 0, out) == -1           # a wave has three q
    assert f(XQUAD, 0, 8, 2, 0, 0, 0, 6, 0, out) == -1           # six q-planes
    assert f(XQUAD, 0, 8, 0, 0, 0, 0, 0, 0, None) == -1
