"""No GPU: the LDS model of conv3d_xquad's pipelined schedule (tm_conv_frag_addrs kernel 5: a ring of two sets of six q-planes,
product n of the running count reads set n & 1 while the planes of product n + 1 are stored into the other), on the byte
addresses the library computes with the kernel's own address functions, all four instantiations and every wave.  The bank rule
is that of tests/test_conv_frag_banks.py, imported: every fragment read of every (p, ky, q) costs four LDS cycles, the staging
stores are conflict-free; per plane set every slot of the six planes is written exactly once; every X fragment of product n
falls on slots of set n & 1 written for that product, and on none of the other set; weight reads stay inside the ring below
64 KiB; planes and exchange area stay inside the kernel's LDS size, which fits the CU and, in the small tiles, twice."""
import ctypes as C

import pytest

from test_conv_frag_banks import READ_GROUPS, WRITE_GROUPS, addrs_of, cycles
from teramind_amd import _lib

PIPE = 5
INST = [(h, tw) for h in (0, 1) for tw in (8, 16)]
RING = 2 * 18 * 256 * 4                               # two product slots of 18 taps x 256 floats


def geo(half, tw):
    nw = 4 if half else 8
    mg, gw = 16 * nw, tw // 4
    tr = min(mg // gw, tw)
    npb = mg // (tr * gw)
    return dict(nw=nw, xp=npb * (tr + 2) * gw, lds=_lib.lib().tm_conv_xquad_lds_bytes(half, tw, 1))


def set_range(g, s):
    lo = RING + s * 6 * g["xp"] * 32
    return lo, lo + 6 * g["xp"] * 32


def stores(g, half, tw, s):
    """{q: the byte addresses written into plane q of set s}, every store group checked against the bank rule"""
    planes = {}
    for q in range(6):
        written = []
        for wave in range(g["nw"]):
            a = addrs_of(PIPE, half, tw, 2, wave, 0, 0, q, s)
            assert a is not None
            act = [sum(1 for lane in grp if a[lane] >= 0) for grp in WRITE_GROUPS]
            assert cycles(a, WRITE_GROUPS, 32) == sum(1 for k in act if k), "a store group meets a bank conflict"
            written += [v for v in a if v >= 0]
        assert len(written) == len(set(written)) == 2 * g["xp"]              # every slot of the plane, once
        base = set_range(g, s)[0] + q * g["xp"] * 32
        assert set(written) == set(range(base, base + g["xp"] * 32, 16))
        planes[q] = set(written)
    return planes


@pytest.mark.parametrize("half,tw", INST)
def test_lds_size(half, tw):
    g = geo(half, tw)
    assert RING <= 65536
    assert g["lds"] >= RING + 12 * g["xp"] * 32                   # ring and both plane sets
    assert g["lds"] >= g["nw"] * 3 * 4096                         # the exchange area behind the K loop
    assert g["lds"] <= 160 * 1024
    if half:
        assert g["lds"] <= 80 * 1024                              # two workgroups of the small tile per CU
    assert g["lds"] < _lib.lib().tm_conv_xquad_lds_bytes(half, tw, 0)
    assert set_range(g, 1)[1] <= g["lds"]


@pytest.mark.parametrize("half,tw", INST)
def test_fragment_reads(half, tw):
    g = geo(half, tw)
    n = 0
    for wave in range(g["nw"]):
        for p in range(3):
            for ky in range(3):
                for q in range(3):
                    a = addrs_of(PIPE, half, tw, 0, wave, p, ky, q, 0)
                    assert a is not None and cycles(a, READ_GROUPS, 64) == 4, (wave, p, ky, q)
                    assert all(0 <= v and v + 16 <= RING // 2 for v in a)             # slot 0; slot 1 lies 18 432 B further
                    for s in (0, 1):
                        a = addrs_of(PIPE, half, tw, 1, wave, p, ky, q, s)
                        assert a is not None and cycles(a, READ_GROUPS, 64) == 4, (wave, p, ky, q, s)
                        lo, hi = set_range(g, s)
                        assert all(lo <= v and v + 16 <= hi for v in a), (wave, p, ky, q, s)
                        n += 1
    assert n == g["nw"] * 27 * 2
    assert addrs_of(PIPE, half, tw, 0, g["nw"], 0, 0, 0, 0) is None          # no such wave


@pytest.mark.parametrize("half,tw", INST)
def test_staging_stores_and_the_ring(half, tw):
    g = geo(half, tw)
    planes = [stores(g, half, tw, s) for s in (0, 1)]
    assert not (set().union(*planes[0].values()) & set().union(*planes[1].values()))
    assert addrs_of(PIPE, half, tw, 2, 0, 0, 1, 0, 0) is None               # one staging item per thread
    # the running product count over three cin blocks (both parities of the block's first product): product n reads set n & 1,
    # which was written for it while product n - 1 read the other set
    for n in range(9):
        p = 2 - n % 3                                                       # pack product: X0, X1, X0 + X1
        s = n & 1
        for wave in range(g["nw"]):
            for ky in range(3):
                for q in range(3):
                    a = set(addrs_of(PIPE, half, tw, 1, wave, p, ky, q, s))
                    assert a <= planes[s][3 * (wave & 1) + q], (n, wave, ky, q)
                    assert not (a & set().union(*planes[s ^ 1].values()))     # never the set being stored meanwhile


def test_refusals():
    out = (C.c_int * 64)()
    f = _lib.lib().tm_conv_frag_addrs
    assert f(PIPE, 0, 32, 0, 0, 0, 0, 0, 0, out) == -1           # the x-quad stops at 16-wide tiles
    assert f(PIPE, 1, 8, 0, 4, 0, 0, 0, 0, out) == -1            # the small tile has four waves
    assert f(PIPE, 0, 8, 1, 0, 0, 0, 0, 2, out) == -1            # two plane sets
    assert f(PIPE, 0, 8, 2, 0, 0, 0, 0, -1, out) == -1
    assert f(PIPE, 0, 8, 0, 0, 0, 0, 0, 1, out) == -1            # a weight fragment has no plane set
    assert f(PIPE, 0, 8, 1, 0, 3, 0, 0, 0, out) == -1            # product
    assert f(PIPE, 0, 8, 1, 0, 0, 0, 3, 0, out) == -1            # a wave has three q
    assert f(PIPE, 0, 8, 2, 0, 0, 0, 6, 0, out) == -1            # six q-planes
    assert f(PIPE, 0, 8, 0, 0, 0, 0, 0, 0, None) == -1
    assert _lib.lib().tm_conv_xquad_lds_bytes(0, 32, 1) == -1
    assert _lib.lib().tm_conv_xquad_lds_bytes(0, 8, 2) == -1
