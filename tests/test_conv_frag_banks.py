"""No GPU: the LDS bank rule applied to every fragment read and staging store of the two fp32 z-pair LDS-DMA conv kernels
(conv3d_zpair, conv3d_zpair_ups; conv3d_xquad has tests/test_xquad_host.py), on the byte addresses the library computes with the
kernels' own address functions (tm_conv_frag_addrs, tm_conv_frag.h).

The rule (MI355X LDS): `ds_read_b128` is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
same of lanes 32-63, bank = (a / 4) mod 64; a group takes one LDS cycle plus one for every further distinct address on a busy
bank.  `ds_write_b128` is served in eight groups of 8 consecutive lanes, bank = (a / 4) mod 32.  Equal addresses broadcast.

  * every weight and activation fragment read of every K-loop position of every instantiation costs exactly four cycles (16
    distinct 16-byte slots per group);
  * the staging stores are conflict-free and as many per thread as before;
  * the same model on the previous maps ([row][8 floats] images, restated here) reports the 2-way conflicts they had: eight
    cycles on every weight read, and the halo collisions of the activation reads -- the model sees what it is meant to see."""
import ctypes as C

import pytest

from teramind_amd import _lib

READ_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
READ_GROUPS += [[l + 32 for l in g] for g in READ_GROUPS[:2]]
WRITE_GROUPS = [list(range(8 * g, 8 * g + 8)) for g in range(8)]
ZPAIR, UPS = 0, 1
# (kernel, half, tw): every instantiation the launcher takes
INST = [(k, h, tw) for k in (ZPAIR, UPS) for h, tw in ((1, 4), (0, 8), (1, 8), (0, 16), (1, 16), (0, 32), (1, 32))]


def cycles(addrs, groups, banks):
    """LDS-array cycles of one wave instruction of 16-byte accesses: per group the largest number of distinct addresses that
    share a bank (lanes with address -1 are idle)."""
    total = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            a = addrs[lane]
            if a < 0:
                continue
            assert a % 16 == 0
            per_bank.setdefault((a // 4) % banks, set()).add(a)
        total += max((len(s) for s in per_bank.values()), default=0)
    return total


def addrs_of(kernel, half, tw, what, wave, p, ky, kx, sub):
    out = (C.c_int * 64)()
    rc = _lib.lib().tm_conv_frag_addrs(kernel, half, tw, what, wave, p, ky, kx, sub, out)
    return None if rc else list(out)


# ---- geometry, restated ----
def zp_geo(half, tw, new=False):
    """new: the pitch of the 8-wide tile is 12 and the patches of the 4-wide tile lie 40 rows apart"""
    mv = 64 if half else 128
    tr = min(mv // tw, tw)
    npb = mv // (tr * tw)
    hr, hc = tr + 2, 12 if (new and tw == 8) else tw + 2
    return dict(tr=tr, npb=npb, hr=hr, hc=hc, xv=npb * (40 if (new and tw == 4) else hr * hc))


def fragments(kernel, half):
    """every (what, p, ky, kx, sub) of the K loop"""
    kw = 2 if kernel == UPS else 3
    for p in range(3):
        for ky in range(kw):
            for kx in range(kw):
                for ct in range(1 if half else 2):
                    yield 0, p, ky, kx, ct
                for ph in range(4 if kernel == UPS else 1):
                    yield 1, p, ky, kx, ph


# ---- the previous maps: operand images of [row][8 floats], a lane reads float row * 8 + 4 h ----
def old_addrs(kernel, half, tw, what, wave, p, ky, kx, sub):
    out = []
    for lane in range(64):
        i32, h = lane & 31, lane >> 5
        g = zp_geo(half, tw)
        vt, ct0 = (wave & 1, wave >> 1) if half else (wave, 0)
        if what == 0:
            tap = p * 4 + ky * 2 + kx if kernel == UPS else p * 9 + ky * 3 + kx
            a = tap * 512 + sub * 256 + ct0 * 256 + i32 * 8 + 4 * h
        else:
            v = vt * 32 + i32
            ps, rem = divmod(v, g["tr"] * tw)
            r, c = divmod(rem, tw)
            a = p * g["xv"] * 8 + (ky * g["hc"] + kx) * 8 + ((ps * g["hr"] + r + (sub >> 1)) * g["hc"] + c + (sub & 1)) * 8 + 4 * h
        out.append(a * 4)
    return out


@pytest.mark.parametrize("kernel,half,tw", INST)
def test_fragment_reads_are_conflict_free(kernel, half, tw):
    n = 0
    for wave in range(4):
        for what, p, ky, kx, sub in fragments(kernel, half):
            a = addrs_of(kernel, half, tw, what, wave, p, ky, kx, sub)
            assert a is not None and min(a) >= 0
            cyc = cycles(a, READ_GROUPS, 64)
            assert cyc == 4, (wave, what, p, ky, kx, sub, cyc)
            n += 1
    per_wave = {ZPAIR: 27 * (1 if half else 2) + 27, UPS: 12 * (1 if half else 2) + 48}[kernel]
    assert n == 4 * per_wave


@pytest.mark.parametrize("kernel,half,tw", INST)
def test_fragments_stay_inside_their_areas(kernel, half, tw):
    """weights inside the ring (LDS-DMA destinations below 64 KiB), activations inside the X planes, both 16-byte aligned"""
    g = zp_geo(half, tw, new=True)
    w_end = (2 * 12 * 512 if kernel == UPS else 27 * 512) * 4
    x_end = w_end + 3 * g["xv"] * 8 * 4
    assert w_end <= 65536 and x_end <= 81920                     # two workgroups per CU
    for wave in range(4):
        for what, p, ky, kx, sub in fragments(kernel, half):
            a = addrs_of(kernel, half, tw, what, wave, p, ky, kx, sub)
            lo, hi = (0, w_end) if what == 0 else (w_end, x_end)
            assert all(lo <= v and v + 16 <= hi for v in a), (wave, what, p, ky, kx, sub)


@pytest.mark.parametrize("kernel,half,tw", INST)
def test_staging_stores(kernel, half, tw):
    """conflict-free (eight cycles per full wave instruction, as the interleaved image's stores were), every slot a fragment
    read touches written exactly once per plane, and no more store instructions per thread than before"""
    items_old = (2 * zp_geo(half, tw)["xv"] + 255) // 256
    for p in range(3):
        written = []
        k = 0
        while True:
            per_wave = [addrs_of(kernel, half, tw, 2, wave, p, k, 0, 0) for wave in range(4)]
            if per_wave[0] is None:
                break
            for a in per_wave:
                act = [sum(1 for lane in g if a[lane] >= 0) for g in WRITE_GROUPS]
                assert cycles(a, WRITE_GROUPS, 32) == sum(1 for n in act if n), "a store group meets a bank conflict"
                written += [v for v in a if v >= 0]
            k += 1
        assert k == items_old
        assert len(written) == len(set(written))
        if p == 0:
            first = written
    # the reads of plane 0 fall on written slots (pad columns of the pitch and rows nobody reads excepted: never read)
    ws = set(first)
    for wave in range(4):
        for what, p, ky, kx, sub in fragments(kernel, half):
            if what == 1 and p == 0:
                a = addrs_of(kernel, half, tw, 1, wave, p, ky, kx, sub)
                assert set(a) <= ws, (wave, ky, kx, sub)


def test_previous_maps_show_their_conflicts():
    """[row][8] images: every weight read is 2-way conflicted in all four groups (8 cycles); the halo rows of the z-pair kernels
    collide wherever a group's rows repeat mod 8: 2-way or worse."""
    seen_x = {}
    for kernel, half, tw in INST:
        for wave in range(4):
            for what, p, ky, kx, sub in fragments(kernel, half):
                cyc = cycles(old_addrs(kernel, half, tw, what, wave, p, ky, kx, sub), READ_GROUPS, 64)
                if what == 0:
                    assert cyc == 8, (kernel, half, tw, wave, what, cyc)
                else:
                    seen_x.setdefault((kernel, tw), set()).add(cyc)
    for (kernel, tw), s in seen_x.items():
        assert min(s) >= 8, (kernel, tw, s)                      # 2-way at the least (4-way on the 4- and 8-wide tiles)


@pytest.mark.parametrize("tw", [4, 8, 16])
def test_half_arrays_alone_do_not_suffice(tw):
    """Two k-half arrays with the plain lane -> voxel map and the halo pitch TW + 2 still collide in the z-pair kernels (at
    TW = 16 row 0 columns 12, 13 meet row 1 columns 10, 11): the lane map and the pitches of tm_conv_frag.h are needed."""
    g = zp_geo(1, tw)
    a = []
    for lane in range(64):
        ps, rem = divmod(lane & 31, g["tr"] * tw)
        r, c = divmod(rem, tw)
        a.append((((lane >> 5) * g["xv"]) + (ps * g["hr"] + r) * g["hc"] + c) * 16)
    assert cycles(a, READ_GROUPS, 64) > 4


def test_refusals():
    out = (C.c_int * 64)()
    f = _lib.lib().tm_conv_frag_addrs
    assert f(3, 0, 8, 0, 0, 0, 0, 0, 0, out) == -1               # kernel
    assert f(0, 0, 4, 0, 0, 0, 0, 0, 0, out) == -1               # the 4-wide tile has no 128-voxel form
    assert f(2, 0, 8, 0, 0, 0, 0, 0, 0, out) == -1               # kernel 2 is no kernel any more
    assert f(2, 0, 16, 0, 0, 0, 0, 0, 0, out) == -1
    assert f(0, 1, 8, 0, 0, 0, 0, 0, 1, out) == -1               # the small tile has one cout sub-tile per wave
    assert f(0, 0, 8, 1, 0, 3, 0, 0, 0, out) == -1               # product
    assert f(1, 0, 8, 1, 0, 0, 2, 0, 0, out) == -1               # 2 x 2 window
    assert f(0, 0, 8, 0, 4, 0, 0, 0, 0, out) == -1               # wave
    assert f(0, 0, 8, 0, 0, 0, 0, 0, 0, None) == -1
