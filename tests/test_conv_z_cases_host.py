"""CPU: the case tables of the z-size conv tests (tests/conv_z_cases.py) keep what they promise -- exact integer sums, launches
that really split at 256 CUs, and for each z size the stage structures that Z = 2 never produces."""
import pytest

import conv_z_cases as cz


def test_integer_cases_are_exact_in_fp32():
    """Every partial sum of conv + bias + residual is an integer below 2^24: fp32 holds it exactly in any order, and so does
    torch's reference -- torch.equal is the right criterion."""
    cases = cz.integer_cases()
    assert len(cases) > 60
    for Cin, Z in cases:
        assert cz.worst_abs_sum(Cin) < 2 ** 24, (Cin, Z)
    assert cz.worst_abs_sum(max(c for c, _ in cases)) == 27 * 229 * 3 * 2 + 4 + 100


def test_hgeo_constants():
    """The workgroup geometries the launcher instantiates (HGeo<TN, TW, NWV>): voxels, rows, patches, LDS bytes."""
    want = {(64, 8, 8): (1024, 8, 16), (64, 8, 4): (512, 8, 8), (128, 8, 8): (512, 8, 8), (128, 8, 4): (256, 8, 4),
            (64, 16, 8): (1024, 16, 4), (64, 16, 4): (512, 16, 2), (128, 16, 8): (512, 16, 2), (128, 16, 4): (256, 16, 1),
            (64, 32, 8): (1024, 32, 1), (64, 32, 4): (512, 16, 1), (128, 32, 8): (512, 16, 1), (128, 32, 4): (256, 8, 1)}
    for (TN, TW, wv), (tm, tr, npb) in want.items():
        g = cz.hgeo(TN, TW, wv)
        assert (g["TM"], g["TR"], g["NPB"]) == (tm, tr, npb), (TN, TW, wv, g)
        assert g["LDS_BYTES"] <= 160 * 1024
    assert cz.hgeo(128, 8, 4)["LDS_BYTES"] == 2 * (9 * 128 * 2 + 2 * 512) * 16       # 4 patches x 10 rows x 12 slots -> 512


@pytest.mark.parametrize("case,want", zip(cz.TAIL_SPLIT_CASES, [(260, 256, 8), (272, 256, 28), (264, 256, 16)]))
def test_tail_split_cases_split_at_256_cus(case, want):
    N, Cin, Cout, Z, S = case
    r = cz.tail_split(N, Cout, Z, S, 256)
    assert (r["grid8"], r["full"], r["tail4"]) == want
    assert r["w8"] and r["full"] >= 256 and 0 < r["tail4"] <= r["cap"] and r["split"]
    # the split sits on a patch-group boundary: the 8-wave part is whole units of (n-tiles x planes x tiles)
    assert r["full"] % r["unit"] == 0


def test_tail_split_cases_cover_each_z_and_tile_width():
    assert sorted(c[3] for c in cz.TAIL_SPLIT_CASES) == [1, 4, 8]
    assert sorted(cz.tw_of(c[4]) for c in cz.TAIL_SPLIT_CASES) == [8, 16, 32]
    assert {cz.tn_of(c[2]) for c in cz.TAIL_SPLIT_CASES} == {64, 128}


def test_small_automatic_cases_take_the_4_wave_form():
    assert sorted(c[3] for c in cz.AUTO_SMALL_CASES) == [1, 4, 8]
    for N, Cin, Cout, Z, S in cz.AUTO_SMALL_CASES:
        r = cz.tail_split(N, Cout, Z, S, 256)
        assert not r["w8"] and not r["split"]


@pytest.mark.parametrize("Z", [1, 4, 8])
def test_h16_table_varies_the_stage_structure(Z):
    cases = cz.H16_CASES[Z]
    assert any(cz.cbp_of(c[1]) == 1 for c in cases)                                    # NH = npl
    assert any(cz.cbp_of(c[1]) % 2 == 1 and cz.cbp_of(c[1]) > 1 for c in cases)        # odd Cbp > 1
    assert any(cz.partial_group(c[0], c[2], c[3]) for c in cases)                      # partial last patch group
    assert any(c[2] % 8 for c in cases)                                                # output pad slots
    assert {cz.tn_of(c[2]) for c in cases} == {64, 128}
    assert {c[3] for c in cases} == {8, 16, 32, 64}
    assert any((c[2] + 127) // 128 > 1 for c in cases)                                 # several n-tiles
    assert Z in cz.H16_LOCKSTEP and Z in cz.STREAM_CASES and Z in cz.FUSED_CASES
    assert {c[2] for c in cz.FUSED_CASES[Z]} == {64, 128} and {c[4] for c in cz.FUSED_CASES[Z]} == {1, 2, 4}
    assert any(c[3] == Z for c in cz.RANDOM_CASES)


def test_tables_stay_in_the_sizes_asked_for():
    for Z, cases in cz.H16_CASES.items():
        for N, Cin, Cout, S in cases:
            assert N in (1, 3, 9, 17) and Cin in (8, 16, 24, 13, 229) and Cout in (37, 40, 64, 128, 192, 512)
            assert N * max(Cin, Cout) * Z * S * S * 4 < 20e6
    assert {c[3] for c in cz.F32_CASES} == {1, 3, 4, 8} and {c[4] for c in cz.F32_CASES} == {4, 8, 16, 32, 64}
    assert {c[4] for c in cz.F32_CASES if c[3] == 8} == {4, 8, 16, 32, 64}             # Z = 8 at every S
    assert {c[1] for c in cz.F32_CASES} == {13, 24, 229} and {c[2] for c in cz.F32_CASES} == {37, 40, 64, 192}
    assert {c[3] for c in cz.F32_INPLANE_CASES} == {1, 4, 8}
