"""Case tables of tests/test_gpu_conv_zsizes.py (the 3x3x3 convs at the z sizes of rna_slc 1 / 8 / 16, Z = 1 / 4 / 8, plus
Z = 3) and a Python restatement of the 16-bit launcher's geometry and tail-split rule (launch_conv27_bf16, TM_LAUNCHH in
tera-mind_amd/csrc/tm_conv_bf16.hip), so that the tables can be checked on the host (tests/test_conv_z_cases_host.py)."""

# integer operand ranges (those of the Z = 2 tests): x, w, bias, residual
X_R, W_R, B_R, RES_R = 3, 2, 4, 100


def worst_abs_sum(Cin):
    """Upper bound of |conv + bias + res| on the integer operands: 27 taps * Cin products of |x| <= 3, |w| <= 2."""
    return 27 * Cin * X_R * W_R + B_R + RES_R


def tn_of(Cout):
    return 64 if Cout <= 64 else 128                  # conv_bf16_tn


def tw_of(S):
    return 32 if S >= 32 else S                       # S in {8, 16} -> TW = S


def cbp_of(Cin):
    return ((Cin + 7) // 8 + 1) // 2                  # channel-block pairs of the 16-bit kernels' operand


def hgeo(TN, TW, waves):
    """HGeo<TN, TW, NWV> (not the upsampled-input form): TM voxels, TR rows, NPB patches per workgroup and its LDS bytes."""
    wnw = TN // 64
    tm = (waves // wnw) * 128
    tr = min(tm // TW, TW)
    npb = tm // (tr * TW)
    hcp = 12 if TW == 8 else TW + 2
    xs = npb * (tr + 2) * hcp
    xsp = (xs + 63) // 64 * 64
    buf16 = 9 * TN * 2 + 2 * xsp
    return {"TM": tm, "TR": tr, "NPB": npb, "LDS_BYTES": 2 * buf16 * 16}


def grid_of(N, Cout, Z, S, waves):
    TN, TW = tn_of(Cout), tw_of(S)
    g = hgeo(TN, TW, waves)
    ntile = (Cout + TN - 1) // TN
    tiles = (S // TW) * (S // g["TR"])
    return (N + g["NPB"] - 1) // g["NPB"] * Z * tiles * ntile


def tail_split(N, Cout, Z, S, ncu, tail_pct=80):
    """The automatic form's rule: dict(grid8, w8, unit, full, grid4, tail4, cap, split).  split: `full` 8-wave workgroups
    on the ping-pong kernel, then `tail4` 4-wave workgroups from block id 2 * full."""
    TN, TW = tn_of(Cout), tw_of(S)
    g8, g4 = hgeo(TN, TW, 8), hgeo(TN, TW, 4)
    ntile = (Cout + TN - 1) // TN
    tiles8 = (S // TW) * (S // g8["TR"])
    grid8 = grid_of(N, Cout, Z, S, 8)
    unit = ntile * Z * tiles8
    full = grid8 // ncu * ncu // unit * unit
    grid4 = grid_of(N, Cout, Z, S, 4)
    tail4 = grid4 - 2 * full
    cap = 2 * ncu * tail_pct // 100 if 2 * g4["LDS_BYTES"] <= 160 * 1024 else ncu
    w8 = grid8 >= 256
    return {"grid8": grid8, "w8": w8, "unit": unit, "full": full, "grid4": grid4, "tail4": tail4, "cap": cap,
            "split": bool(w8 and full >= ncu and 0 < tail4 <= cap)}


def partial_group(N, Cout, S):
    """True when the last patch group is partly empty in the 8-wave AND the 4-wave form."""
    TN, TW = tn_of(Cout), tw_of(S)
    return all(N % hgeo(TN, TW, wv)["NPB"] for wv in (4, 8))


# ---- 16-bit 3x3x3 conv, forced workgroup forms: Z -> [(N, Cin, Cout, S)] ----
# Cin 8 / 16 / 13: Cbp = 1 (NH = npl: 1 at Z = 1 -- a main loop of one stage); 24: Cbp = 2; 229: Cbp = 15 (odd: NH odd at
# npl = 1 / 3).  Cout 40: 5 of the 8 cout blocks of TN = 64; 37: 3 pad slots in the last block (must read zero); 192 / 512:
# 2 / 4 n-tiles of 128 (192: the second one half empty).
# S = 8: 16 / 8 (TN 64) or 8 / 4 (TN 128) patches per workgroup, S = 16: 4 / 2 or 2 / 1: N = 1, 3, 9, 17 leave the last
# patch group partly empty.  Every tensor stays below 20 MB.
H16_CASES = {
    1: [(3, 8, 64, 8), (17, 16, 128, 8), (9, 24, 37, 8), (3, 229, 192, 8), (3, 13, 512, 16), (1, 24, 64, 16),
        (1, 16, 128, 32), (1, 13, 40, 64)],
    3: [(3, 8, 64, 8), (9, 24, 128, 8), (3, 229, 37, 8), (3, 16, 192, 16), (1, 24, 64, 32), (1, 13, 128, 64)],
    4: [(3, 16, 64, 8), (17, 8, 128, 8), (9, 24, 37, 8), (1, 229, 512, 8), (3, 13, 192, 16), (1, 24, 64, 16),
        (1, 16, 128, 32), (1, 8, 40, 64)],
    8: [(3, 8, 64, 8), (9, 16, 128, 8), (17, 24, 37, 8), (1, 229, 192, 8), (3, 13, 512, 16), (1, 24, 64, 16),
        (1, 16, 128, 32), (1, 13, 40, 64)],
}
# one case per Z on the lockstep 8-wave kernel (waves = 9)
H16_LOCKSTEP = {1: (3, 229, 192, 8), 3: (9, 24, 128, 8), 4: (3, 13, 192, 16), 8: (17, 24, 37, 8)}

# ---- the model's forms: 16-bit residual in / 16-bit result out: Z -> [(N, Cin, Cout, S)] ----
STREAM_CASES = {
    1: [(5, 24, 64, 8), (3, 229, 192, 8), (1, 16, 128, 32)],
    3: [(3, 24, 128, 16)],
    4: [(5, 24, 64, 8), (3, 40, 192, 16), (1, 24, 128, 64)],
    8: [(9, 13, 40, 8), (2, 16, 128, 16), (1, 24, 64, 32)],
}
# ---- fused norm / modulate / SiLU epilogue: Z -> [(N, Cin, Cout, S, per_image)] ----
FUSED_CASES = {
    1: [(5, 24, 64, 8, 2), (3, 16, 128, 16, 1), (17, 13, 128, 8, 4), (1, 40, 64, 32, 1)],
    3: [(5, 229, 128, 8, 4)],
    4: [(5, 24, 64, 8, 2), (3, 96, 128, 16, 1), (17, 13, 128, 8, 4), (2, 16, 64, 32, 2)],
    8: [(5, 24, 128, 8, 2), (3, 16, 64, 16, 1), (17, 13, 64, 8, 4), (1, 24, 128, 32, 1)],
}

# ---- automatic form (waves = 0) ----
# launches that split at 256 CUs: (N, Cin, Cout, Z, S) -> grid8 / full / tail4 = 260 / 256 / 8, 272 / 256 / 28, 264 / 256 / 16
TAIL_SPLIT_CASES = [(517, 16, 128, 4, 8), (135, 16, 512, 1, 16), (33, 16, 64, 8, 32)]
# small launches (grid8 < 256): the 4-wave form
AUTO_SMALL_CASES = [(3, 24, 128, 1, 8), (3, 24, 128, 4, 8), (3, 24, 128, 8, 8)]

# ---- random operands: (N, Cin, Cout, Z, S) ----
RANDOM_CASES = [(3, 64, 128, 1, 8), (3, 64, 128, 4, 8), (3, 64, 128, 8, 8)]

# ---- fp32, zmode 0 at Z != 2 (the three-plane form, zoff = -1): (N, Cin, Cout, Z, S); S = 4 .. 64, each with some Z ----
F32_CASES = [
    (5, 13, 40, 1, 4), (3, 24, 64, 1, 8), (2, 229, 192, 1, 16), (1, 13, 64, 1, 64),
    (3, 24, 40, 3, 4), (3, 13, 192, 3, 8), (1, 24, 64, 3, 32),
    (5, 229, 40, 4, 4), (3, 13, 64, 4, 8), (2, 24, 192, 4, 16), (1, 13, 40, 4, 64),
    (5, 13, 37, 1, 8), (5, 13, 37, 8, 8),                  # 3 output pad slots
    (3, 24, 64, 8, 4), (2, 229, 40, 8, 8), (1, 13, 192, 8, 16), (1, 24, 64, 8, 32), (1, 13, 40, 8, 64),
]
# ---- fp32 in-plane form (zmode 1): (N, Cin, Cout, Z, S) ----
F32_INPLANE_CASES = [(3, 229, 128, 1, 8), (5, 13, 40, 1, 4), (2, 24, 64, 4, 16), (3, 229, 40, 4, 8), (2, 13, 64, 8, 16),
                     (1, 24, 128, 8, 32)]


def integer_cases():
    """Every (Cin, Z) pair that is compared with torch.equal."""
    out = []
    for tab in (H16_CASES, STREAM_CASES, FUSED_CASES):
        out += [(c[1], Z) for Z, cs in tab.items() for c in cs]
    out += [(c[1], Z) for Z, c in H16_LOCKSTEP.items()]
    out += [(c[1], c[3]) for c in TAIL_SPLIT_CASES + AUTO_SMALL_CASES + F32_CASES + F32_INPLANE_CASES]
    return out
