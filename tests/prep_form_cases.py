"""Cases, float64 model and bounds of the block-input pass in the forms the executor launches and the two older hooks cannot
express (tm_op_prep_form -> launch_prep: prep_kernel<1, true>, prep_kernel<4, false>, RS_PICK2 in prep_kernel and
prep_h16_kernel, fp32 sources with a 16-bit output, pad_blocks).  Shared by tests/test_prep_form_cases_host.py (no GPU) and
tests/test_gpu_prep_forms.py.

Every tensor that meets the checker is in the kernel's own layout, CB8 [N][blocks][Z][S][S][8] over the concatenated sources,
each source padded to whole blocks, pad_blocks zero blocks behind them: channel pads and pad blocks are compared like every
other element (reference 0, bound 0).

FORMS
  a  fp32 -> fp32, same / up2, at most 32 channel blocks (prep_kernel<1, true>): the five modes, the float64 model and the bound
     of tests/test_gpu_prep_wide.py (imported, not copied).
  b  fp32 down2 with norm, with and without SiLU (prep_kernel<4, false>): out = 0.25 (((v0 + v1) + v2) + v3), v_s the result of
     (a) at sub-voxel s with its own statistic.  Bound: the mean of the four bounds of (a), plus U for each of the three
     additions on the partial sums (at most 0.25 sum |v_s| after the exact scaling).  raw, the mean of the four inputs, has the
     three additions only.
  c  pick2: out (z, y, x) <- source (z, 2y, 2x) at 2S, after the collage remap in SOURCE coordinates.  Without norm and SiLU the
     pass is a gather: equality in bits.  With SiLU alone: train_op_ref.silu_hw_rel_bound.
  d  fp32 sources -> 16-bit out: reference and bound of (a) (a bare conversion has bound 0), then the 16-bit interval below.
  h  16-bit sources -> 16-bit out (prep_h16_kernel, or prep_kernel under variant 1), same / pick2: the model of (a) on the
     16-bit source values, then the interval.  The bound of (a) is a count of roundings that holds for any order of the sum.

THE 16-BIT INTERVAL (the rule of train_op_ref.window_attn_fwd): rounding is monotone, so a kernel whose fp32 value lies in
[ref - bound, ref + bound] stores a value in [round16(ref - bound), round16(ref + bound)].  A conversion may flush a result below
the smallest normal number of the type: 0 is admitted wherever the fp32 interval reaches under it.

No constant here comes from an observed error.
"""
import torch
import torch.nn.functional as F

import test_gpu_prep_wide as pw
from oracle import teramind_cpu as tc
from train_op_ref import silu_hw_rel_bound

U, FLT_MIN, EPS = pw.U, pw.FLT_MIN, pw.EPS
F32, BF16, F16 = 0, 1, 2                                  # TM_DTYPE_*
TORCH = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
TINY = {BF16: 2.0 ** -126, F16: 2.0 ** -14}
SAME, UP2, DOWN2, PICK2 = 0, 1, 2, 3
P1, P2 = 3, 2                                             # encoder grid of the collage cases: 2 x 1 output patches per image

# mod, act, per_image, mod_half -- the five of test_gpu_prep_wide plus what the other forms need
MODES = dict(pw.MODES)
MODES.update({"norm": (0, 0, 1, 0), "act_only": (0, 1, 1, 0), "gather": (0, 0, 1, 0)})
NO_NORM = ("act_only", "gather")

# channel blocks -> channels per source (one, two and three sources); what each count crosses is in the issue's table:
# 1 three waves own nothing, 5 uneven split, 8 | 9 and 16 | 17 the instantiations of prep_h16_kernel, 29 = 229 channels with 3
# pad channels inside a concat, 32 the last cached size
SIZES = {
    "cb1": (8,), "cb1p": (5,), "cb2": (16,), "cb2_2": (8, 3), "cb5": (40,), "cb5_2": (16, 24), "cb5_3": (8, 16, 13),
    "cb8": (64,), "cb8_3": (8, 16, 40), "cb9": (72,), "cb9_2": (32, 37), "cb16": (128,), "cb16_2": (64, 61), "cb17": (136,),
    "cb17_3": (64, 8, 61), "cb29": (229,), "cb32": (256,), "cb32_2": (229, 24), "cb32_3": (128, 64, 59),
}
ONE_SRC = [k for k, v in SIZES.items() if len(v) == 1]

WRONG = ["pick_odd_row", "collage_out_coords", "swap_ij", "one_stat", "no_quarter", "mean_padded_c", "scale_plain", "pad_copied"]


def case(form, size, mode, flags=None, Z=2, S=4, b=3, rs=SAME, src=F32, out=F32, raw=None, pad=0, mod_dt=F32):
    cins = SIZES[size]
    flags = tuple(flags) if flags else (0,) * len(cins)
    col = any(flags)
    mod, act, per_image, mod_half = MODES[mode]
    N = b * (P1 - 1) * (P2 - 1) if col else b
    if per_image > 1:
        per_image = (P1 - 1) * (P2 - 1) if col else N
    return dict(form=form, size=size, cins=cins, flags=flags, Z=Z, S=S, b=b, N=N, rs=rs, src=src, out=out, raw=raw, pad=pad,
                mode=mode, mod=mod, act=act, per_image=per_image, mod_half=mod_half, mod_dt=mod_dt, norm=mode not in NO_NORM)


def case_id(c):
    t = "f32 bf16 f16".split()
    s = f"{c['form']}-{c['size']}-{c['mode']}-Z{c['Z']}S{c['S']}N{c['N']}-rs{c['rs']}-{t[c['src']]}>{t[c['out']]}"
    if any(c["flags"]):
        s += "-col" + "".join(map(str, c["flags"]))
    if c["raw"] is not None:
        s += "-raw" + t[c["raw"]]
    if c["pad"]:
        s += "-pad%d" % c["pad"]
    if c["mod_dt"]:
        s += "-mod" + t[c["mod_dt"]]
    return s


def _collage_flags(size, k=0):
    n = len(SIZES[size])
    return [(0,), (1,)][k % 2] if n == 1 else ([(0, 1), (1, 0)][k % 2] if n == 2 else [(0, 1, 1), (1, 0, 1)][k % 2])


def _cases_a():
    cs = []
    for i, size in enumerate(SIZES):                      # N = 3, Z = 2, S = 4: 96 voxels, the second workgroup half empty
        for mode in pw.MODES:
            cs.append(case("a", size, mode, raw=F32 if mode == "norm_silu" else None))
        cs.append(case("a", size, "image_3", flags=_collage_flags(size, i), b=2 - i % 2))     # N = 4 | 2 on the 3 x 2 grid
    for size, mode, kw in [("cb5_3", "norm_silu", dict(Z=1, S=6)), ("cb32_2", "image_1", dict(Z=1, S=6)),   # 36 voxels
                           ("cb9_2", "voxel", dict(Z=1, S=6, flags=(1, 0), b=2)),                            # 144 voxels
                           ("cb17_3", "norm_silu", dict(rs=UP2)), ("cb8", "voxel_half", dict(rs=UP2)),
                           ("cb29", "norm_silu", dict(rs=UP2, Z=1, S=6, raw=F32)),
                           ("cb1", "act_only", {}), ("cb29", "act_only", dict(Z=1, S=6)), ("cb2_2", "gather", dict(raw=F32))]:
        cs.append(case("a", size, mode, **kw))
    return cs


def _cases_b():
    cs = []
    for size in ONE_SRC:
        cs.append(case("b", size, "norm_silu", rs=DOWN2, raw=F32))
        cs.append(case("b", size, "norm", rs=DOWN2))
    cs.append(case("b", "cb5", "norm_silu", rs=DOWN2, Z=1, S=6, raw=F32))
    cs.append(case("b", "cb1p", "norm", rs=DOWN2, Z=1, S=6, b=1, raw=F32))
    return cs


def _cases_c():
    cs = []
    for i, size in enumerate(["cb1", "cb1p", "cb2_2", "cb5_3", "cb8", "cb9_2", "cb16_2", "cb17_3", "cb29", "cb32_2"]):
        for dt in (F32, BF16, F16):
            for col in (0, 1):
                kw = dict(rs=PICK2, src=dt, out=dt, flags=_collage_flags(size, i) if col else None, b=2 if col else 3)
                if dt != F32:
                    kw["pad"] = len_blocks(size) % 2
                cs.append(case("c", size, "act_only", **kw))
                cs.append(case("c", size, "gather", raw=dt if (i + col) % 2 else None, **kw))
    cs.append(case("c", "cb5_2", "act_only", rs=PICK2, Z=1, S=6, flags=(1, 1), b=1))
    cs.append(case("c", "cb5_2", "gather", rs=PICK2, Z=1, S=6, src=BF16, out=BF16, flags=(0, 1), b=2, pad=1, raw=BF16))
    return cs


def len_blocks(size):
    return sum((c + 7) // 8 for c in SIZES[size])


def _cases_d():
    cs = []
    for i, size in enumerate(["cb1p", "cb2_2", "cb5", "cb8_3", "cb9", "cb16_2", "cb17", "cb29", "cb32_3"]):
        dt = (BF16, F16)[i % 2]
        for pad in (0, 1):
            cs.append(case("d", size, "norm_silu", out=dt, pad=pad))
            other = (F16, BF16)[i % 2]
            cs.append(case("d", size, "gather", out=other, pad=pad, raw=other if pad else None))    # level 0 entering the stream
            cs.append(case("d", size, "image_3", out=dt, pad=pad))
            cs.append(case("d", size, "voxel", out=dt, pad=pad, mod_dt=dt))
        cs.append(case("d", size, "act_only", out=dt, pad=1))
        cs.append(case("d", size, "voxel_half", out=dt, pad=0, mod_dt=dt, Z=1, S=6))
    return cs


def _cases_h():
    cs = []
    for i, size in enumerate(["cb1", "cb2_2", "cb5_3", "cb8", "cb9_2", "cb16_2", "cb17_3", "cb29", "cb32_2"]):
        for dt in (BF16, F16):
            pad = len_blocks(size) % 2
            cs.append(case("h", size, "norm_silu", src=dt, out=dt, pad=pad))
            cs.append(case("h", size, "voxel", src=dt, out=dt, pad=pad, mod_dt=dt, flags=_collage_flags(size, i), b=2 - i % 2))
        cs.append(case("h", size, "voxel_half", src=(BF16, F16)[i % 2], out=(BF16, F16)[i % 2], pad=len_blocks(size) % 2,
                       mod_dt=(BF16, F16)[i % 2], Z=1, S=6))
    return cs


CASES = {"a": _cases_a(), "b": _cases_b(), "c": _cases_c(), "d": _cases_d(), "h": _cases_h()}


# ---- layout ------------------------------------------------------------------------------------------------------------------
def cb8(t, cins, pad_blocks=0):
    """NCDHW over the concat's real channels -> CB8 with every source padded to whole blocks and pad_blocks zero blocks"""
    parts, o = [], 0
    N, _, Z, H, W = t.shape
    for c in cins:
        cb = (c + 7) // 8
        p = F.pad(t[:, o:o + c], (0, 0, 0, 0, 0, 0, 0, cb * 8 - c))
        parts.append(p.reshape(N, cb, 8, Z, H, W).permute(0, 1, 3, 4, 5, 2))
        o += c
    if pad_blocks:
        parts.append(torch.zeros((N, pad_blocks, Z, H, W, 8), dtype=t.dtype))
    return torch.cat(parts, 1).contiguous()


def r16(t, dt):
    return t.to(TORCH[dt]).double()


# ---- inputs and the gather -----------------------------------------------------------------------------------------------------
def src_index(c, collage, sub=0, wrong=None):
    """The source patch, row and column every output (n, y, x) reads, in plain index arithmetic: the deliberately wrong gathers are
    written here; make() holds the right one against oracle.teramind_cpu.collage and slicing."""
    N, S, rs = c["N"], c["S"], c["rs"]
    Ss = S // 2 if rs == UP2 else (S if rs == SAME else 2 * S)
    n = torch.arange(N)[:, None, None].expand(N, S, S)
    y = torch.arange(S)[None, :, None].expand(N, S, S)
    x = torch.arange(S)[None, None, :].expand(N, S, S)
    ys, xs = y, x
    if rs == UP2:
        ys, xs = y >> 1, x >> 1
    elif rs == DOWN2:
        ys, xs = 2 * y + (sub >> 1), 2 * x + (sub & 1)
    elif rs == PICK2:
        ys, xs = 2 * y + (1 if wrong == "pick_odd_row" else 0), 2 * x
    ns = n
    if collage:
        q1, q2 = P1 - 1, P2 - 1
        bi, q = n // (q1 * q2), n % (q1 * q2)
        i, j = q // q2, q % q2
        h = (S if wrong == "collage_out_coords" else Ss) // 2
        ys = ys + h
        i, ys = i + (ys >= Ss).long(), ys % Ss
        xs = xs + h
        j, xs = j + (xs >= Ss).long(), xs % Ss
        ns = bi * P1 * P2 + (j * P2 + i if wrong == "swap_ij" else i * P2 + j)
    return ns, ys, xs


def _gather(x, c, collage, sub=0, wrong=None):
    ns, ys, xs = src_index(c, collage, sub, wrong)
    return x[ns, :, :, ys, xs].permute(0, 3, 4, 1, 2).contiguous()            # [N, S, S, C, Z] -> NCDHW


def _gather_plain(x, c, collage, sub):
    """the same gather from the oracle's collage and torch slicing"""
    y = tc.collage(x, c["N"] // ((P1 - 1) * (P2 - 1)), P1, P2) if collage else x
    if c["rs"] == UP2:
        return y.repeat_interleave(2, 3).repeat_interleave(2, 4)
    if c["rs"] == DOWN2:
        return y[:, :, :, (sub >> 1)::2, (sub & 1)::2]
    return y[:, :, :, ::2, ::2] if c["rs"] == PICK2 else y


def make(c, seed=11):
    """The inputs of a case on the CPU, fp32 holding values of the tensor's type: sources NCDHW, norm weights per source, scale /
    shift, and the gathered concat per sub-voxel (one, or the four of down2)."""
    g = torch.Generator().manual_seed(seed)
    N, Z, S, rs = c["N"], c["Z"], c["S"], c["rs"]
    Ne = N // ((P1 - 1) * (P2 - 1)) * P1 * P2
    Ss = S // 2 if rs == UP2 else (S if rs == SAME else 2 * S)
    xs = []
    for cn, f in zip(c["cins"], c["flags"]):
        x = torch.randn((Ne if f else N, cn, Z, Ss, Ss), generator=g) * 1.5
        xs.append(x.to(TORCH[c["src"]]).float())
    ws = [torch.rand((cn,), generator=g) + 0.5 for cn in c["cins"]]
    Ct = sum(c["cins"])
    scale = shift = None
    if c["mod"] == 1:
        nimg = N // c["per_image"]
        scale, shift = torch.randn((nimg, Ct), generator=g) * 0.3, torch.randn((nimg, Ct), generator=g) * 0.3
    elif c["mod"] == 2:
        Sm = S // 2 if c["mod_half"] else S
        scale, shift = torch.randn((N, Ct, Z, Sm, Sm), generator=g) * 0.3, torch.randn((N, Ct, Z, Sm, Sm), generator=g) * 0.3
        scale, shift = scale.to(TORCH[c["mod_dt"]]).float(), shift.to(TORCH[c["mod_dt"]]).float()
    d = dict(xs=xs, ws=ws, scale=scale, shift=shift)
    d["subs"] = gathered(c, d)
    for sub, xc in enumerate(d["subs"]):
        plain = torch.cat([_gather_plain(x, c, f, sub) for x, f in zip(xs, c["flags"])], 1)
        assert torch.equal(xc, plain), "src_index disagrees with the oracle's collage"
    return d


def gathered(c, d, wrong=None):
    nsub = 4 if c["rs"] == DOWN2 else 1
    return [torch.cat([_gather(x, c, f, sub, wrong) for x, f in zip(d["xs"], c["flags"])], 1) for sub in range(nsub)]


# ---- float64 model and bounds ------------------------------------------------------------------------------------------------
def _one(c, d, xc):
    """(reference, bound) of one gathered concat: NCDHW float64"""
    if c["norm"]:
        return pw._reference(xc, d["ws"], d["scale"], d["shift"], c["mod"], c["act"], c["per_image"], c["mod_half"])
    m = xc.double()
    if not c["act"]:
        return m, torch.zeros_like(m)
    ref = F.silu(m)
    return ref, silu_hw_rel_bound(m) * ref.abs() + FLT_MIN


def _wrong_one(c, d, xc, stat=None, cdiv=None, plain_scale=False):
    """the model of (a) with a deliberate error: the statistic of another tensor, another divisor, scale for 1 + scale"""
    xd = xc.double()
    var = (xd if stat is None else stat.double()).pow(2).sum(1, keepdim=True) / (cdiv or xc.shape[1])
    m = torch.cat(d["ws"]).double().view(1, -1, 1, 1, 1) * (xd * torch.rsqrt(var + EPS))
    if c["mod"]:
        sc = pw._full_mod(d["scale"].double(), c["mod"], c["per_image"], c["mod_half"], c["N"])
        sh = pw._full_mod(d["shift"].double(), c["mod"], c["per_image"], c["mod_half"], c["N"])
        m = m * (sc if plain_scale else 1 + sc) + sh
    return F.silu(m) if c["act"] else m


def reference(c, d):
    """dict(out=(ref, bound), raw=(ref, bound) or None), CB8 float64 in the layout of the kernel's tensors"""
    subs = d["subs"]
    lay = lambda t, pad: cb8(t, c["cins"], pad)
    if c["rs"] == DOWN2:
        rb = [_one(c, d, xc) for xc in subs]
        ref = sum(r for r, _ in rb) * 0.25
        bound = sum(b for _, b in rb) * 0.25 + 3 * U * 0.25 * sum(r.abs() for r, _ in rb)
        raw = sum(xc.double() for xc in subs) * 0.25
        rawb = 3 * U * 0.25 * sum(xc.double().abs() for xc in subs) + FLT_MIN
    else:
        ref, bound = _one(c, d, subs[0])
        raw, rawb = subs[0].double(), torch.zeros_like(ref)
    res = dict(out=(lay(ref, c["pad"]), lay(bound, c["pad"])), raw=None)
    if c["raw"] is not None:
        rp = c["pad"] if c["raw"] != F32 else 0
        res["raw"] = (lay(raw, rp), lay(rawb, rp))
    return res


def wrong_model(c, d, wrong):
    """dict(out=..., raw=...) float64 CB8 tensors of the deliberately wrong pass `wrong`, stored in the output's type"""
    assert wrong in WRONG
    subs = gathered(c, d, wrong) if wrong in ("pick_odd_row", "collage_out_coords", "swap_ij") else d["subs"]
    Ct = sum(c["cins"])
    cdiv = len_blocks(c["size"]) * 8 if wrong == "mean_padded_c" else None
    one = lambda xc, stat=None: (_wrong_one(c, d, xc, stat, cdiv, wrong == "scale_plain") if c["norm"] else _one(c, d, xc)[0])
    if c["rs"] == DOWN2:
        vs = [one(xc, subs[0] if wrong == "one_stat" else None) for xc in subs]
        out = sum(vs) * (1.0 if wrong == "no_quarter" else 0.25)
        raw = sum(xc.double() for xc in subs) * (1.0 if wrong == "no_quarter" else 0.25)
    else:
        out, raw = one(subs[0]), subs[0].double()
    assert Ct == out.shape[1]
    out = cb8(out, c["cins"], c["pad"])
    if wrong == "pad_copied":
        assert c["pad"] == 1
        out[:, -1] = out[:, -2]
    res = dict(out=out.to(TORCH[c["out"]]), raw=None)
    if c["raw"] is not None:
        res["raw"] = cb8(raw, c["cins"], c["pad"] if c["raw"] != F32 else 0).to(TORCH[c["raw"]])
    return res


def emulate_f32(c, d):
    """The kernel's evaluation in float32, in its own order (test_gpu_prep_wide._emulate_f32: 8-term fused sums per block, four
    chains over the blocks from 0.f, c0 + c1 + c2 + c3); down2: o = 0.f + v0 + v1 + v2 + v3 in that order, times 0.25.  Stored in
    the output's type, CB8."""
    def one(xc):
        if c["norm"]:
            return pw._emulate_f32(xc, d["ws"], d["scale"], d["shift"], c["mod"], c["act"], c["per_image"], c["mod_half"])
        return F.silu(xc) if c["act"] else xc
    vs = [one(xc) for xc in d["subs"]]
    if c["rs"] == DOWN2:
        out = (((vs[0] + vs[1]) + vs[2]) + vs[3]) * 0.25
        raw = (((d["subs"][0] + d["subs"][1]) + d["subs"][2]) + d["subs"][3]) * 0.25
    else:
        out, raw = vs[0], d["subs"][0]
    res = dict(out=cb8(out, c["cins"], c["pad"]).to(TORCH[c["out"]]), raw=None)
    if c["raw"] is not None:
        res["raw"] = cb8(raw, c["cins"], c["pad"] if c["raw"] != F32 else 0).to(TORCH[c["raw"]])
    return res


# ---- the check ---------------------------------------------------------------------------------------------------------------
def check_tensor(got, ref, bound, dt, pad_blocks=0):
    """got (CB8, its own type, CPU) against (ref, bound) float64.  Returns (ok, worst |d| / bound, exact): every element is
    compared; an element with bound 0 must be equal (ratio inf otherwise); pad blocks must be zero in bits; exact = every element
    equals the (rounded) reference."""
    if got.shape != ref.shape or bool(torch.isnan(got.float()).any()):
        return False, float("inf"), False
    g = got.double()
    if dt == F32:
        centre, dist = ref, bound
        ok = (g - ref).abs() <= bound
    else:
        centre, lo, hi = r16(ref, dt), r16(ref - bound, dt), r16(ref + bound, dt)
        flush = ((ref - bound).abs() < TINY[dt]) | ((ref + bound).abs() < TINY[dt])
        ok = ((g >= lo) & (g <= hi)) | ((g == 0) & flush)
        dist = torch.maximum(hi - centre, centre - lo)
    dd = (g - centre).abs()
    ratio = torch.where(dist > 0, dd / dist.clamp_min(1e-300), torch.where(dd > 0, torch.full_like(dd, float("inf")), torch.zeros_like(dd)))
    ratio = torch.where(ok, ratio.clamp_max(1.0), ratio)                     # an admitted flush to zero is inside
    good = bool(ok.all())
    if pad_blocks and dt != F32:
        good = good and bool((got[:, -pad_blocks:].contiguous().view(torch.int16) == 0).all())
    return good, float(ratio.max()), bool((dd == 0).all())


def check(c, ref, res):
    """res: dict(out=..., raw=...) of CB8 tensors in their own types.  (ok, worst ratio, exact)"""
    ok, worst, exact = check_tensor(res["out"], *ref["out"], c["out"], c["pad"])
    if c["raw"] is not None:
        ok2, w2, ex2 = check_tensor(res["raw"], *ref["raw"], c["raw"], c["pad"] if c["raw"] != F32 else 0)
        ok, worst, exact = ok and ok2, max(worst, w2), exact and ex2
    return ok, worst, exact
