"""Cases, float64 model and bounds of the stem and head kernels on their own (tm_kernels.hip stem_kernel, head_kernel<H16, CO>;
hooks tm_op_stem / tm_op_head).  Shared by tests/test_stem_head_cases_host.py (no GPU) and tests/test_gpu_stem_head.py.

STEM  x NCHW '(s z) h w' [N][Cin Z][S][S] -> Conv3d(Cin -> Cout, (1, 3, 3), pad (0, 1, 1)) -> CB8 [N][Cout / 8][Z][S][S][8] in fp32,
      bf16 or f16.  A thread owns one voxel and 32 couts: acc = bias, then one FMA per (cin, ky, kx) in that order.
HEAD  x CB8 (fp32, bf16 or f16, pad channels zero by contract) -> Conv3d(C -> Cout <= 8, (1, 3, 3)) -> fp32 NCHW [N][Cout Z][S][S].
      acc = 0, one FMA per (channel block, ky, kx, channel of the block), then + bias.  head_kernel<*, 4> computes 4 couts
      (Cout 1, 2, 4 here), head_kernel<*, 8> 8 (Cout 3, 5, 8).

Z S S N is never a multiple of 256 here (the largest is 3 * 36 * 3 = 324: one full workgroup and a partly filled one), so the
guard of the last workgroup `vidx >= vpn * N` is exercised by every case.

INTEGER CASES  x in [-3, 3], w in [-2, 2], b in [-4, 4].  Stem: every partial sum is an integer of magnitude <= 9 * 2 * 6 + 4 = 112,
exact in fp32, f16 (integers to 2048) and bf16 (to 256).  Head: <= 9 * 128 * 6 + 4 < 2^24.  Every order of summation and every
fusing gives the same bits: the criterion is equality with F.conv3d.
RANDOM CASES  bound L U mag, U = 2^-24, mag the expression on absolute values in float64, L the roundings a term passes through:
stem 9 Cin FMAs and one for the second-order terms, (9 Cin + 1); head 72 Cb FMAs (Cb channel blocks) and the bias add,
(72 Cb + 1).  A 16-bit stem output then lies in the interval a monotone rounding of [ref - bound, ref + bound] reaches
(prep_form_cases.check_tensor).  No constant comes from an observed error.
"""
import itertools

import torch
import torch.nn.functional as F

from prep_form_cases import BF16, F16, F32, TORCH, check_tensor     # noqa: F401  (re-exported for the tests)
from test_gpu_prep_wide import _fma

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
GEO = [(Z, S, N) for Z in (1, 2, 3) for S in (4, 6) for N in (1, 3)]
assert all((Z * S * S * N) % 256 for Z, S, N in GEO)

# (kernel, Cin, Cout, Z, S, N, dtype, kind)
STEM_INT = [("stem", Cin, Cout, Z, S, N, dt, "int") for Cin in (1, 2) for Cout in (32, 64, 96) for Z, S, N in GEO for dt in (F32, BF16, F16)]
STEM_RAND = [("stem", 2, 96, 3, 6, 3, dt, "rand") for dt in (F32, BF16, F16)]
# the head runs every geometry in every type in both CO forms, and walks the nine (C, Cout) pairs of a form along them
_HC = [list(itertools.product((24, 64, 128), couts)) for couts in ((1, 2, 4), (3, 5, 8))]
HEAD_INT = [("head", *_HC[co][k % 9], *geo, dt, "int") for co in (0, 1) for k, (geo, dt) in enumerate(itertools.product(GEO, (F32, BF16, F16)))]
HEAD_INT += [("head", 61, Cout, *GEO[k], dt, "int") for k, (Cout, dt) in enumerate([(2, F32), (5, BF16), (8, F16), (4, BF16), (3, F32), (1, F16)])]
HEAD_RAND = [("head", 128, 5, 3, 6, 3, dt, "rand") for dt in (F32, BF16, F16)]
CASES = STEM_INT + STEM_RAND + HEAD_INT + HEAD_RAND

WRONG = {"stem": ["zs_unfold", "kykx_swapped", "bias_group0", "one_sided_pad"], "head": ["kykx_swapped", "one_sided_pad", "plane_stride"]}


def case_id(c):
    return "%s-C%d-Co%d-Z%dS%dN%d-%s-%s" % (c[:6] + ("f32 bf16 f16".split()[c[6]], c[7]))


def make(c):
    """x [N, Cin, Z, S, S] (the stem's '(s z)' channel order is this tensor's memory order; the head's x holds values of its
    type), w [Cout, Cin, 1, 3, 3], b [Cout]: fp32 on the CPU"""
    kern, Cin, Cout, Z, S, N, dt, kind = c
    g = torch.Generator().manual_seed(7000 + Cin * 131 + Cout * 17 + Z * 5 + S * 3 + N + 1000 * dt + (50000 if kern == "stem" else 0))
    if kind == "int":
        x = torch.randint(-3, 4, (N, Cin, Z, S, S), generator=g).float()
        w = torch.randint(-2, 3, (Cout, Cin, 1, 3, 3), generator=g).float()
        b = torch.randint(-4, 5, (Cout,), generator=g).float()
    else:
        x = torch.randn((N, Cin, Z, S, S), generator=g)
        w = torch.randn((Cout, Cin, 1, 3, 3), generator=g) / (9 * Cin) ** 0.5
        b = torch.randn((Cout,), generator=g)
    if kern == "head":
        x = x.to(TORCH[dt]).float()
    return x, w, b


def _conv(x, w, b, wrong=None):
    if wrong == "kykx_swapped":
        w = w.transpose(-1, -2)
    if wrong == "one_sided_pad":                       # zeros above and left only; below and right the border value is read again
        xp = F.pad(F.pad(x, (1, 0, 1, 0)), (0, 1, 0, 1, 0, 0), mode="replicate")
        return F.conv3d(xp, w, b)
    return F.conv3d(x, w, b, padding=(0, 1, 1))


def reference(c, x, w, b, wrong=None):
    """(ref, bound) float64: the stem's in CB8 [N][Cout / 8][Z][S][S][8], the head's NCDHW [N, Cout, Z, S, S] (its NCHW memory)"""
    kern, Cin, Cout, Z, S, N, dt, kind = c
    xd, wd, bd = x.double(), w.double(), b.double()
    if wrong == "zs_unfold":                           # the state read as '(z s) h w'
        xd = xd.reshape(N, Z, Cin, S, S).transpose(1, 2)
    if wrong == "bias_group0":                         # every 32-cout group adds the first group's bias
        bd = bd[:32].repeat(Cout // 32)
    ref = _conv(xd, wd, bd, wrong)
    if wrong == "plane_stride":                        # cout planes S S apart instead of Z S S: later writes land on earlier ones
        flat = torch.full((N * Cout * Z * S * S,), float("nan"), dtype=torch.float64)
        for n in range(N):
            for j in range(Cout):
                for z in range(Z):
                    o = ((n * Cout + j) + z) * S * S
                    flat[o:o + S * S] = ref[n, j, z].reshape(-1)
        ref = flat.reshape(ref.shape)
    L = 9 * Cin + 1 if kern == "stem" else 72 * ((Cin + 7) // 8) + 1
    bound = torch.zeros_like(ref) if kind == "int" else L * U * _conv(xd.abs(), wd.abs(), bd.abs()) + FLT_MIN
    if kern == "stem":
        lay = lambda t: t.reshape(N, Cout // 8, 8, Z, S, S).permute(0, 1, 3, 4, 5, 2).contiguous()
        return lay(ref), lay(bound)
    return ref, bound


def emulate_f32(c, x, w, b):
    """the kernel's chain in float32: stem acc = bias, FMAs over (cin, ky, kx); head acc = 0, FMAs over (block, ky, kx, channel of
    the block) -- which is (cin, ky, kx) regrouped -- then + bias.  Stored in the output's type and layout."""
    kern, Cin, Cout, Z, S, N, dt, kind = c
    xp = F.pad(x, (1, 1, 1, 1))
    acc = (b if kern == "stem" else torch.zeros(Cout)).view(1, Cout, 1, 1, 1).expand(N, Cout, Z, S, S).contiguous()
    order = [(ci, ky, kx) for ci in range(Cin) for ky in range(3) for kx in range(3)] if kern == "stem" else \
            [(ci, ky, kx) for cb in range((Cin + 7) // 8) for ky in range(3) for kx in range(3) for ci in range(cb * 8, min(cb * 8 + 8, Cin))]
    for ci, ky, kx in order:
        acc = _fma(w[:, ci, 0, ky, kx].view(1, Cout, 1, 1, 1), xp[:, ci, :, ky:ky + S, kx:kx + S].unsqueeze(1), acc)
    if kern == "head":
        return acc + b.view(1, Cout, 1, 1, 1)
    return acc.reshape(N, Cout // 8, 8, Z, S, S).permute(0, 1, 3, 4, 5, 2).contiguous().to(TORCH[dt])


def check(c, ref, bound, got):
    """(ok, worst |d| / bound, exact); an integer case must be exact"""
    ok, worst, exact = check_tensor(got, ref, bound, c[6] if c[0] == "stem" else F32)
    return ok and (exact or c[7] != "int"), worst, exact
