"""-m gpu: every inference window-attention kernel (tm_attn.hip: window_attn_mfma_kernel, window_attn_kernel<32>,
window_attn_mfma_long_kernel<256 / 512>, window_attn_generic_kernel; tm_conv_bf16.hip, compiled for bf16 and f16:
window_attn_bf16<128 / 64 / 32>, window_attn_long<256 / 512>) through tm_op_window_attn_kv, which hands them k and v as the
two channel halves of one kv tensor at full or half in-plane resolution, the way attn_block (tm_model.hip) does.

Rules of every case (the house style of test_gpu_conv_zpair.py and test_window_attn_train):
  * the output starts as NaN: every element must be written;
  * the launch is made twice and the two results must agree in bits;
  * the result is compared element by element with the float64 model train_op_ref.window_attn_fwd, against the bound that
    function derives from the kernels' accumulation lengths and rounding points (its docstring holds the derivation: U = 2^-24,
    R.exp_rel_bound for the device expf, and for the 16-bit kernels the interval of 16-bit values a monotone rounding can
    reach).  No constant in it comes from an observed error; tests/test_window_attn_ref.py shows on the CPU that it rejects
    a wrong scale, a dropped key, swapped v tokens, the wrong norm weight, a wrong token order and a wrong half-resolution read;
  * the worst |d| / bound of the case is printed and appended to window_attn_bounds.txt in the suite's output directory (the out_dir fixture).

Case -> kernel (T = Z (S/2)^2 tokens per window), see kernel_of():
  fp32   T = 128, C % 128 == 0, C <= 512      window_attn_mfma_kernel                 (+ half-resolution k / v)
         T = 32, C % 128 == 0                 window_attn_kernel<32>                  (+ half-resolution k / v)
         T = 256 / 512, C <= 256              window_attn_mfma_long_kernel<256 / 512>
         everything else                      window_attn_generic_kernel
  16-bit T = 128 / 64 / 32                    window_attn_bf16<T>   (bf16 and f16 builds; + half-resolution k / v)
         T = 256 / 512, C <= 256              window_attn_long<T>   (bf16 and f16 builds)
The 16-bit T = 64 and T = 32 forms put two and four windows into a workgroup, but a workgroup never spans two patches (the
grid is N * 2 and N * 1 workgroups), so there is no partly filled last workgroup: N = 1, 3 and 5 cover odd counts all the same.

Shapes of the shipped models (attention at resolution 16 and in the middle block; Z = 1, 2, 4, 8 for rna_slc 1, 4, 8, 16):
patch 64: (C, S) = (256, 16), (512, 8); patch 32 (fp32 only): (128, 16), (512, 4); patch 128: (512, 16) twice."""
import os

import pytest
import torch

import train_op_ref as R
import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
DTYPE = {None: (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}


def kernel_of(C, Z, S, dt):
    T = Z * (S // 2) ** 2
    if dt:
        return f"window_attn_long<{T}> {dt}" if T >= 256 else f"window_attn_bf16<{T}> {dt}"
    if T in (256, 512) and C <= 256:
        return f"window_attn_mfma_long_kernel<{T}>"
    if T == 128 and C % 128 == 0:
        return "window_attn_mfma_kernel"
    if T == 32 and C % 128 == 0:
        return "window_attn_kernel<32>"
    return "window_attn_generic_kernel"


def _run(q, kv, qw, kw, Z, S, dt, kv_half):
    N, C = q.shape[:2]
    code, td = DTYPE[dt]
    qc, kvc = util.to_cb8(q.to(DEV)), util.to_cb8(kv.to(DEV))
    qwd, kwd = qw.to(DEV), kw.to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((N, C // 8, Z, S, S, 8), NAN, dtype=td, device=DEV)
        _lib.check(_lib.lib().tm_op_window_attn_kv(_lib.ptr(qc), _lib.ptr(kvc), _lib.ptr(qwd), _lib.ptr(kwd), _lib.ptr(out), N, C, Z, S,
                                                   code, int(kv_half), _lib.current_stream_ptr()), "tm_op_window_attn_kv")
        outs.append(out)
    bits = torch.int32 if dt is None else torch.int16
    assert torch.equal(outs[0].view(bits), outs[1].view(bits)), "two launches on the same inputs differ in bits"
    assert not torch.isnan(outs[0]).any(), f"{int(torch.isnan(outs[0]).sum())} output elements not written"
    return util.from_cb8(outs[0].float(), C).cpu().double()


def _check(N, C, Z, S, kv_half, dt, kind, out_dir):
    q, kv, qw, kw = R.attn_inputs(N, C, Z, S, kv_half, kind, seed=11)
    got = _run(q, kv, qw, kw, Z, S, dt, kv_half)
    ref, bound = R.window_attn_fwd(q.double(), kv.double(), qw, kw, Z, S, dt, kv_half)
    d = (got - ref).abs()
    ratio = d / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    line = (f"{kernel_of(C, Z, S, dt):40s} kv_half={int(kv_half)} {kind:5s} N={N} C={C} Z={Z} S={S}  worst |d|/bound = {worst:.3g}  "
            f"max|d| = {float(d.max()):.3e}  exact = {float((d == 0).double().mean()):.4f}")
    print(line)
    with open(os.path.join(out_dir, "window_attn_bounds.txt"), "a") as f:
        f.write(line + "\n")
    if worst > 1.0:
        i = int(ratio.argmax())
        n, c, z, y, x = (int(t) for t in torch.unravel_index(torch.tensor(i), ratio.shape))
        hs = S // 2
        where = (f"n={n} c={c} z={z} y={y} x={x}: window {(y // hs) * 2 + x // hs}, token {(z * hs + y % hs) * hs + x % hs}, "
                 f"got {float(got[n, c, z, y, x])!r} ref {float(ref[n, c, z, y, x])!r} bound {float(bound[n, c, z, y, x]):.3e}")
        pytest.fail(f"{line}\n  {int((ratio > 1).sum())} of {ratio.numel()} elements outside the bound; worst at {where}")


def _with_n(cases):
    return [((1, 3, 5)[i % 3],) + c for i, c in enumerate(cases)]


# ---- fp32 (C, Z, S, kv_half) ---------------------------------------------------------------------------------------------------
F32_MFMA = [(C, Z, S, h) for C in (128, 256, 384, 512) for Z, S in ((2, 16), (8, 8)) for h in (False, True)]
F32_T32 = [(C, Z, S, h) for C in (128, 512) for Z, S in ((2, 8), (8, 4)) for h in (False, True)]
F32_LONG = [(C, Z, S, False) for Z, S in ((4, 16), (1, 32), (8, 16), (2, 32)) for C in (64, 128, 256)]
# generic: T = 64 (the z_size 1 and 4 models), T = 16, 8, 2, 1; T = 128 off the MFMA kernel's C % 128 rule; T = 256 with C = 512
# (patch 128, z_size 4) and T = 512 with C = 384 (past the long kernel's C <= 256); then the shipped shapes not listed yet:
# (512, 1, 8) T = 16, (512, 1, 4) T = 4, (512, 2, 4) T = 8, (512, 4, 4) T = 16, (128 / 512, 1, 16) T = 64
F32_GENERIC = [(256, 1, 16, False), (512, 4, 8, False), (64, 4, 4, False), (64, 2, 4, False), (64, 2, 2, False), (64, 1, 2, False),
               (64, 2, 16, False), (192, 2, 16, False), (512, 4, 16, False), (384, 8, 16, False),
               (512, 1, 8, False), (512, 1, 4, False), (512, 2, 4, False), (512, 4, 4, False), (128, 1, 16, False), (512, 1, 16, False)]


@pytest.mark.parametrize("N,C,Z,S,kv_half", _with_n(F32_MFMA + F32_T32 + F32_LONG + F32_GENERIC))
def test_window_attn_f32(N, C, Z, S, kv_half, out_dir):
    _check(N, C, Z, S, kv_half, None, "plain", out_dir)


# ---- bf16 and f16 ----------------------------------------------------------------------------------------------------------------
# every S here is a multiple of 4, so each (C, Z, S) runs with k / v at full and at half resolution
H16_SHORT = [(C, Z, S, h) for Z, S in ((2, 16), (8, 8), (1, 16), (4, 8), (2, 8), (8, 4)) for C in (64, 128, 192, 256, 512)
             for h in (False, True)]
H16_LONG = [(C, Z, S, False) for Z, S in ((4, 16), (1, 32), (8, 16), (2, 32)) for C in (64, 256)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("N,C,Z,S,kv_half", _with_n(H16_SHORT + H16_LONG))
def test_window_attn_h16(N, C, Z, S, kv_half, dt, out_dir):
    _check(N, C, Z, S, kv_half, dt, "plain", out_dir)


# ---- near one-hot softmax and all-zero tokens, one case per kernel form --------------------------------------------------------------
EDGE_F32 = [(3, 256, 2, 16, True), (3, 512, 2, 8, True), (3, 256, 4, 16, False), (3, 128, 8, 16, False), (3, 256, 1, 16, False)]
EDGE_H16 = [(3, 256, 2, 16, True), (3, 512, 4, 8, True), (5, 512, 2, 8, True), (3, 256, 4, 16, False), (3, 64, 8, 16, False)]


@pytest.mark.parametrize("kind", ["sharp", "zeros"])
@pytest.mark.parametrize("N,C,Z,S,kv_half,dt", [c + (None,) for c in EDGE_F32] + [c + (dt,) for dt in ("bf16", "f16") for c in EDGE_H16])
def test_window_attn_edges(N, C, Z, S, kv_half, dt, kind, out_dir):
    """sharp: q_norm.weight times 60, logits spanning several tens, the max subtraction matters.  zeros: all-zero q tokens
    (uniform softmax, the mean of v), all-zero k / v tokens and one patch whose k / v are zero throughout."""
    _check(N, C, Z, S, kv_half, dt, kind, out_dir)


# ---- rejections: TM_ERR_ARG before any device call ---------------------------------------------------------------------------------
# (C, Z, S, dtype code, kv_half, a word of the error text)
REJECT = [(256, 4, 16, 0, 1, "half-resolution"), (256, 8, 16, 0, 1, "half-resolution"),       # kv_half at T = 256 / 512, fp32
          (256, 4, 16, 1, 1, "long windows"), (64, 8, 16, 2, 1, "long windows"),              # ... and 16-bit
          (512, 4, 16, 1, 0, "> 256"), (320, 8, 16, 2, 0, "> 256"),                           # C > 256 with a long window, 16-bit
          (100, 2, 16, 0, 0, "multiple of 64"), (72, 2, 16, 1, 0, "multiple of 64"),          # C % 64 != 0
          (256, 2, 7, 0, 0, "even S"), (256, 2, 15, 2, 0, "even S"),                          # odd S
          (64, 16, 16, 0, 0, "at most 512"), (64, 3, 32, 1, 0, "at most 512"),                # T > 512
          (576, 2, 16, 0, 0, "> 512"), (576, 1, 16, 0, 0, "> 512"), (576, 2, 16, 1, 0, "> 512"),   # C > 512
          (64, 2, 16, 0, 1, "half-resolution"), (256, 1, 16, 0, 1, "half-resolution"),        # fp32 kv_half off the MFMA / T = 32 kernels
          (256, 32, 2, 1, 1, "multiple of 4"),                                                # 16-bit kv_half with S % 4 != 0
          (256, 4, 4, 1, 0, "32, 64, 128"), (256, 3, 8, 2, 0, "32, 64, 128"),                 # 16-bit window of 16 / 48 tokens
          (256, 2, 16, 3, 0, "dtype"), (256, 0, 16, 0, 0, "even S")]


def test_window_attn_rejections():
    """Every form the launchers refuse comes back as TM_ERR_ARG (-1) with a text, before any device call: the pointers handed
    over here are never dereferenced."""
    L = _lib.lib()
    buf = torch.zeros(8)
    p = _lib.ptr(buf)
    for C, Z, S, code, kv_half, word in REJECT:
        rc = L.tm_op_window_attn_kv(p, p, p, p, p, 1, C, Z, S, code, kv_half, None)
        assert rc == -1, (C, Z, S, code, kv_half, rc)
        assert word.encode() in L.tm_last_error(), (C, Z, S, code, kv_half, L.tm_last_error())
    assert L.tm_op_window_attn_kv(p, None, p, p, p, 1, 256, 2, 16, 0, 0, None) == -1 and b"null" in L.tm_last_error()
