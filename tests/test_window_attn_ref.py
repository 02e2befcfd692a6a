"""CPU: the float64 model of the inference attention cores (train_op_ref.window_attn_fwd, what tests/test_gpu_window_attn.py
holds the nine HIP kernels to) against the oracle, and its bound against deliberately wrong variants: the bound must accept a
plain fp32 (and 16-bit rounded) restatement of the operation and reject every error of R.ATTN_WRONG in at least one element."""
import pytest
import torch

import train_op_ref as R
from oracle import teramind_cpu as tc


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _d(q, kv, qw, kw):
    return q.double(), kv.double(), qw, kw


@pytest.mark.parametrize("Z,S", [(2, 8), (1, 4), (3, 12)])
def test_full_resolution_model_matches_oracle(Z, S):
    """With identity q / k / proj Linears and a random v Linear the model (no rounding) is the oracle's
    windowed_cross_attention; k and v differ, as the two halves of the kv tensor do."""
    g = _g(2)
    N, C = 2, 13
    q, kin = (torch.randn(N, C, Z, S, S, generator=g, dtype=torch.float64) for _ in range(2))
    M = torch.randn(C, C, generator=g, dtype=torch.float64) * 0.3
    qw, kw = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    eye, zero = torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    W = {f"a.{n}.weight": eye for n in ("q", "k", "proj")}
    W["a.v.weight"] = M
    W.update({f"a.{n}.bias": zero for n in ("q", "k", "v", "proj")})
    W["a.q_norm.weight"], W["a.k_norm.weight"] = qw.double(), kw.double()
    tok = lambda t: t.permute(0, 2, 3, 4, 1).reshape(N, Z * S * S, C)
    ref = tc.windowed_cross_attention(W, "a", tok(q), tok(kin), Z)
    v = torch.einsum("dc,nczyx->ndzyx", M, kin)
    got, bound, mag = R.window_attn_fwd(q, torch.cat([kin, v], 1), qw, kw, Z, S, mag=True)
    assert torch.allclose(tok(got), ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(got, R.window_attn(q, kin, v, qw.double(), kw.double(), Z, S), rtol=1e-12, atol=1e-12)
    # the magnitude companion bounds what it accompanies, and the bound is positive
    assert torch.all(got.abs() <= mag["omag"] * (1 + 1e-12)) and torch.all(mag["l"].abs() <= mag["lmag"] * (1 + 1e-12))
    assert torch.all(bound > 0)


@pytest.mark.parametrize("dt", [None, "bf16", "f16"])
@pytest.mark.parametrize("Z,S", [(2, 8), (1, 4), (2, 16)])
def test_half_resolution_model_equals_full_resolution_on_upsampled_kv(Z, S, dt):
    q, kv, qw, kw = _d(*R.attn_inputs(2, 16, Z, S, True, seed=3))
    up = kv.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    a, ba = R.window_attn_fwd(q, kv, qw, kw, Z, S, dt, True)
    b, bb = R.window_attn_fwd(q, up, qw, kw, Z, S, dt, False)
    assert torch.equal(a, b) and torch.equal(ba, bb)
    assert torch.equal(R.kv_full(kv, S), up)


def test_zero_tokens_get_the_mean_of_v():
    """An all-zero q token has logits 0 against every key: its output is the mean of its window's v."""
    Z, S, C = 2, 8, 16
    q, kv, qw, kw = _d(*R.attn_inputs(3, C, Z, S, False, "zeros", 4))
    o, _ = R.window_attn_fwd(q, kv, qw, kw, Z, S)
    vmean = R.from_windows(R.to_windows(kv[:, C:], Z, S).mean(2, keepdim=True).expand(-1, -1, Z * 16, -1), Z, S)
    assert torch.allclose(o[:, :, :, 0, :], vmean[:, :, :, 0, :], rtol=1e-12, atol=1e-14)
    assert float(o[2].abs().max()) == 0.0                  # the patch whose k / v are all zero


# ---- the bounds must bite ------------------------------------------------------------------------------------------------
def _restated(q, kv, qw, kw, Z, S, dt, kv_half):
    """The operation once more in plain fp32 torch, written the way tests/test_gpu_ops.py states it (normalise, weight, one
    softmax); for a 16-bit type with the operands, P and the output rounded to it."""
    C = q.shape[1]
    td = R.H16[dt][0] if dt else None
    rnd = (lambda t: t.to(td).float()) if dt else (lambda t: t)
    q, kv = rnd(q.float()), rnd(kv.float())
    k, v = kv[:, :C], kv[:, C:]
    if kv_half:
        k, v = (t.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4) for t in (k, v))
    qs, ks, vs = (R.to_windows(t, Z, S) for t in (q, k, v))
    rms = lambda t: torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)
    if dt:
        logits = (rnd(qs * (qw * kw)) @ ks.transpose(-2, -1)) * (rms(qs) / C) * rms(ks).transpose(-2, -1)
    else:
        logits = ((qs * rms(qs) * qw) / C) @ (ks * rms(ks) * kw).transpose(-2, -1)
    return R.from_windows(rnd(rnd(torch.softmax(logits, -1)) @ vs), Z, S).double()


# (C, Z, S, kv_half, dt): one small case per kernel form and bound formula -- fp32 MFMA T = 128, T = 32, long T = 256 / 512,
# generic (T = 16, 64); 16-bit T = 128 / 64 / 32 and long T = 256 / 512 in both types; half-resolution k / v where a form has it
BITE_F32 = [(128, 2, 16, False), (128, 2, 16, True), (128, 2, 8, False), (128, 2, 8, True), (64, 4, 16, False), (64, 8, 16, False),
            (64, 4, 4, False), (64, 4, 8, False)]
BITE_H16 = [(64, 2, 16, False), (64, 2, 16, True), (64, 4, 8, False), (64, 4, 8, True), (64, 2, 8, False), (64, 2, 8, True),
            (64, 4, 16, False), (64, 8, 16, False)]
BITE_CASES = [c + (None,) for c in BITE_F32] + [c + (dt,) for dt in ("bf16", "f16") for c in BITE_H16]


@pytest.mark.parametrize("C,Z,S,kv_half,dt", BITE_CASES)
def test_bound_accepts_the_restatement_and_rejects_every_wrong_variant(C, Z, S, kv_half, dt):
    """Every case has Z > 1 and S / 2 > 1, so the (h, w, z) token order differs from (z, h, w).  "hwz" orders the QUERY tokens
    (h, w, z) while the output is written back (z, h, w): attention is equivariant under one common permutation of a
    window's tokens, so a wrong order only shows where the read and the write disagree."""
    q, kv, qw, kw = R.attn_inputs(1, C, Z, S, kv_half, seed=5)
    qd, kvd = q.double(), kv.double()
    ref, bound = R.window_attn_fwd(qd, kvd, qw, kw, Z, S, dt, kv_half)
    d = (_restated(q, kv, qw, kw, Z, S, dt, kv_half) - ref).abs()
    assert bool((d <= bound).all()), f"restatement outside the bound: worst |d|/bound = {float((d / bound.clamp_min(1e-300)).max()):.3g}"
    for wrong in R.ATTN_WRONG:
        if wrong == "kv_mod" and not kv_half:
            continue
        bad, _ = R.window_attn_fwd(qd, kvd, qw, kw, Z, S, dt, kv_half, wrong=wrong)
        out = ((bad - ref).abs() > bound)
        assert bool(out.any()), f"{wrong}: inside the bound everywhere"
