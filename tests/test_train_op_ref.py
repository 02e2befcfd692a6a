"""CPU: the float64 references of tests/train_op_ref.py (what tests/test_gpu_train_ops.py holds the training kernels to)
against torch.autograd and the oracle."""
import pytest
import torch

import train_op_ref as R
from oracle import teramind_cpu as tc


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_rms_rows_backward_matches_autograd():
    g = _g(0)
    x = torch.randn(7, 37, generator=g, dtype=torch.float64).requires_grad_(True)
    w = (torch.rand(37, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    dy = torch.randn(7, 37, generator=g, dtype=torch.float64)
    y = tc.rms_norm_last(x, w)
    assert torch.allclose(R.rms_rows(x, w)[0], y)
    y.backward(dy)
    dx, dw = R.rms_rows_bwd(x.detach(), w.detach(), dy)
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-12) and torch.allclose(dw, w.grad, rtol=1e-12, atol=1e-12)


def test_softmax_backward_matches_autograd():
    g = _g(1)
    x = (torch.randn(5, 65, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    dy = torch.randn(5, 65, generator=g, dtype=torch.float64)
    p = torch.softmax(x, -1)
    p.backward(dy)
    assert torch.allclose(R.softmax_bwd(p.detach(), dy), x.grad, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("fn,grad,ref", [(R.gelu_tanh, R.gelu_tanh_grad, tc.gelu_tanh), (R.silu, R.silu_grad, tc.silu)])
def test_activation_derivatives_match_autograd(fn, grad, ref):
    x = torch.linspace(-12, 12, 1001, dtype=torch.float64).requires_grad_(True)
    y = ref(x)
    assert torch.allclose(fn(x.detach()), y.detach(), rtol=1e-12, atol=1e-14)     # 1 + tanh cancels in float64 too
    y.sum().backward()
    assert torch.allclose(grad(x.detach()), x.grad, rtol=1e-12, atol=1e-14)


def test_window_partition_and_core_match_oracle():
    """The core with identity q / k / v / proj Linears is the oracle's windowed_cross_attention (tokens ordered (z h w))."""
    g = _g(2)
    N, C, Z, S = 2, 13, 2, 8
    q, k = torch.randn(N, C, Z, S, S, generator=g, dtype=torch.float64), torch.randn(N, C, Z, S, S, generator=g, dtype=torch.float64)
    qw, kw = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    assert torch.equal(R.from_windows(R.to_windows(q, Z, S), Z, S), q)
    eye, zero = torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    W = {f"a.{n}.weight": eye for n in ("q", "k", "v", "proj")}
    W.update({f"a.{n}.bias": zero for n in ("q", "k", "v", "proj")})
    W["a.q_norm.weight"], W["a.k_norm.weight"] = qw, kw
    tok = lambda t: t.permute(0, 2, 3, 4, 1).reshape(N, Z * S * S, C)
    # q and k differ, v = k (cross attention: k and v come from the same tokens)
    ref = tc.windowed_cross_attention(W, "a", tok(q), tok(k), Z)
    got = R.window_attn(q, k, k, qw, kw, Z, S)
    assert torch.allclose(tok(got), ref, rtol=1e-12, atol=1e-12)


def test_window_attn_magnitudes_bound_the_gradients():
    """Every gradient of the core is at most its magnitude (the sums over |terms| of window_attn_mag)."""
    g = _g(3)
    N, C, Z, S = 1, 8, 2, 8
    q, k, v, d = (torch.randn(N, C, Z, S, S, generator=g, dtype=torch.float64) for _ in range(4))
    qw, kw = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, qw, kw)]
    o = R.window_attn(*leaves, Z, S)
    o.backward(d)
    mag, _ = R.window_attn_mag(q, k, v, qw, kw, d, Z, S)
    assert torch.all(o.detach().abs() <= mag["o"] * (1 + 1e-12))
    for name, t in zip(("dq", "dk", "dv", "dqw", "dkw"), leaves):
        assert torch.all(t.grad.abs() <= mag[name] * (1 + 1e-12) + 1e-15), name


@pytest.mark.parametrize("step,wd,gscale", [(1, 0.0, 1.0), (1000, 0.05, 0.37)])
def test_adam_formula_matches_torch(step, wd, gscale):
    g = _g(4)
    p = torch.randn(33, generator=g, dtype=torch.float64)
    gr = torch.randn(33, generator=g, dtype=torch.float64)
    m0 = torch.randn(33, generator=g, dtype=torch.float64) * 0.1 if step > 1 else torch.zeros(33, dtype=torch.float64)
    v0 = torch.rand(33, generator=g, dtype=torch.float64) * 0.1 if step > 1 else torch.zeros(33, dtype=torch.float64)
    f = lambda a: float(torch.tensor(a, dtype=torch.float32))
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    pt = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([pt], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps), weight_decay=f(wd))
    opt.state[pt] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    pt.grad = gr * f(gscale)
    opt.step()
    p2, m2, v2, _, _ = R.adam(p, gr, m0, v0, lr, b1, b2, eps, wd, step, gscale)
    assert torch.allclose(p2, pt.detach(), rtol=1e-12, atol=1e-15)
    assert torch.allclose(m2, opt.state[pt]["exp_avg"], rtol=1e-12) and torch.allclose(v2, opt.state[pt]["exp_avg_sq"], rtol=1e-12)


def test_silu_hw_bound_covers_a_float32_silu():
    """Sanity: the bound is at least the error of a correctly rounded fp32 SiLU chain and stays below 1e-6 for |x| <= 4."""
    x = torch.linspace(-20, 20, 4001, dtype=torch.float64)
    x32 = x.float()
    y32 = (x32 * torch.reciprocal(1 + torch.exp2(x32 * -1.4426950408889634))).double()
    ref = R.silu(x32.double())
    b = R.silu_hw_rel_bound(x32.double())
    assert torch.all((y32 - ref).abs() <= b * ref.abs() + R.FLT_MIN)
    assert float(b[x.abs() <= 4].max()) < 1e-6
