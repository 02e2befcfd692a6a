"""-m gpu: the training attention core at short windows (tm_op_window_attn_train, T = 4 / 8 / 16 tokens: attn_short_kernel of
csrc/tm_train.hip, one wave per window) on its own, against float64 autograd of train_op_ref.window_attn.

Bounds: tests/train_short_cases.py derives them from the kernel's accumulation orders (per-lane channel sums and their butterfly,
C-term logit and dP chains, T-term softmax sums and product chains, the window partials of the norm-weight gradients) times
U = 2^-24 times the |terms| magnitudes of train_op_ref.window_attn_mag; its docstring carries the derivation, and
tests/test_window_attn_train_short_ref.py shows that the same bounds reject five deliberate errors.  No tolerance comes from an
observed error.  Every case also checks that two calls give the same bits, that the pad channel slots of the CB8 outputs are
zero and that NaN-filled output buffers are overwritten everywhere.  Input kinds: "plain", "sharp" (near one-hot softmax) and
"zeros" (zero rows: uniform softmax, zero patches)."""
import pytest
import torch

import train_short_cases as L
import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _nan_cb8(N, Cc, Z, S):
    return torch.full((N, (Cc + 7) // 8, Z, S, S, 8), NAN, dtype=torch.float32, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _out_cb8(raw, Cc, name):
    assert not torch.isnan(raw).any(), f"{name}: {int(torch.isnan(raw).sum())} elements not written"
    if Cc % 8:
        assert float(raw[:, -1, ..., Cc % 8:].abs().max()) == 0.0, f"{name}: pad channel slots not zero"
    return util.from_cb8(raw, Cc).cpu().double()


def run_core(q, k, v, qw, kw, d, Z, S, pad=None):
    """Forward and backward, twice each: ([o, o], [(dq, dk, dv, dqw, dkw)] * 2) as the op left them.  `pad`: a value written
    into the pad channel slots of the four CB8 inputs (zeros otherwise)."""
    N, Cc = q.shape[:2]
    qc, kc, vc, dc = (util.to_cb8(t.to(DEV)) for t in (q, k, v, d))
    if pad is not None and Cc % 8:
        for t in (qc, kc, vc, dc):
            t[:, -1, ..., Cc % 8:] = pad
    st = _lib.current_stream_ptr()
    fwd, bwd = [], []
    for _ in range(2):
        o = _nan_cb8(N, Cc, Z, S)
        _lib.check(_lib.lib().tm_op_window_attn_train(_lib.ptr(qc), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(qw), _lib.ptr(kw), None, _lib.ptr(o),
                                                      None, None, None, None, None, N, Cc, Z, S, st), "tm_op_window_attn_train")
        fwd.append(o)
        dq, dk, dv = _nan_cb8(N, Cc, Z, S), _nan_cb8(N, Cc, Z, S), _nan_cb8(N, Cc, Z, S)
        dqw, dkw = torch.full((Cc,), NAN), torch.full((Cc,), NAN)
        _lib.check(_lib.lib().tm_op_window_attn_train(_lib.ptr(qc), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(qw), _lib.ptr(kw), _lib.ptr(dc),
                                                      None, _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(dqw), _lib.ptr(dkw), N, Cc, Z,
                                                      S, st), "tm_op_window_attn_train")
        bwd.append((dq, dk, dv, dqw, dkw))
    return fwd, bwd


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("N,Cc,Z,S", L.SHORT_CASES)
def test_window_attn_train_short(N, Cc, Z, S, kind):
    x = L.inputs(N, Cc, Z, S, kind)
    fwd, bwd = run_core(*x, Z, S)
    assert _same_bits(fwd[0], fwd[1]) and all(_same_bits(a, b) for a, b in zip(*bwd)), "attention core not reproducible"
    ref, mag, lmax = L.reference(*x, Z, S)
    bound = L.bounds(N, Cc, Z, S, mag, lmax)
    dq, dk, dv, dqw, dkw = bwd[0]
    got = dict(o=_out_cb8(fwd[0], Cc, "o"), dq=_out_cb8(dq, Cc, "dq"), dk=_out_cb8(dk, Cc, "dk"), dv=_out_cb8(dv, Cc, "dv"),
               dqw=dqw.double(), dkw=dkw.double())
    bad = []
    for name in L.OUTPUTS:
        d = (got[name] - ref[name]).abs()
        worst = float((d / bound[name].clamp_min(1e-300)).max())
        print(f"RATIO {name} N={N} C={Cc} Z={Z} S={S} {kind}: max|d|={float(d.max()):.3e} worst |d|/bound={worst:.3g}")
        if not bool(((d <= bound[name]) & ~torch.isnan(got[name])).all()):
            bad.append(f"{name}: max|d|={float(d.max()):.3e}, worst |d|/bound={worst:.3g}")
    assert not bad, "; ".join(bad)


def test_pad_slots_of_the_inputs_are_never_read_as_values():
    """The op owns the pad channels of the last CB8 block on the input side too: with NaN in the pad slots of q, k, v and dout
    every output has the bits of the run with zeros there."""
    N, Cc, Z, S = 2, 13, 1, 4
    x = L.inputs(N, Cc, Z, S, "plain")
    fwd, bwd = run_core(*x, Z, S)
    fwd_p, bwd_p = run_core(*x, Z, S, pad=NAN)
    assert _same_bits(fwd[0], fwd_p[0]), "o"
    for name, a, b in zip(("dq", "dk", "dv", "dqw", "dkw"), bwd[0], bwd_p[0]):
        assert _same_bits(a, b), name


def test_other_window_sizes_are_still_refused():
    """A window the cores do not take (18 tokens: Z 2, S 6) is refused before any launch; the message names the token count and
    lists the short sizes."""
    p = torch.zeros(8, device=DEV)
    h = torch.zeros(8)
    rc = _lib.lib().tm_op_window_attn_train(_lib.ptr(p), _lib.ptr(p), _lib.ptr(p), _lib.ptr(h), _lib.ptr(h), None, _lib.ptr(p), None, None,
                                            None, None, None, 1, 64, 2, 6, _lib.current_stream_ptr())
    assert rc == -1
    msg = _lib.lib().tm_last_error().decode()
    assert "18 tokens" in msg and "4, 8, 16, 32" in msg, msg
