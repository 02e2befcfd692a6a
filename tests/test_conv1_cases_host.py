"""No GPU: the float64 model, the case tables and the bounds of tests/test_gpu_conv1_f32.py (tests/conv1_cases.py), and the
host-side pieces of the library they lean on (the tile rule tm_conv1_form, the refusals of the two hooks).

  * the model equals torch's conv3d / tanh-GELU built independently in float64, on every case's data;
  * every deliberate error (conv1_cases.WRONG) that applies to a case changes at least one element of that case's result --
    past the case's bound where the case is held to one -- so a kernel with that error cannot pass;
  * the bounds hold for a float32 evaluation of the formula (dyadic GELU cases and every randn case); the GELU bound on exact
    pre-activations rejects erf-GELU and a GELU constant of 0.0447; what the randn GELU bound can and cannot reject is stated;
  * the launcher's tile rule returns the form the tables expect; the hooks refuse bad arguments without a device."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv1_cases as K
import train_op_ref as R
from teramind_amd import _lib

INT_SE = sorted({(s, e) for s, e, _ in K.int_cases()})
GELU_SE = sorted({(s, e) for s, e, _ in K.gelu_cases()})
FLOAT_SE = sorted({(s, e) for s, e, _ in K.float_cases()})


def _id(se):
    return "-".join(map(str, se[0])) + "-" + se[1]


def _torch_model(c):
    """conv3d + F.gelu + repeat_interleave, float64, from the case's tensors."""
    out = F.conv3d(c["x"], c["w"][:, :, None, None, None], c["b"])
    if c["gelu"]:
        out = F.gelu(out, approximate="tanh")
    if c["gate"] is not None:
        g = c["gate"]
        if c["gate_half"]:
            g = F.interpolate(g.flatten(0, 1), scale_factor=2, mode="nearest").reshape(*g.shape[:3], *out.shape[-2:])
        out = out * g
    return c["res"] + out if c["res"] is not None else out


@pytest.mark.parametrize("kind,se", [("int", se) for se in INT_SE + GELU_SE] + [("float", se) for se in FLOAT_SE],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_reference_matches_torch(kind, se):
    c = K.make(se[0], se[1], kind)
    ref, tm = K.ref_of(c), _torch_model(c)
    if kind == "int" and not c["gelu"]:
        assert torch.equal(ref, tm)                       # integers: both exact
    else:
        assert torch.allclose(ref, tm, rtol=1e-13, atol=1e-13)
    # the slices are what they claim to be
    assert torch.equal(c["x"], c["xw"][:, c["x_c0"]:c["x_c0"] + se[0][1]])
    assert float(c["xw"][:, c["x_c0"] + se[0][1]:(c["x_cb0"] + K.cb(se[0][1])) * 8].abs().sum()) == 0.0


def test_integer_data_is_exact_in_fp32():
    for s in K.SHAPES + [a[0] for a in K.AUTO_CASES]:
        assert K.worst_abs_sum(s[1]) < 2 ** 24
    for se in GELU_SE:
        pre = K.preact(K.make(se[0], se[1], "int"))
        assert torch.equal(pre, pre.float().double()) and float(pre.abs().max()) <= 7.0
        assert torch.equal(pre * 8, (pre * 8).round())


@pytest.mark.parametrize("se", INT_SE + GELU_SE, ids=_id)
def test_every_applicable_wrong_variant_is_caught(se):
    """Applicability is conv1_cases.applies: gate errors need a gate (gate_clip a half-resolution one at S >= 4, gate_z0 Z > 1,
    the chunk errors a gate that is a chunk of a wider tensor), x_block_off a sliced x, gelu_after_gate GELU with a gate,
    res_times_gate a gate and a residual, erf_gelu GELU, swap_g4 more than 32 couts, swap_halves128 the 128-cout form;
    no_bias applies everywhere.  Integer cases: any difference is caught (torch.equal).  GELU cases: past the bound."""
    shape, epi = se
    c = K.make(shape, epi, "int")
    ref = K.ref_of(c)
    bnd = K.bound(c, True)
    exact = not c["gelu"]
    forms = {K.conv1_form(K.vox_of(shape[0], shape[3], shape[4]), K.ntile_of(shape[2]), v) for v in K.variants_of(shape)}
    seen = 0
    for e in K.WRONG:
        if not any(K.applies(e, epi, shape, f) for f in forms):
            continue
        seen += 1
        bad = K.reference(c["x"], c["w"], c["b"], c["res"], c["gate"], c["gate_half"], c["gelu"], wrong=e, wide=c)
        d = (bad - ref).abs()
        if exact:
            assert bool((d > 0).any()), f"{e}: the data of {_id(se)} cannot tell it from the right model"
        else:
            assert bool((d > bnd).any()), f"{e}: inside the bound of {_id(se)} everywhere"
    assert seen >= 2                                     # no_bias and swap_g4 at the least (every Cout here is > 32)


def test_every_wrong_variant_applies_somewhere():
    cases = K.int_cases() + K.gelu_cases()
    for e in K.WRONG:
        n = sum(K.applies(e, ep, s, K.conv1_form(K.vox_of(s[0], s[3], s[4]), K.ntile_of(s[2]), v)) for s, ep, v in cases)
        assert n >= 2, e


def _kid(v):
    return v if isinstance(v, str) else _id(v)


@pytest.mark.parametrize("kind,se", [("int", se) for se in GELU_SE] + [("float", se) for se in FLOAT_SE], ids=_kid)
def test_bounds_hold_for_a_float32_evaluation(kind, se):
    """Not too tight: the dyadic GELU cases (exact pre-activation) and every randn case, those under GELU included (there the
    error of the pre-activation passes through GELU_SLOPE)."""
    c = K.make(se[0], se[1], kind)
    assert (kind == "int") == bool(torch.equal(c["x"] * 8, (c["x"] * 8).round()))      # the family the id names
    ref, bnd = K.ref_of(c), K.bound(c, kind == "int")
    d = (K.emulate_f32(c).double() - ref).abs()
    assert bool((d <= bnd).all()), f"worst |d| / bound = {float((d / bnd.clamp_min(1e-300)).max()):.3g}"


def _gelu_variants(c):
    g = c["gate"] if c["gate"] is not None else 1.0
    r = c["res"] if c["res"] is not None else 0.0
    pre = K.preact(c)
    return {"erf": r + g * K.gelu_erf(pre), "0.0447": r + g * K.gelu_tanh_k(pre, 0.0447)}


@pytest.mark.parametrize("se", GELU_SE, ids=_id)
def test_gelu_bound_rejects_erf_gelu_and_a_shortened_constant(se):
    """Not too loose, on the dyadic GELU cases (exact pre-activation: the bound is that of gelu_tanh_hw alone, a few U to 250 U
    relative): erf-GELU and tanh-GELU with 0.0447 for 0.044715 lie outside it, the worst element by more than 20 bounds."""
    c = K.make(se[0], se[1], "int")
    ref, bnd = K.ref_of(c), K.bound(c, True)
    for name, bad in _gelu_variants(c).items():
        d = (bad - ref).abs()
        assert bool((d > bnd).any()), name
        worst = float((d / bnd.clamp_min(1e-300)).max())
        assert worst > 20, (name, worst)


@pytest.mark.parametrize("se", [se for se in FLOAT_SE if K.EPILOGUES[se[1]][0]], ids=_id)
def test_what_the_randn_gelu_bound_can_reject(se):
    """On randn data the bound carries the summation error of the pre-activation, (Kp + 2) U (sum |w x| + |b|) times
    GELU_SLOPE, which grows with Cin; a GELU whose curve is off by up to 5e-4 (erf-GELU) or 5e-6 (0.0447) is then only
    separated where that term is small.  Asserted here: erf-GELU lies outside at every randn GELU shape (Cin 13, 40, 229: the
    worst element at 146, 48 and 3.6 bounds); the shortened constant lies outside at Cin 13 (Kp = 16: 3.9 bounds) and INSIDE at
    Cin 229 (Kp = 232: 0.07 bounds) -- the dyadic cases above are what pins the constant, in all three tile forms."""
    c = K.make(se[0], se[1], "float")
    assert not torch.equal(c["x"] * 8, (c["x"] * 8).round())
    ref, bnd = K.ref_of(c), K.bound(c, False)
    worst = {n: float(((bad - ref).abs() / bnd.clamp_min(1e-300)).max()) for n, bad in _gelu_variants(c).items()}
    assert worst["erf"] > 1, worst
    if se[0][1] == 13:
        assert worst["0.0447"] > 1, worst
    if se[0][1] == 229:
        assert worst["0.0447"] < 1, worst


def test_gelu_bound_covers_the_step_by_step_float32_gelu_on_a_dense_grid():
    x = torch.cat([torch.linspace(-12, 12, 200001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 2.0 ** -126])]).float()
    d = (K.gelu_hw_f32(x).double() - R.gelu_tanh(x.double())).abs()
    assert bool((d <= K.gelu_hw_bound(x)).all())
    assert float(K.gelu_hw_bound(torch.tensor([7.0]))) < 7 * 40 * K.U        # a few tens of U relative, no more


# ---------------------------------------------------------------------------------------------------------- the tile rule
def test_tile_rule_of_the_launcher():
    L = _lib.lib()
    every = K.int_cases() + K.gelu_cases() + K.float_cases()
    got = set()
    for s, _, v in every:
        vox, nt = K.vox_of(s[0], s[3], s[4]), K.ntile_of(s[2])
        want = K.conv1_form(vox, nt, v)
        assert want == v                                 # small launches: a forced 2 stays under the 512 threshold
        assert L.tm_conv1_form(vox, nt, v) == want, (s, v)
        got.add(want)
    assert got == {1, 2, 3}
    for s, form in K.AUTO_CASES:
        vox, nt = K.vox_of(s[0], s[3], s[4]), K.ntile_of(s[2])
        assert L.tm_conv1_form(vox, nt, 0) == form == K.conv1_form(vox, nt, 0), s
    assert [f for _, f in K.AUTO_CASES] == [3, 2, 2, 2, 1]
    # exactly at and just under the two thresholds
    assert L.tm_conv1_form(8192, 32, 0) == 3 and L.tm_conv1_form(8192 - 1, 32, 0) == 2
    assert L.tm_conv1_form(8192, 16, 0) == 2 and L.tm_conv1_form(8192 - 1, 16, 0) == 1
    # forced forms
    assert L.tm_conv1_form(75, 2, 3) == 3 and L.tm_conv1_form(75, 2, 2) == 2 and L.tm_conv1_form(1 << 20, 32, 1) == 1
    assert L.tm_conv1_form(1 << 20, 32, 2) == 3          # 2 keeps the size rule for the cout tile
    for nt in (1, 3, 31):
        assert L.tm_conv1_form(1 << 20, nt, 3) == 0      # 128-cout tile on an odd tile count: refused
    # the grids the tables reach (xcd_swizzle: below 8 workgroups, and no multiple of 8)
    grids = {K.grid_of(K.vox_of(s[0], s[3], s[4]), K.ntile_of(s[2]), K.conv1_form(K.vox_of(s[0], s[3], s[4]), K.ntile_of(s[2]), v))
             for s, _, v in every}
    assert min(grids) == 1 and any(g < 8 for g in grids) and any(g > 8 and g % 8 for g in grids)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_hook_refusals_need_no_device():
    """TM_ERR_ARG (-1) before any device call: the pointers are never dereferenced."""
    L = _lib.lib()
    buf = torch.zeros(8)
    p = _lib.ptr(buf)
    form = C.c_int(-7)

    def f32(x_cbtot=2, x_cb0=0, g_cbtot=9, g_cb0=0, half=0, tv=0, gate=p, S=8, Cout=72):
        # args: x w b y res gate | x_cbtot x_cb0 gate_cbtot gate_cb0 gate_half gelu tile_variant | N Cin Cout Z S | form stream
        return L.tm_op_conv1_f32(p, p, p, p, None, gate, x_cbtot, x_cb0, g_cbtot, g_cb0, half, 0, tv, 1, 13, Cout, 2, S,
                                 C.byref(form), None)

    for kw, word in [(dict(x_cbtot=1), b"x slice"), (dict(x_cb0=1), b"x slice"), (dict(x_cb0=-1), b"x slice"),
                     (dict(g_cbtot=8), b"gate slice"), (dict(g_cbtot=63, g_cb0=55), b"gate slice"), (dict(g_cb0=-1), b"gate slice"),
                     (dict(half=1, gate=None), b"gate_half"), (dict(half=1, S=6), b"power of two"), (dict(half=1, S=1), b"power of two"),
                     (dict(half=1, S=12), b"power of two"), (dict(tv=4), b"tile_variant"), (dict(tv=-1), b"tile_variant"),
                     (dict(tv=3, Cout=37, g_cbtot=5), b"even"), (dict(tv=3, Cout=129, g_cbtot=17), b"even")]:
        assert f32(**kw) == -1 and word in L.tm_last_error(), (kw, L.tm_last_error())
    assert form.value == -7                              # untouched by a refused call
    assert L.tm_op_conv1_f32(p, None, p, p, None, None, 2, 0, 0, 0, 0, 0, 0, 1, 13, 72, 2, 8, None, None) == -1

    def h16(half=0, g_cbtot=9, g_cb0=0, gate=p, S=8, dtype=1, waves=4):
        # args: x w b y | N Cin Cout Z S gelu dtype waves | res_h16 gate_h16 y_h16 | gate_half gate_cbtot gate_cb0 | stream
        return L.tm_op_conv1_h16_gate(p, p, p, p, 1, 13, 72, 2, S, 0, dtype, waves, None, gate, None, half, g_cbtot, g_cb0, None)

    for kw, word in [(dict(half=1, gate=None), b"gate_half"), (dict(half=1, S=6), b"power of two"), (dict(half=1, S=1), b"power of two"),
                     (dict(g_cbtot=8), b"gate slice"), (dict(g_cbtot=63, g_cb0=55), b"gate slice"), (dict(g_cb0=-2), b"gate slice"),
                     (dict(dtype=0), b"dtype"), (dict(waves=5), b"waves")]:
        assert h16(**kw) == -1 and word in L.tm_last_error(), (kw, L.tm_last_error())
