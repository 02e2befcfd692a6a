"""-m gpu: the fp32 1x1x1 conv / Linear kernel conv1_mfma (every fp32 nn.Linear of the AttnBlocks, the ResBlock skip conv, the
1x1 data gradient) on its own, through tm_op_conv1_f32, in every form the model launches: the three instantiations (128 x 64,
256 x 64 and 256 x 128 voxels x couts per workgroup), the epilogues of attn_block (plain, tanh-GELU, gate + residual, the
in-place update x <- x + gate * Linear(.), the gate at half resolution), x and the gate as channel-block slices of wider
tensors, Z = 1, 2, 4, 8.  Model, data, bounds and tables: tests/conv1_cases.py (checked on the host by
tests/test_conv1_cases_host.py: every deliberate error there is caught by these cases' data).

Rules of every case:
  * integer data: torch.equal against the float64 model (no tolerance); dyadic data under GELU and randn data: inside the
    bound derived in conv1_cases (never from the kernel's output);
  * the output starts as NaN (in place: as the residual): an element the kernel skips fails; the pad slots of the last cout
    block end as exactly 0; y sits between two guard blocks of a sentinel value, which must survive, as must every input;
  * the channel blocks of x and of the gate OUTSIDE the slice the conv is given are NaN: a read outside poisons the output;
  * form_out must name the instantiation the tables expect.
The 16-bit 1x1 conv takes the half-resolution gate as a chunk of a wider tensor through tm_op_conv1_h16_gate, bit for bit."""
import ctypes as C
import functools
import os
import time

import pytest
import torch

import conv1_cases as K
import util
from teramind_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 12345.0
CASE_SECONDS = 5.0            # every case, its float64 model and all its fences included, stays well under this

STATS = {"cases": 0, "t0": None, "slowest": (0.0, ""), "ratio": {}, "forms": set()}


@pytest.fixture(scope="module", autouse=True)
def _record(out_dir):
    """The figures of profiles/conv1_f32_tests.txt, written next to the other GPU run products."""
    STATS["t0"] = time.time()
    yield
    with open(os.path.join(out_dir, "conv1_f32_tests.txt"), "w") as f:
        f.write(f"cases {STATS['cases']}  wall {time.time() - STATS['t0']:.1f} s  forms launched {sorted(STATS['forms'])}\n")
        f.write(f"slowest case {STATS['slowest'][0]:.2f} s  {STATS['slowest'][1]}\n")
        for fam, (r, cid) in sorted(STATS["ratio"].items()):
            f.write(f"worst |d| / bound  {fam:28s} {r:.3f}  {cid}\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cb8_dev(t, C_pad=None, keep=None):
    """float64 NCDHW -> fp32 CB8 on the device; channels padded with zeros to C_pad; keep = (cb0, ncb): every other block NaN."""
    if C_pad is not None and t.shape[1] < C_pad:
        t = torch.cat([t, torch.zeros(t.shape[0], C_pad - t.shape[1], *t.shape[2:], dtype=t.dtype)], 1)
    o = K.to_cb8(t.float())
    if keep is not None:
        o[:, :keep[0]] = NAN
        o[:, keep[0] + keep[1]:] = NAN
    return o.to(DEV)


@functools.lru_cache(maxsize=2)
def _ref(shape, epi, kind):
    """(float64 model, bound) of a case, shared by its tile variants."""
    c = K.make(shape, epi, kind)
    exact = kind == "int" and not c["gelu"]
    return K.ref_of(c), (None if exact else K.bound(c, kind == "int"))


def run(c, variant):
    """One launch through tm_op_conv1_f32 with all the fences up.  Returns (float64 NCDHW output on the CPU, form)."""
    N, Cin, Cout, Z, S = c["shape"]
    Cbi, Cob = K.cb(Cin), K.cb(Cout)
    x = _cb8_dev(c["xw"], keep=(c["x_cb0"], Cbi))
    gate = _cb8_dev(c["gw"], keep=(c["g_cb0"], Cob)) if c["gate"] is not None else None
    res = _cb8_dev(c["res"], Cob * 8) if c["res"] is not None else None
    buf = torch.full((N * Cob + 2, Z, S, S, 8), NAN, dtype=torch.float32, device=DEV)
    buf[0] = SENTINEL
    buf[-1] = SENTINEL
    y = buf[1:-1].view(N, Cob, Z, S, S, 8)
    assert y.data_ptr() == buf.data_ptr() + 4 * Z * S * S * 8
    if c["in_place"]:
        y.copy_(res)
    x0, g0, r0 = x.clone(), (gate.clone() if gate is not None else None), (res.clone() if res is not None else None)
    rp = y if c["in_place"] else res
    wh, bh = c["w"].float().contiguous(), c["b"].float().contiguous()
    form = C.c_int(-1)
    _lib.check(_lib.lib().tm_op_conv1_f32(_lib.ptr(x), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(y), _lib.ptr(rp),
                                          _lib.ptr(gate), c["x_cbtot"], c["x_cb0"], c["g_cbtot"], c["g_cb0"], int(c["gate_half"]),
                                          int(c["gelu"]), variant, N, Cin, Cout, Z, S, C.byref(form), _lib.current_stream_ptr()),
               "tm_op_conv1_f32")
    torch.cuda.synchronize()
    assert torch.equal(buf[0], torch.full_like(buf[0], SENTINEL)) and torch.equal(buf[-1], torch.full_like(buf[-1], SENTINEL)), \
        "a guard block next to y was written"
    assert torch.equal(_bits(x), _bits(x0)), "x was written"
    assert gate is None or torch.equal(_bits(gate), _bits(g0)), "the gate was written"
    assert res is None or torch.equal(_bits(res), _bits(r0)), "the residual was written"
    assert not torch.isnan(y).any(), f"{int(torch.isnan(y).sum())} elements of y are NaN: not written, or computed from outside a slice"
    if Cout % 8:
        assert float(y[:, -1, ..., Cout % 8:].abs().max()) == 0.0, "pad slots of the last cout block are not zero"
    return K.from_cb8(y.cpu())[:, :Cout].double(), form.value


def _case(case, kind, family=None):
    shape, epi, variant = case
    t0 = time.time()
    c = K.make(shape, epi, kind)
    ref, bnd = _ref(shape, epi, kind)
    got, form = run(c, variant)
    want_form = K.conv1_form(K.vox_of(shape[0], shape[3], shape[4]), K.ntile_of(shape[2]), variant)
    assert form == want_form, f"launched form {form}, expected {want_form}"
    STATS["forms"].add(form)
    d = (got - ref).abs()
    cid = K.case_id(case)
    if bnd is None:
        print(f"conv1_f32 {cid}: form {form}, max|d| = {float(d.max()):.3e} (exact case)")
        assert torch.equal(got, ref), util.report("conv1_f32 " + cid, got, ref)
    else:
        ratio = float((d / bnd.clamp_min(1e-300)).max())
        print(f"conv1_f32 {cid}: form {form}, max|d| = {float(d.max()):.3e}, worst |d| / bound = {ratio:.3f}")
        if family:
            key = f"{family} {epi}"
            if ratio > STATS["ratio"].get(key, (0.0, ""))[0]:
                STATS["ratio"][key] = (ratio, cid)
        assert bool((d <= bnd).all()), f"conv1_f32 {cid}: max|d| = {float(d.max()):.3e}, worst |d| / bound = {ratio:.3g}"
    STATS["cases"] += 1
    dt = time.time() - t0
    if dt > STATS["slowest"][0]:
        STATS["slowest"] = (dt, cid)
    assert dt < CASE_SECONDS, f"conv1_f32 {cid} took {dt:.1f} s"


@pytest.mark.parametrize("case", K.int_cases(), ids=K.case_id)
def test_conv1_f32_exact_integers(case):
    _case(case, "int")


@pytest.mark.parametrize("case", K.gelu_cases(), ids=K.case_id)
def test_conv1_f32_gelu_on_exact_preactivations(case):
    """x in multiples of 1/8 and one nonzero input channel: W x + b is an exact dyadic in [-7, 7], so the whole error is that
    of gelu_tanh_hw (two rounded constants, x * x, the fma, the product, v_exp_f32 and v_rcp_f32 at 1 ulp, 1 + e, the final
    product): conv1_cases.gelu_hw_bound, a few tens of U relative."""
    _case(case, "int", "gelu-dyadic")


@pytest.mark.parametrize("case", K.float_cases(), ids=K.case_id)
def test_conv1_f32_float(case):
    """randn data: (Kp + 2) U (sum |w x| + |b|) on the linear part, scaled by |gate|, plus 2 U (|res| + |out|)."""
    _case(case, "float", "float")


@pytest.mark.parametrize("shape,form", K.AUTO_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else f"form{v}")
def test_conv1_f32_automatic_tile_choice(shape, form):
    """tile_variant 0 at the boundaries of the launcher's rule (8192 voxels = 32 tiles of 256): the 128-cout tile exactly at
    512 workgroups, an odd tile count, 480 workgroups, and the two sides of the 128- / 256-voxel threshold."""
    t0 = time.time()
    c = K.make(shape, "plain", "int")
    got, launched = run(c, 0)
    assert launched == form
    STATS["forms"].add(launched)
    STATS["cases"] += 1
    assert torch.equal(got, K.ref_of(c)), util.report("conv1_f32 auto", got, K.ref_of(c))
    assert time.time() - t0 < CASE_SECONDS


def test_conv1_f32_automatic_choice_with_the_half_gate_in_place():
    """The model's proj / fc2 launch at the size where the automatic choice is the 128-cout tile: S = 64, gate at 32 x 32."""
    shape = K.AUTO_CASES[0][0]
    t0 = time.time()
    c = K.make(shape, "gatehalf_chunk2", "int")
    got, launched = run(c, 0)
    assert launched == 3
    STATS["cases"] += 1
    assert torch.equal(got, K.ref_of(c)), util.report("conv1_f32 auto half gate", got, K.ref_of(c))
    assert time.time() - t0 < CASE_SECONDS


def test_conv1_f32_form_out_names_all_three_instantiations():
    c = K.make((3, 13, 72, 1, 5), "plain", "int")
    assert [run(c, v)[1] for v in (1, 2, 3)] == [1, 2, 3]


# ------------------------------------------------------------------------------------------------------------ 16-bit twin
@pytest.mark.parametrize("N,Cin,Cout,Z,S", K.H16_GATE_CASES)
@pytest.mark.parametrize("out16", [True, False])
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_conv1_16bit_gate_at_half_resolution_as_a_chunk(N, Cin, Cout, Z, S, out16, waves, dtype):
    """test_conv1_16bit_stream_epilogue's recipe (x <- x + gate * Linear(.), 16-bit gate and residual) with the gate at S / 2 and
    as chunk 2 of a tensor 7 chunks wide (the other chunks NaN), through tm_op_conv1_h16_gate: out16 = the gated stream
    epilogue (16-bit output), otherwise the generic one (fp32 output).  Bit-equal to the float64 model rounded to the type."""
    code, td = util.H16[dtype]
    g = torch.Generator().manual_seed(90 + Z + S)
    ri = lambda shp, r: torch.randint(-r, r + 1, shp, generator=g).double()
    Cob = K.cb(Cout)
    x, w, b = ri((N, Cin, Z, S, S), 3), ri((Cout, Cin), 2), ri((Cout,), 4)
    res = ri((N, Cout, Z, S, S), 100)
    gw = ri((N, 7 * Cob * 8, Z, S // 2, S // 2), 2)
    g_c0 = 2 * Cob * 8
    gw[:, g_c0 + Cout:g_c0 + Cob * 8] = 0
    gate = gw[:, g_c0:g_c0 + Cout]
    ref = K.reference(x, w, b, res, gate, True, False)
    ref = ref.to(td).double() if out16 else ref
    bad = K.reference(x, w, b, res, gate, True, False, wrong="gate_clip")
    assert not torch.equal(bad, K.reference(x, w, b, res, gate, True, False))
    xc = _cb8_dev(x, K.cb(Cin) * 8)
    gh = _cb8_dev(gw, keep=(2 * Cob, Cob)).to(td)
    rh = _cb8_dev(res, Cob * 8).to(td)
    shp = (N, Cob, Z, S, S, 8)
    yc = torch.full(shp, NAN, dtype=torch.float32, device=DEV) if not out16 else None
    yh = torch.full(shp, NAN, dtype=td, device=DEV) if out16 else None
    wh, bh = w.float().contiguous(), b.float().contiguous()
    _lib.check(_lib.lib().tm_op_conv1_h16_gate(_lib.ptr(xc), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()), _lib.ptr(yc),
                                               N, Cin, Cout, Z, S, 0, code, waves, _lib.ptr(rh), _lib.ptr(gh), _lib.ptr(yh),
                                               1, 7 * Cob, 2 * Cob, _lib.current_stream_ptr()), "tm_op_conv1_h16_gate")
    y = (yh if out16 else yc).float()
    assert not torch.isnan(y).any(), f"{int(torch.isnan(y).sum())} NaN elements: not written, or read outside the gate's chunk"
    if Cout % 8:
        assert float(y[:, -1, ..., Cout % 8:].abs().max()) == 0.0, "pad slots of the last cout block are not zero"
    got = K.from_cb8(y.cpu())[:, :Cout].double()
    assert torch.equal(got, ref), util.report(f"conv1 {dtype} half gate", got, ref)
