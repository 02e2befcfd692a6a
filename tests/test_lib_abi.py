"""CPU: the C-ABI library loads (no GPU needed for dlopen) and exports every function that
include/teramind_hip.h declares; argument validation paths that never touch the device."""
import ctypes as C
import os
import re

import pytest

import util
from teramind_amd import _lib


def header_functions():
    src = open(os.path.join(util.ROOT, "include", "teramind_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in teramind_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "ctypes signature table out of sync with the header"
    assert L.tm_version() == 1


def test_error_paths_without_device():
    L = _lib.lib()
    cfg = _lib.TmConfig()
    cfg.patch_size, cfg.rna_slc, cfg.n_stain, cfg.rna_num, cfg.net_ch = 48, 4, 2, 229, 64
    cfg.embed_ch, cfg.attn_res, cfg.num_res_blocks = 512, 16, 2
    for i, v in enumerate((1, 2, 4, 8)):
        cfg.ch_mult[i] = v
    h = C.c_void_p(0)
    assert L.tm_model_create(C.byref(cfg), C.byref(h)) == -1           # TM_ERR_ARG: unsupported patch size
    assert b"patch_size" in L.tm_last_error()
    cfg.patch_size = 64
    assert L.tm_model_create(C.byref(cfg), C.byref(h)) == 0
    assert L.tm_model_num_params(h) == 399
    assert L.tm_model_param_key(h, 0) == b"time_embed.time_embed.0.weight"
    shp = (C.c_int64 * 2)(3, 3)
    buf = (C.c_float * 9)()
    assert L.tm_model_load_param(h, b"no.such.key", buf, shp, 2, 0) == -3      # TM_ERR_KEY
    assert L.tm_model_load_param(h, b"time_embed.time_embed.0.weight", buf, shp, 2, 0) == -3   # shape mismatch
    assert L.tm_model_finalize(h) == -3                                          # strict: missing keys
    assert b"missing key" in L.tm_last_error()
    assert L.tm_workspace_bytes(h, 1, 2, 2, 0) == 0                              # not finalized
    assert L.tm_model_destroy(h) == 0


def test_op_argument_checks_without_device():
    """The single-operator hooks reject bad arguments (TM_ERR_ARG = -1) before their first HIP call."""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ms = C.c_float(0)
    # row op 1 keeps 4 * D floats of dynamic LDS per workgroup: D <= 4096
    assert L.tm_op_rows(1, p, p, p, p, p, 4, 4097, None) == -1
    assert b"4096" in L.tm_last_error() and b"LDS" in L.tm_last_error()
    # conv27 timing hook: waves 0, 4, 8 or 9 (args: N Cin Cout S dtype waves ups with_res fused iters)
    assert L.tm_op_conv27_time(1, 64, 64, 16, 1, 5, 0, 0, 0, 1, C.byref(ms), None) == -1
    assert b"waves" in L.tm_last_error()
    # 16-bit conv27 without weights
    assert L.tm_op_conv27_bf16(p, None, p, p, 1, 64, 64, 16, 1, 0, None, None, 0, 0, None) == -1
    assert b"null" in L.tm_last_error()
    # the Z-taking twins: 1 <= Z <= 8; the upsampled-input form and the half-resolution residual are Z == 2 only
    # (args: x w b y N Cin Cout S dtype waves res_h16 y_h16 ups res_half Z)
    assert L.tm_op_conv27_h16_z(p, p, p, p, 1, 64, 128, 16, 1, 0, None, None, 0, 0, 0, None) == -1
    assert b"Z must be" in L.tm_last_error()
    assert L.tm_op_conv27_h16_z(p, p, p, p, 1, 64, 128, 16, 1, 0, None, None, 0, 0, 9, None) == -1
    assert b"Z must be" in L.tm_last_error()
    assert L.tm_op_conv27_fused_z(p, p, p, p, p, p, p, 1, 64, 128, 16, 1, 1, 0, 9, None) == -1
    assert b"Z must be" in L.tm_last_error()
    assert L.tm_op_conv27_h16_z(p, p, p, p, 1, 64, 128, 16, 1, 0, None, None, 1, 0, 4, None) == -1
    assert b"ups" in L.tm_last_error() and b"Z == 2" in L.tm_last_error()
    assert L.tm_op_conv27_h16_z(p, p, p, None, 1, 64, 128, 16, 1, 0, p, p, 0, 1, 1, None) == -1
    assert b"res_half" in L.tm_last_error() and b"Z == 2" in L.tm_last_error()
    # training attention core: Z = 2, S = 6 is a window of 18 tokens
    assert L.tm_op_window_attn_train(p, p, p, p, p, None, p, None, None, None, None, None, 1, 64, 2, 6, None) == -1
    assert b"18 tokens" in L.tm_last_error()
    # gene-gene attention hooks (args: rna w_host[12] gidx B gn zs G form zlo zhi out_tok attn_map): D = gn^2 zs <= 512, G <= 512,
    # the fused form is D = 64 with G <= 232; one output is required; the read-out is rna_slc = 4 with 1 <= K <= 8
    wh = (C.c_void_p * 12)(*[p.value] * 12)
    gl = (C.c_int * 2)(0, 1)
    assert L.tm_op_gene_attn(p, wh, None, 1, 8, 16, 229, 0, 0, 16, p, p, None) == -1
    assert b"D = gn^2 * zs = 1024 > 512" in L.tm_last_error()
    assert L.tm_op_gene_attn(p, wh, None, 1, 4, 4, 233, 1, 0, 4, p, p, None) == -1
    assert b"G = 233 > 232" in L.tm_last_error()
    assert L.tm_op_gene_attn(p, wh, None, 1, 4, 8, 229, 1, 0, 8, p, p, None) == -1
    assert b"!= D = 64" in L.tm_last_error()
    assert L.tm_op_gene_attn(p, wh, None, 1, 4, 4, 229, 0, 0, 4, None, None, None) == -1
    assert b"null" in L.tm_last_error()
    assert L.tm_op_gene_attn(p, None, None, 1, 4, 4, 229, 0, 0, 4, p, p, None) == -1
    assert b"null" in L.tm_last_error()
    assert L.tm_op_rna_mid(p, 1, 4, 4, 229, None, None) == -1
    assert b"null" in L.tm_last_error()
    assert L.tm_op_gene_readout(p, wh, None, 1, 4, 4, 229, gl, 9, 0, p, None, None) == -1
    assert b"outside [1, 8]" in L.tm_last_error()
    assert L.tm_op_gene_readout(p, wh, None, 1, 4, 8, 229, gl, 2, 0, p, None, None) == -1
    assert b"rna_slc = 4" in L.tm_last_error()
    assert L.tm_op_gene_readout(p, wh, None, 1, 4, 4, 229, gl, 2, 0, None, None, None) == -1
    assert b"null" in L.tm_last_error()
    # prep backward: scale without shift
    assert L.tm_op_prep_bwd(p, p, p, p, None, None, C.c_float(1.0), 1, p, p, p, p, 1, 8, 2, 4, None) == -1
    assert b"scale without shift" in L.tm_last_error()


def test_product_path_has_no_cpu_fallback():
    import torch
    from teramind_amd.config import PathConfig
    from teramind_amd.unet import BeatGANsUNetModel
    with pytest.raises(RuntimeError):
        BeatGANsUNetModel(PathConfig(), "cpu")
    # nothing under the package imports the oracle
    pkg = os.path.join(util.ROOT, "tera-mind_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, f)).read().replace("CPU oracle", ""), f
