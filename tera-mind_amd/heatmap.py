"""Attention heat maps: a slice of the gene-gene attention mosaic -> smoothed scalar field -> colour bytes, on the GPU.

Restates what the reference draws its figures from (test_attn.py:145-250, `gen_img`): sum the read-out channels of a group,
`log2(v * wei + 1)`, mask by where every pathway gene is expressed, `scipy.ndimage.gaussian_filter(sigma=2)`, paint through
`cm.inferno` or a two-colour palette per gene.  `field` is tm_heat_field, `render` is tm_heat_render (the definitions are in
include/teramind_hip.h); stitch.save_attn_heatmaps_pyramid writes the result as a tiled pyramid.

The reference halves the mosaic with torchvision's resize before it draws, to fit its figure size; that is layout and is not
restated: the field is computed at the mosaic's own resolution.  Not pinned either: the reference's rendered JPEGs
(matplotlib rasterises a figure), the 3-D surface and joint plots of draw_attplot, colour bars.
"""
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

SCALES = (1, 2, 4, 8, 16)
MODES = ("att_all", "att_up", "att_dn", "expr")

# utils/__init__.py:93-95 (`CM`): the end colour of each gene's two-colour palette, per pathway (attn_maps.PATHWAYS has the genes)
PATHWAY_COLOURS = {"GLUT": ((0, 1, 0.82), (0.69, 1, 0), (0.89, 0, 1)),
                   "DOPA": ((1, 0, 0.4), (1, 0.4, 0), (1, 1, 0.4)),
                   "BLOD": ((1, 0.43, 1), (1, 0.2, 0.49))}
# test_attn.py:173-176 (`vextr`): the upper end of each colour scale
PATHWAY_VMAX = {"GLUT": {"att_updn": (2, 4), "att_all": 2, "expr": (1, 3)},
                "DOPA": {"att_updn": (2, 4), "att_all": 2, "expr": (1, 1)},
                "BLOD": {"att_updn": (2, 4), "att_all": 2, "expr": (1, 1)}}


def gene_weight(rna_num: int) -> int:
    """`wei` of test_attn.py:190: 229 for the 229-gene panel (mouse 638850), 500 otherwise."""
    return 229 if int(rna_num) == 229 else 500


def gaussian_taps(sigma: float, truncate: float = 4.0) -> Tuple[int, np.ndarray]:
    """(r, taps): scipy.ndimage's Gaussian, r = int(truncate * sigma + 0.5), exp(-x^2 / (2 sigma^2)) normalised in float64,
    cast to float32 once.  sigma = 0 gives (0, [1])."""
    sigma = float(sigma)
    if not sigma >= 0:
        raise ValueError(f"sigma must be >= 0, got {sigma}")
    r = int(float(truncate) * sigma + 0.5)
    if r == 0 or sigma == 0:
        return 0, np.ones(1, dtype=np.float32)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return r, (w / w.sum()).astype(np.float32)


def two_colour(end: Sequence[float], n: int = 100, start: Sequence[float] = (0, 0, 0)) -> np.ndarray:
    """uint8 [n, 3]: row j = trunc((start + (end - start) * j / (n - 1)) * 255), the bytes of
    LinearSegmentedColormap.from_list("Custom", [start, end], N=n) (test_attn.py:136-142, `cm_platte`).  Truncation, not
    rounding."""
    st, ed = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    if not 2 <= int(n) <= 256 or st.shape != (3,) or ed.shape != (3,):
        raise ValueError("two_colour takes two RGB triples in 0 .. 1 and 2 <= n <= 256")
    j = np.arange(int(n), dtype=np.float64)[:, None] / (int(n) - 1)
    return np.clip((st + (ed - st) * j) * 255, 0, 255).astype(np.uint8)


def mode_ranges(K: int, mode: str, gene: Optional[int] = None) -> Tuple[int, int, int, int]:
    """(sum0, nsum, mask0, nmask) of `mode` in the [4K] channels of a read-out slice: K maps to the partner above, K to the
    one below, K ensemble maps, K expression planes (attn_maps.pathway_readout)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {', '.join(MODES)}, got {mode!r}")
    if mode == "expr":
        if gene is None or not 0 <= int(gene) < K:
            raise ValueError(f"mode 'expr' takes gene = 0 .. {K - 1}, got {gene}")
        return 3 * K + int(gene), 1, 0, 0                        # test_attn.py:228-229: no mask
    sum0 = {"att_up": 0, "att_dn": K, "att_all": 2 * K}[mode]    # test_attn.py:253-258, 204-206
    return sum0, K, 3 * K, K


def field(mosaic_slice, K: int, mode: str = "att_all", wei: float = 229, sigma: float = 2.0, gene: Optional[int] = None,
          truncate: float = 4.0) -> torch.Tensor:
    """The smoothed field of one slice, float32 device [H, W], at the mosaic's own resolution (the reference's pre-halving
    is layout and is not restated).  mosaic_slice: float16 [4K, H, W], a device tensor (views are read in place through
    their strides as long as columns are unit-stride) or a numpy array (uploaded).  Modes: att_all sums [2K, 3K), att_up
    [0, K), att_dn [K, 2K), all masked by every channel of [3K, 4K) being non-zero; expr takes channel 3K + gene with
    wei = 1 and no mask."""
    if isinstance(mosaic_slice, np.ndarray):
        mosaic_slice = torch.from_numpy(np.ascontiguousarray(mosaic_slice)).cuda()
    t = mosaic_slice
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.dim() == 3):
        raise ValueError("a heat-map field takes a float16 [4K, H, W] device tensor or numpy array")
    if t.shape[0] != 4 * K:
        raise ValueError(f"{t.shape[0]} channels are not 4 K = {4 * K}")
    if t.stride(2) != 1:
        t = t.contiguous()
    sum0, nsum, mask0, nmask = mode_ranges(K, mode, gene)
    r, taps = gaussian_taps(sigma, truncate)
    Cn, H, W = t.shape
    dst = torch.empty((H, W), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().tm_heat_field(C.c_void_p(t.data_ptr()), Cn, H, W, t.stride(1), t.stride(0), sum0, nsum,
                                            1.0 if mode == "expr" else float(wei), mask0, nmask,
                                            taps.ctypes.data_as(C.POINTER(C.c_float)), r, _lib.ptr(dst), dst.stride(0),
                                            _lib.current_stream_ptr()), "tm_heat_field")
    return dst


def render(fld: torch.Tensor, lut: np.ndarray, vmin: float = 0.0, vmax: float = 1.0, scale: int = 1, floor: int = 0,
           interleaved: bool = False):
    """Colour bytes of a float32 device field [H, W] through the uint8 [N, 3] table `lut`: three planar uint8 [H scale,
    W scale] device planes (r, g, b), as ometiff.Composite / write_pyramid_rgb take, or with interleaved=True one
    [H scale, W scale, 3] image, as the colour encoder's overlay takes.  Values at or below vmin take entry 0, at or above
    vmax entry N - 1; entries below `floor` are painted black (the overlay blend treats black as transparent)."""
    if not (isinstance(fld, torch.Tensor) and fld.is_cuda and fld.dtype == torch.float32 and fld.dim() == 2 and fld.stride(1) == 1):
        raise ValueError("render takes a 2-D float32 device tensor with unit column stride")
    lut = np.ascontiguousarray(lut)
    if lut.dtype != np.uint8 or lut.ndim != 2 or lut.shape[1] != 3:
        raise ValueError(f"the table is uint8 [N, 3], got {lut.dtype} {lut.shape}")
    if not float(vmax) > float(vmin):
        raise ValueError(f"vmax {vmax} must exceed vmin {vmin}")
    inv_range = np.float32(1.0 / (float(vmax) - float(vmin)))
    H, W = fld.shape
    s = int(scale)
    if s not in SCALES:                                            # the library refuses it too; the sizes below need it first
        raise ValueError(f"scale must be one of {SCALES}, got {scale}")
    if interleaved:
        out = torch.empty((H * s, W * s, 3), dtype=torch.uint8, device=fld.device)
        dst = (None, None, _lib.ptr(out), out.stride(0))
    else:
        out = tuple(torch.empty((H * s, W * s), dtype=torch.uint8, device=fld.device) for _ in range(3))
        dst = ((C.c_void_p * 3)(*[p.data_ptr() for p in out]), (C.c_int64 * 3)(*[p.stride(0) for p in out]), None, 0)
    with torch.cuda.device(fld.device):
        _lib.check(_lib.lib().tm_heat_render(C.c_void_p(fld.data_ptr()), H, W, fld.stride(0), s, float(np.float32(vmin)),
                                             float(inv_range), lut.ctypes.data_as(C.c_void_p), lut.shape[0], int(floor), *dst,
                                             _lib.current_stream_ptr()), "tm_heat_render")
    return out


# cm.inferno(np.arange(256), bytes=True)[:, :3] of matplotlib 3.10 (the table itself has not changed since 1.5), as plain data
INFERNO = np.array([
    0, 0, 3, 0, 0, 4, 0, 0, 6, 1, 0, 7, 1, 1, 9, 1, 1, 11, 2, 1, 14, 2, 2, 16, 3, 2, 18, 4, 3, 20, 4, 3, 22, 5, 4, 24,
    6, 4, 27, 7, 5, 29, 8, 6, 31, 9, 6, 33, 10, 7, 35, 11, 7, 38, 13, 8, 40, 14, 8, 42, 15, 9, 45, 16, 9, 47, 18, 10,
    50, 19, 10, 52, 20, 11, 54, 22, 11, 57, 23, 11, 59, 25, 11, 62, 26, 11, 64, 28, 12, 67, 29, 12, 69, 31, 12, 71,
    32, 12, 74, 34, 11, 76, 36, 11, 78, 38, 11, 80, 39, 11, 82, 41, 11, 84, 43, 10, 86, 45, 10, 88, 46, 10, 90, 48,
    10, 92, 50, 9, 93, 52, 9, 95, 53, 9, 96, 55, 9, 97, 57, 9, 98, 59, 9, 100, 60, 9, 101, 62, 9, 102, 64, 9, 102, 65,
    9, 103, 67, 10, 104, 69, 10, 105, 70, 10, 105, 72, 11, 106, 74, 11, 106, 75, 12, 107, 77, 12, 107, 79, 13, 108,
    80, 13, 108, 82, 14, 108, 83, 14, 109, 85, 15, 109, 87, 15, 109, 88, 16, 109, 90, 17, 109, 91, 17, 110, 93, 18,
    110, 95, 18, 110, 96, 19, 110, 98, 20, 110, 99, 20, 110, 101, 21, 110, 102, 21, 110, 104, 22, 110, 106, 23, 110,
    107, 23, 110, 109, 24, 110, 110, 24, 110, 112, 25, 110, 114, 25, 109, 115, 26, 109, 117, 27, 109, 118, 27, 109,
    120, 28, 109, 122, 28, 109, 123, 29, 108, 125, 29, 108, 126, 30, 108, 128, 31, 107, 129, 31, 107, 131, 32, 107,
    133, 32, 106, 134, 33, 106, 136, 33, 106, 137, 34, 105, 139, 34, 105, 141, 35, 105, 142, 36, 104, 144, 36, 104,
    145, 37, 103, 147, 37, 103, 149, 38, 102, 150, 38, 102, 152, 39, 101, 153, 40, 100, 155, 40, 100, 156, 41, 99,
    158, 41, 99, 160, 42, 98, 161, 43, 97, 163, 43, 97, 164, 44, 96, 166, 44, 95, 167, 45, 95, 169, 46, 94, 171, 46,
    93, 172, 47, 92, 174, 48, 91, 175, 49, 91, 177, 49, 90, 178, 50, 89, 180, 51, 88, 181, 51, 87, 183, 52, 86, 184,
    53, 86, 186, 54, 85, 187, 55, 84, 189, 55, 83, 190, 56, 82, 191, 57, 81, 193, 58, 80, 194, 59, 79, 196, 60, 78,
    197, 61, 77, 199, 62, 76, 200, 62, 75, 201, 63, 74, 203, 64, 73, 204, 65, 72, 205, 66, 71, 207, 68, 70, 208, 69,
    68, 209, 70, 67, 210, 71, 66, 212, 72, 65, 213, 73, 64, 214, 74, 63, 215, 75, 62, 217, 77, 61, 218, 78, 59, 219,
    79, 58, 220, 80, 57, 221, 82, 56, 222, 83, 55, 223, 84, 54, 224, 86, 52, 226, 87, 51, 227, 88, 50, 228, 90, 49,
    229, 91, 48, 230, 92, 46, 230, 94, 45, 231, 95, 44, 232, 97, 43, 233, 98, 42, 234, 100, 40, 235, 101, 39, 236,
    103, 38, 237, 104, 37, 237, 106, 35, 238, 108, 34, 239, 109, 33, 240, 111, 31, 240, 112, 30, 241, 114, 29, 242,
    116, 28, 242, 117, 26, 243, 119, 25, 243, 121, 24, 244, 122, 22, 245, 124, 21, 245, 126, 20, 246, 128, 18, 246,
    129, 17, 247, 131, 16, 247, 133, 14, 248, 135, 13, 248, 136, 12, 248, 138, 11, 249, 140, 9, 249, 142, 8, 249, 144,
    8, 250, 145, 7, 250, 147, 6, 250, 149, 6, 250, 151, 6, 251, 153, 6, 251, 155, 6, 251, 157, 6, 251, 158, 7, 251,
    160, 7, 251, 162, 8, 251, 164, 10, 251, 166, 11, 251, 168, 13, 251, 170, 14, 251, 172, 16, 251, 174, 18, 251, 176,
    20, 251, 177, 22, 251, 179, 24, 251, 181, 26, 251, 183, 28, 251, 185, 30, 250, 187, 33, 250, 189, 35, 250, 191,
    37, 250, 193, 40, 249, 195, 42, 249, 197, 44, 249, 199, 47, 248, 201, 49, 248, 203, 52, 248, 205, 55, 247, 207,
    58, 247, 209, 60, 246, 211, 63, 246, 213, 66, 245, 215, 69, 245, 217, 72, 244, 219, 75, 244, 220, 79, 243, 222,
    82, 243, 224, 86, 243, 226, 89, 242, 228, 93, 242, 230, 96, 241, 232, 100, 241, 233, 104, 241, 235, 108, 241, 237,
    112, 241, 238, 116, 241, 240, 121, 241, 242, 125, 242, 243, 129, 242, 244, 133, 243, 246, 137, 244, 247, 141, 245,
    248, 145, 246, 250, 149, 247, 251, 153, 249, 252, 157, 250, 253, 160, 252, 254, 164], dtype=np.uint8).reshape(256, 3)
INFERNO.setflags(write=False)
