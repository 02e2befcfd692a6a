// Attention heat maps (test_attn.py:145-250, `gen_img`): the smoothed scalar field of one mosaic slice and its colour bytes.
// C entry points: tm_heat_field, tm_heat_render (bottom of this file); the statements are in include/teramind_hip.h.
// This unit is compiled with -ffp-contract=off: the render rule is held bit for bit to a float32 restatement in which every
// operation is rounded once; the field kernel asks for its multiply-adds by name (__builtin_fmaf), it is held to a bound.
//
// heat_field_kernel, one pass per slice, a workgroup of 256 lanes owns a HF_TH x HF_TW = 32 x 64 tile of dst:
//   stage   p = mask ? log2(sum * wei + 1) : 0 of the tile plus an r-wide halo, (32 + 2 r) x (64 + 2 r) cells, into LDS; the
//           reflection is applied to the source index, so neighbouring workgroups compute the halo again (no global scratch)
//   axis 0  item (g, x): column x of the staged width, the 4 output rows 4 g ..: 2 r + 4 LDS reads for 4 outputs, taps in
//           order 0 .. 2 r from a zero accumulator, into mid[32][64 + 2 r]
//   axis 1  item (y, g): row y, the 4 output columns 4 g ..; the same march along x; stored to dst
// Lanes of a wave read consecutive columns in axis 0 and, in axis 1, columns 4 apart in rows an odd number of dwords apart
// (hf_row): neither meets a bank twice within a 32-lane group.  LDS: (32 + 2 r) + 32 rows of 65 + 2 r floats, 37 KB at r = 16,
// 26 KB at r = 8, asked for per launch: the staged cells are 1.9 x the tile's at r = 8 and six workgroups still fit a CU.
// No atomics, no data-dependent order: two calls give the same bits.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/teramind_hip.h"
#include "tm_kernels.h"

namespace tmk {

constexpr int HF_TH = 32, HF_TW = 64, HF_RMAX = 16, HF_CMAX = 8, HF_Q = 4;
struct HeatTaps {
  float w[2 * HF_RMAX + 1];
  int r;
};
struct HeatSrc {
  const __half* p;
  long pitch, chan;             // in elements
  int H, W, sum0, nsum, mask0, nmask;
  float wei;
};

// scipy's mode='reflect' (half-sample): -j -> j - 1, n - 1 + j -> n - j.  One reflection is enough for |overshoot| <= n; the
// clamp keeps the cells of a partial tile that no output reads inside the plane.
__device__ __forceinline__ int hf_reflect(int i, int n) {
  i = i < 0 ? -i - 1 : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// staged row length in floats: odd, so that the lanes of axis 1 (columns 4 apart, rows apart by the row length) spread over the banks
__host__ __device__ constexpr int hf_row(int r) { return (HF_TW + 2 * r) | 1; }
static size_t hf_lds_bytes(int r) { return (size_t)(2 * HF_TH + 2 * r) * hf_row(r) * sizeof(float); }

// HF_Q neighbouring outputs of one filter axis: acc[q] = sum_j t[j] in[(q + j) step], taps in order 0 .. 2 r from zero, each
// input read once.  RT >= 0: unrolled for that radius, the taps from the kernel arguments (scalar registers); RT < 0: the radius
// at run time, the taps from LDS.  A tap meets only the inputs of its own window (no zero-padded taps: 0 x inf stays out).
template <int RT>
__device__ __forceinline__ void hf_march(const float* in, int step, int r, const float* tk, const float* tl, float* acc) {
#pragma unroll
  for (int q = 0; q < HF_Q; ++q) acc[q] = 0.f;
  if (RT >= 0) {
#pragma unroll
    for (int k = 0; k < 2 * RT + HF_Q; ++k) {
      const float v = in[k * step];
#pragma unroll
      for (int q = 0; q < HF_Q; ++q)
        if (k - q >= 0 && k - q <= 2 * RT) acc[q] = __builtin_fmaf(tk[k - q], v, acc[q]);
    }
  } else {
#pragma unroll 1
    for (int k = 0; k < 2 * r + HF_Q; ++k) {
      const float v = in[k * step];
#pragma unroll
      for (int q = 0; q < HF_Q; ++q)
        if (k - q >= 0 && k - q <= 2 * r) acc[q] = __builtin_fmaf(tl[k - q], v, acc[q]);
    }
  }
}

// RT: the radius the tap loops are unrolled for, -1 = taps.r at run time.  Both give the same bits.
template <int RT>
__global__ __launch_bounds__(256) void heat_field_kernel(const HeatSrc s, const HeatTaps taps, int tiles_x, float* __restrict__ dst,
                                                         long dpitch) {
  extern __shared__ float hf_lds[];
  __shared__ float s_taps[2 * HF_RMAX + 1];
  if (RT < 0 && threadIdx.x <= 2 * HF_RMAX) s_taps[threadIdx.x] = taps.w[threadIdx.x];      // before the first barrier
  const int r = RT >= 0 ? RT : taps.r;
  const int row = hf_row(r), sw = HF_TW + 2 * r, sh = HF_TH + 2 * r;
  float* stage = hf_lds;                       // [sh][row]
  float* mid = hf_lds + sh * row;              // [HF_TH][row]
  const int tid = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * HF_TH, x0 = tx * HF_TW;

  for (int i = tid; i < sh * sw; i += 256) {
    const int ly = i / sw, lx = i - ly * sw;
    const int gy = hf_reflect(y0 - r + ly, s.H), gx = hf_reflect(x0 - r + lx, s.W);
    const __half* c = s.p + (long)gy * s.pitch + gx;
    float v = 0.f;
    for (int k = 0; k < s.nsum; ++k) v = v + fmaxf(__half2float(c[(long)(s.sum0 + k) * s.chan]), 0.f);
    bool m = true;
    for (int k = 0; k < s.nmask; ++k) m = m && (__half2float(c[(long)(s.mask0 + k) * s.chan]) != 0.f);
    const float f = log2f(v * s.wei + 1.0f);
    stage[ly * row + lx] = m ? f : 0.f;
  }
  __syncthreads();

  // axis 0: mid[y][x] = sum_j t[j] stage[y + j][x]
  for (int i = tid; i < (HF_TH / HF_Q) * sw; i += 256) {
    const int g = i / sw, x = i - g * sw;
    const float* in = stage + (g * HF_Q) * row + x;
    float acc[HF_Q];
    hf_march<RT>(in, row, r, taps.w, s_taps, acc);
#pragma unroll
    for (int q = 0; q < HF_Q; ++q) mid[(g * HF_Q + q) * row + x] = acc[q];
  }
  __syncthreads();

  // axis 1: dst[y][x] = sum_j t[j] mid[y][x + j]
  for (int i = tid; i < HF_TH * (HF_TW / HF_Q); i += 256) {
    const int y = i / (HF_TW / HF_Q), g = i - y * (HF_TW / HF_Q);
    const float* in = mid + y * row + g * HF_Q;
    float acc[HF_Q];
    hf_march<RT>(in, 1, r, taps.w, s_taps, acc);
    const int gy = y0 + y;
    if (gy < s.H) {
#pragma unroll
      for (int q = 0; q < HF_Q; ++q) {
        const int gx = x0 + g * HF_Q + q;
        if (gx < s.W) dst[(long)gy * dpitch + gx] = acc[q];
      }
    }
  }
}

static hipError_t launch_heat_field(const HeatSrc& src, const HeatTaps& taps, float* dst, long dpitch, hipStream_t s) {
  const int tiles_x = (src.W + HF_TW - 1) / HF_TW, tiles_y = (src.H + HF_TH - 1) / HF_TH;
  const dim3 grid((unsigned)((long)tiles_x * tiles_y));
  const size_t lds = hf_lds_bytes(taps.r);
  if (taps.r == 8)
    heat_field_kernel<8><<<grid, dim3(256), lds, s>>>(src, taps, tiles_x, dst, dpitch);
  else
    heat_field_kernel<-1><<<grid, dim3(256), lds, s>>>(src, taps, tiles_x, dst, dpitch);
  return hipGetLastError();
}

// ---- render ------------------------------------------------------------------------------------------------------------
// A lane owns 4 consecutive pixels of one output row; a workgroup is 64 x 4 lanes = 256 x 4 pixels.  The table (entries below
// floor_idx already black, done on the host) comes in the kernel arguments and is copied to LDS once per workgroup.  With
// ALIGNED every destination pointer and pitch is a multiple of 4 and a lane stores whole dwords where its 4 pixels are inside.
constexpr int HR_PX = 4;
struct HeatLut {
  uint32_t rgb[256];            // r | g << 8 | b << 16
  int n;
};
struct HeatDst {
  uint8_t* plane[3];            // planar: all three set; interleaved: plane[0] only
  long pitch[3];
  int interleaved;
};

// the pixel rule of tm_heat_render: every operation rounded once (this unit is built without contraction)
__device__ __forceinline__ uint32_t heat_px(const float* __restrict__ field, long fpitch, int H, int W, float inv_scale, int y0, int y1,
                                            float wy, int x, float vmin, float inv_range, int n, const uint32_t* lut) {
  float sx = ((float)x + 0.5f) * inv_scale - 0.5f;
  sx = fminf(fmaxf(sx, 0.f), (float)(W - 1));
  const int xa = (int)sx, xb = min(xa + 1, W - 1);
  const float wx = sx - (float)xa;
  const float f00 = field[(long)y0 * fpitch + xa], f01 = field[(long)y0 * fpitch + xb];
  const float f10 = field[(long)y1 * fpitch + xa], f11 = field[(long)y1 * fpitch + xb];
  const float top = f00 + (f01 - f00) * wx;
  const float bot = f10 + (f11 - f10) * wx;
  const float g = top + (bot - top) * wy;
  const float i = ((g - vmin) * inv_range) * (float)n;
  const int idx = !(i >= 0.f) ? 0 : (i >= (float)n ? n - 1 : (int)i);
  return lut[idx];
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void heat_render_kernel(const float* __restrict__ field, int H, int W, long fpitch, int scale, float vmin,
                                                          float inv_range, const HeatLut lut, int tiles_x, const HeatDst d) {
  __shared__ uint32_t s_lut[256];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  s_lut[tid] = lut.rgb[tid];
  __syncthreads();
  const int h = H * scale, w = W * scale;
  const int by = (int)(blockIdx.x / (unsigned)tiles_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)tiles_x);
  const int y = by * 4 + threadIdx.y, x = (bx * 64 + threadIdx.x) * HR_PX;
  if (y >= h || x >= w) return;
  const float inv_scale = 1.0f / (float)scale;
  float sy = ((float)y + 0.5f) * inv_scale - 0.5f;
  sy = fminf(fmaxf(sy, 0.f), (float)(H - 1));
  const int y0 = (int)sy, y1 = min(y0 + 1, H - 1);
  const float wy = sy - (float)y0;
  uint32_t v[HR_PX];
#pragma unroll
  for (int q = 0; q < HR_PX; ++q) v[q] = heat_px(field, fpitch, H, W, inv_scale, y0, y1, wy, min(x + q, w - 1), vmin, inv_range, lut.n, s_lut);
  const bool whole = x + HR_PX <= w;
  if (d.interleaved) {
    uint8_t* o = d.plane[0] + (long)y * d.pitch[0] + 3L * x;
    if (ALIGNED && whole) {
      uint32_t* o4 = (uint32_t*)o;               // 12 x bytes from a 4-aligned row: aligned
      o4[0] = v[0] | (v[1] << 24);
      o4[1] = (v[1] >> 8) | (v[2] << 16);
      o4[2] = (v[2] >> 16) | (v[3] << 8);
    } else {
      for (int q = 0; q < HR_PX && x + q < w; ++q) {
        o[3 * q] = (uint8_t)v[q];
        o[3 * q + 1] = (uint8_t)(v[q] >> 8);
        o[3 * q + 2] = (uint8_t)(v[q] >> 16);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint8_t* o = d.plane[c] + (long)y * d.pitch[c] + x;
      const int sh = 8 * c;
      if (ALIGNED && whole) {
        *(uint32_t*)o = ((v[0] >> sh) & 255u) | (((v[1] >> sh) & 255u) << 8) | (((v[2] >> sh) & 255u) << 16) | (((v[3] >> sh) & 255u) << 24);
      } else {
        for (int q = 0; q < HR_PX && x + q < w; ++q) o[q] = (uint8_t)(v[q] >> sh);
      }
    }
  }
}

static hipError_t launch_heat_render(const float* field, int H, int W, long fpitch, int scale, float vmin, float inv_range,
                                     const HeatLut& lut, const HeatDst& d, bool aligned, hipStream_t s) {
  const long h = (long)H * scale, w = (long)W * scale;
  const int tiles_x = (int)((w + 64 * HR_PX - 1) / (64 * HR_PX));
  const dim3 grid((unsigned)(tiles_x * ((h + 3) / 4)));
  if (aligned)
    heat_render_kernel<true><<<grid, dim3(64, 4), 0, s>>>(field, H, W, fpitch, scale, vmin, inv_range, lut, tiles_x, d);
  else
    heat_render_kernel<false><<<grid, dim3(64, 4), 0, s>>>(field, H, W, fpitch, scale, vmin, inv_range, lut, tiles_x, d);
  return hipGetLastError();
}

}  // namespace tmk

extern "C" int tm_heat_field(const void* src, int C, int H, int W, int64_t src_pitch, int64_t src_chan, int sum0, int nsum, float wei,
                             int mask0, int nmask, const float* taps_host, int r, void* dst, int64_t dst_pitch, void* stream) {
  using namespace tmk;
  if (!src || !dst || !taps_host) return fail(TM_ERR_ARG, "tm_heat_field: null source / destination / taps");
  if (r < 0 || r > HF_RMAX) return fail(TM_ERR_ARG, "tm_heat_field: radius %d outside 0 .. %d", r, HF_RMAX);
  if (C < 1 || H < 1 || W < 1) return fail(TM_ERR_ARG, "tm_heat_field: C, H and W must be positive, got %d x %d x %d", C, H, W);
  if (H < r || W < r)
    return fail(TM_ERR_ARG, "tm_heat_field: %d x %d is below the radius %d (one reflection must reach every tap)", H, W, r);
  if (nsum < 1 || nsum > HF_CMAX) return fail(TM_ERR_ARG, "tm_heat_field: nsum %d outside 1 .. %d", nsum, HF_CMAX);
  if (nmask < 0 || nmask > HF_CMAX) return fail(TM_ERR_ARG, "tm_heat_field: nmask %d outside 0 .. %d", nmask, HF_CMAX);
  if (sum0 < 0 || sum0 > C - nsum) return fail(TM_ERR_ARG, "tm_heat_field: sum range [%d, %d) outside the %d channels", sum0, sum0 + nsum, C);
  if (nmask && (mask0 < 0 || mask0 > C - nmask))
    return fail(TM_ERR_ARG, "tm_heat_field: mask range [%d, %d) outside the %d channels", mask0, mask0 + nmask, C);
  if (src_pitch < W) return fail(TM_ERR_ARG, "tm_heat_field: source pitch %lld below W %d", (long long)src_pitch, W);
  if (dst_pitch < W) return fail(TM_ERR_ARG, "tm_heat_field: destination pitch %lld below W %d", (long long)dst_pitch, W);
  if (C > 1 && src_chan < (int64_t)(H - 1) * src_pitch + W)
    return fail(TM_ERR_ARG, "tm_heat_field: channel stride %lld below the extent of one channel", (long long)src_chan);
  if (((uintptr_t)src & 1) || ((uintptr_t)dst & 3)) return fail(TM_ERR_ARG, "tm_heat_field: misaligned source (2) / destination (4)");
  if (!(wei == wei)) return fail(TM_ERR_ARG, "tm_heat_field: wei is NaN");
  HeatTaps taps;
  memset(&taps, 0, sizeof taps);
  taps.r = r;
  for (int j = 0; j <= 2 * r; ++j) taps.w[j] = taps_host[j];
  HeatSrc s;
  s.p = (const __half*)src;
  s.pitch = (long)src_pitch;
  s.chan = (long)src_chan;
  s.H = H, s.W = W, s.sum0 = sum0, s.nsum = nsum, s.mask0 = nmask ? mask0 : 0, s.nmask = nmask, s.wei = wei;
  HIP_TRY(launch_heat_field(s, taps, (float*)dst, (long)dst_pitch, (hipStream_t)stream));
  return TM_OK;
}

extern "C" int tm_heat_render(const void* field, int H, int W, int64_t field_pitch, int scale, float vmin, float inv_range,
                              const uint8_t* lut_host, int N, int floor_idx, void* const* planes, const int64_t* pitches,
                              void* interleaved, int64_t inter_pitch, void* stream) {
  using namespace tmk;
  if (!field || !lut_host) return fail(TM_ERR_ARG, "tm_heat_render: null field / table");
  if ((planes != nullptr) == (interleaved != nullptr))
    return fail(TM_ERR_ARG, "tm_heat_render: give the three planes or the interleaved image, one of the two");
  if (planes && (!pitches || !planes[0] || !planes[1] || !planes[2])) return fail(TM_ERR_ARG, "tm_heat_render: null plane / pitches");
  if (H < 1 || W < 1) return fail(TM_ERR_ARG, "tm_heat_render: H and W must be positive, got %d x %d", H, W);
  if (scale != 1 && scale != 2 && scale != 4 && scale != 8 && scale != 16)
    return fail(TM_ERR_ARG, "tm_heat_render: scale %d is not one of 1, 2, 4, 8, 16", scale);
  if (N < 2 || N > 256) return fail(TM_ERR_ARG, "tm_heat_render: table length %d outside 2 .. 256", N);
  if (floor_idx < 0) return fail(TM_ERR_ARG, "tm_heat_render: floor_idx %d is negative", floor_idx);
  if (field_pitch < W || ((uintptr_t)field & 3)) return fail(TM_ERR_ARG, "tm_heat_render: field pitch %lld below W %d, or misaligned field", (long long)field_pitch, W);
  const int64_t h = (int64_t)H * scale, w = (int64_t)W * scale;
  if (3 * w > INT32_MAX || h > INT32_MAX || ((w + 255) / 256) * ((h + 3) / 4) > INT32_MAX)
    return fail(TM_ERR_ARG, "tm_heat_render: the %lld x %lld image is too large", (long long)h, (long long)w);
  HeatDst d;
  memset(&d, 0, sizeof d);
  bool aligned = true;
  if (interleaved) {
    if (inter_pitch < 3 * w) return fail(TM_ERR_ARG, "tm_heat_render: interleaved pitch %lld below 3 W scale = %lld", (long long)inter_pitch, (long long)(3 * w));
    d.interleaved = 1;
    d.plane[0] = (uint8_t*)interleaved;
    d.pitch[0] = (long)inter_pitch;
    aligned = !(((uintptr_t)interleaved | (uintptr_t)inter_pitch) & 3);
  } else {
    for (int c = 0; c < 3; ++c) {
      if (pitches[c] < w) return fail(TM_ERR_ARG, "tm_heat_render: pitch %lld of plane %d below W scale = %lld", (long long)pitches[c], c, (long long)w);
      d.plane[c] = (uint8_t*)planes[c];
      d.pitch[c] = (long)pitches[c];
      aligned = aligned && !(((uintptr_t)planes[c] | (uintptr_t)pitches[c]) & 3);
    }
  }
  HeatLut lut;
  memset(&lut, 0, sizeof lut);
  lut.n = N;
  for (int k = floor_idx < N ? floor_idx : N; k < N; ++k)
    lut.rgb[k] = (uint32_t)lut_host[3 * k] | ((uint32_t)lut_host[3 * k + 1] << 8) | ((uint32_t)lut_host[3 * k + 2] << 16);
  HIP_TRY(launch_heat_render((const float*)field, H, W, (long)field_pitch, scale, vmin, inv_range, lut, d, aligned, (hipStream_t)stream));
  return TM_OK;
}
