// ROI evaluation (utils/metrics.py:201-541 of the reference): the SSIM statistics of plane pairs in one pass, and
// the 2 x 2 padded mean of one MS-SSIM level.  C entry points: tm_ssim_planes, tm_avgpool2_pad (tm_ops.hip, which owns the
// stream-ordered scratch); the Python surface is teramind_amd.metrics.
//
// ssim_planes_kernel: one workgroup of 256 lanes per 64 x 32 tile of the valid output (SSIM_TW x SSIM_TH), per plane.
//   stage   the (32 + n - 1) x (64 + n - 1) pixels the tile needs, minus the tile's shifts (cx, cy: x and y at the tile's
//           first pixel), as fp32 into LDS (rx, ry; pixels outside the plane as 0).  Every pixel of the plane is OWNED by
//           exactly one tile (its 32 x 64 origin block; the last tile row / column also owns the n - 1 border rows /
//           columns): the owner adds (x - y)^2, as an exact integer for uint8 and in fp64 for fp32.
//   rows    item (r, g): input row r, 4 output columns 4 g ..: the five quantities a, b, a^2, b^2, a b (a = x - cx,
//           b = y - cy) filtered along x, taps in order 0 .. n - 1 from a zero accumulator, into hq[5][rows][65]
//   cols    lane (col, wave): 8 output rows 8 wave .. of column col: the same filter along y from hq, then per output
//           mu1 = m1 + cx S, s1 = q11 - m1^2 + (1 - S)(2 cx m1 + cx^2 S), s12 = q12 - m1 m2 + (1 - S)(cy m1 + cx m2 + cx cy S)
//           (S = the weight of the n x n window: the central moments about (cx, cy) equal the ones about 0 up to those
//           terms, which vanish for a normalised window), cs and ssim as utils/metrics.py:300-301
//   sums    the lane's 8 outputs in fp32 in row order, then fp64: xor-butterfly over the wave, the 4 waves in order
// ssim_sum_kernel: per plane, lane l adds the partials of tiles [l k, (l + 1) k) in index order, then the same tree.
// No atomics: two calls give the same bits.  Both loops over taps have trip counts fixed by n alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teramind_hip.h"
#include "tm_kernels.h"
#include "tm_device.h"

namespace tmk {

constexpr int SSIM_OPV = 8;                  // output rows per lane in the column pass (= SSIM_TAP_PAD + 1)
constexpr int SSIM_OPH = 4;                  // output columns per item in the row pass
constexpr int SSIM_HS = SSIM_TW + 1;         // row stride of hq in floats: odd, so the row pass stores without bank conflicts
static_assert(SSIM_TH == 4 * SSIM_OPV && SSIM_TW == 64 && SSIM_OPV == SSIM_TAP_PAD + 1 && SSIM_TW % SSIM_OPH == 0, "tile plan");

template <typename T> struct SsimPix;
template <> struct SsimPix<uint8_t> {
  typedef int Raw;
  typedef uint32_t Sq;                       // a workgroup owns at most 64 x 96 pixels of at most 255^2: below 2^32
  static __device__ __forceinline__ Raw load(const uint8_t* p, int i) { return p[i]; }
  static __device__ __forceinline__ Sq sqdiff(Raw xv, Raw yv) { return (uint32_t)((xv - yv) * (xv - yv)); }   // exact
};
template <> struct SsimPix<float> {
  typedef float Raw;
  typedef double Sq;
  static __device__ __forceinline__ Raw load(const uint8_t* p, int i) { return ((const float*)p)[i]; }
  static __device__ __forceinline__ Sq sqdiff(Raw xv, Raw yv) { const double d = (double)xv - (double)yv; return d * d; }
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the workgroup's sum of three fp64 values: butterfly per wave, then the waves in order; valid in lane 0 of wave 0
__device__ __forceinline__ void block_sum3_f64(double (&v)[3], double* s_red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = wave_sum_f64(v[k]);
    if (lane == 0) s_red[wv * 3 + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = ((s_red[k] + s_red[3 + k]) + s_red[6 + k]) + s_red[9 + k];
}

// NT: the window length the loops are unrolled for (only the taps that meet an output are issued), 0 = taps.n at run time
// (the zero pads of taps.w stand in for the taps that meet none: fma(0, h, acc) = acc).  Both give the same bits.
template <typename T, int NT>
__global__ __launch_bounds__(256) void ssim_planes_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y, int H, int W,
                                                          long xpitch, long xplane, long ypitch, long yplane, SsimTaps taps, float C1,
                                                          float C2, double* __restrict__ partials) {
  extern __shared__ float lds[];
  __shared__ double s_red[12];
  const int n = NT ? NT : taps.n;
  const int RA = SSIM_TH + n - 1, CA = SSIM_TW + n - 1, RS = CA + 1;    // RS odd: the row pass reads down a column of rx / ry
  float* rx = lds;
  float* ry = rx + RA * RS;
  float* hq = ry + RA * RS;                                             // [5][RA][SSIM_HS]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tx = blockIdx.x, ty = blockIdx.y, pl = blockIdx.z;
  const int ox = tx * SSIM_TW, oy = ty * SSIM_TH;
  const int rows = min(RA, H - oy), cols = min(CA, W - ox);             // what the plane holds of the tile's input
  const int own_r = ty == (int)gridDim.y - 1 ? rows : SSIM_TH, own_c = tx == (int)gridDim.x - 1 ? cols : SSIM_TW;
  const uint8_t* xt = x + (long)pl * xplane + (long)oy * xpitch;
  const uint8_t* yt = y + (long)pl * yplane + (long)oy * ypitch;
  const float cx = (float)SsimPix<T>::load(xt, ox), cy = (float)SsimPix<T>::load(yt, ox);

  // wave wv takes rows wv, wv + 4, ..; a lane the columns lane and lane + 64 (CA <= 96).  A pixel outside the plane reads the
  // clamped address instead (always inside the tile's part of the plane) and is replaced by 0 afterwards: no branch around a
  // load, so every load of the lane is in flight before the first use and the tile pays the memory latency once
  constexpr int KMAX = (SSIM_TH + (NT ? NT : SSIM_MAX_TAPS) - 1 + 3) / 4;
  typename SsimPix<T>::Raw vx[KMAX][2], vy[KMAX][2];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int r = min(wv + 4 * k, rows - 1);
    const uint8_t* px = xt + (long)r * xpitch;
    const uint8_t* py = yt + (long)r * ypitch;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cc = ox + min(lane + 64 * h, cols - 1);
      vx[k][h] = SsimPix<T>::load(px, cc);
      vy[k][h] = SsimPix<T>::load(py, cc);
    }
  }
  typename SsimPix<T>::Sq sq = 0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int r = wv + 4 * k;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cc = lane + 64 * h;
      const bool in = r < rows && cc < cols;
      if (r < own_r && cc < own_c) sq += SsimPix<T>::sqdiff(vx[k][h], vy[k][h]);          // own_r <= rows, own_c <= cols
      if (r < RA && cc < CA) {
        rx[r * RS + cc] = in ? (float)vx[k][h] - cx : 0.0f;                                // exact for uint8
        ry[r * RS + cc] = in ? (float)vy[k][h] - cy : 0.0f;
      }
    }
  }
  __syncthreads();

  for (int item = tid; item < RA * (SSIM_TW / SSIM_OPH); item += 256) {
    const int g = item / RA, r = item - g * RA;
    const float* px = rx + r * RS + g * SSIM_OPH;
    const float* py = ry + r * RS + g * SSIM_OPH;
    float acc[5][SSIM_OPH];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int o = 0; o < SSIM_OPH; ++o) acc[q][o] = 0.0f;
#pragma unroll
    for (int j = 0; j < SSIM_OPH + n - 1; ++j) {
      const float a = px[j], b = py[j];
      const float p[5] = {a, b, a * a, b * b, a * b};
#pragma unroll
      for (int o = 0; o < SSIM_OPH; ++o) {
        if (NT && (j - o < 0 || j - o >= NT)) continue;
        const float wt = taps.w[SSIM_TAP_PAD + j - o];
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q][o] = __builtin_fmaf(wt, p[q], acc[q][o]);
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int o = 0; o < SSIM_OPH; ++o) hq[(q * RA + r) * SSIM_HS + g * SSIM_OPH + o] = acc[q][o];
  }
  __syncthreads();

  float acc[5][SSIM_OPV];
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int o = 0; o < SSIM_OPV; ++o) acc[q][o] = 0.0f;
  const float* hc = hq + wv * SSIM_OPV * SSIM_HS + lane;
#pragma unroll
  for (int j = 0; j < SSIM_OPV + n - 1; ++j) {
    float h[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) h[q] = hc[(q * RA + j) * SSIM_HS];
#pragma unroll
    for (int o = 0; o < SSIM_OPV; ++o) {
      if (NT && (j - o < 0 || j - o >= NT)) continue;
      const float wt = taps.w[SSIM_TAP_PAD + j - o];
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[q][o] = __builtin_fmaf(wt, h[q], acc[q][o]);
    }
  }

  const float S = taps.sum, d = taps.one_minus_sum, cxS = cx * S, cyS = cy * S;
  const int Ho = H - n + 1, Wo = W - n + 1;
  float s_ssim = 0.0f, s_cs = 0.0f;
#pragma unroll
  for (int o = 0; o < SSIM_OPV; ++o) {
    const float m1 = acc[0][o], m2 = acc[1][o];
    const float mu1 = m1 + cxS, mu2 = m2 + cyS;
    const float s1 = (acc[2][o] - m1 * m1) + d * (2.0f * cx * m1 + cx * cxS);
    const float s2 = (acc[3][o] - m2 * m2) + d * (2.0f * cy * m2 + cy * cyS);
    const float s12 = (acc[4][o] - m1 * m2) + d * ((cy * m1 + cx * m2) + cx * cyS);
    const float cs = (2.0f * s12 + C2) / (s1 + s2 + C2);
    const float ss = ((2.0f * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs;
    const bool valid = oy + wv * SSIM_OPV + o < Ho && ox + lane < Wo;
    s_ssim += valid ? ss : 0.0f;
    s_cs += valid ? cs : 0.0f;
  }
  double v[3] = {(double)s_ssim, (double)s_cs, (double)sq};
  block_sum3_f64(v, s_red);
  if (tid == 0) {
    double* o = partials + ((long)pl * gridDim.y * gridDim.x + (long)ty * gridDim.x + tx) * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
}

__global__ __launch_bounds__(256) void ssim_sum_kernel(const double* __restrict__ partials, long ntiles, double* __restrict__ out) {
  __shared__ double s_red[12];
  const double* p = partials + (long)blockIdx.x * ntiles * 3;
  const long chunk = (ntiles + 255) / 256, t0 = threadIdx.x * chunk, t1 = t0 + chunk < ntiles ? t0 + chunk : ntiles;
  double v[3] = {0.0, 0.0, 0.0};
  for (long t = t0; t < t1; ++t) { v[0] += p[t * 3]; v[1] += p[t * 3 + 1]; v[2] += p[t * 3 + 2]; }
  block_sum3_f64(v, s_red);
  if (threadIdx.x == 0) { out[blockIdx.x * 3] = v[0]; out[blockIdx.x * 3 + 1] = v[1]; out[blockIdx.x * 3 + 2] = v[2]; }
}

size_t ssim_lds_bytes(int n) {
  const int RA = SSIM_TH + n - 1, RS = SSIM_TW + n;
  return (size_t)(2 * RA * RS + 5 * RA * SSIM_HS) * sizeof(float);
}
size_t ssim_partial_doubles(int P, int H, int W, int n) {
  return (size_t)3 * P * ((H - n + SSIM_TH) / SSIM_TH) * ((W - n + SSIM_TW) / SSIM_TW);
}

template <typename T, int NT>
static hipError_t ssim_launch(const uint8_t* x, const uint8_t* y, int P, int H, int W, long xpitch, long xplane, long ypitch, long yplane,
                              const SsimTaps& taps, float C1, float C2, double* partials, hipStream_t s) {
  static DevOnce once;
  if (once.need()) {                                     // the 33-tap window takes 133 KB of the CU's 160 KB
    hipError_t e = hipFuncSetAttribute((const void*)ssim_planes_kernel<T, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)ssim_lds_bytes(NT ? NT : SSIM_MAX_TAPS));
    if (e != hipSuccess) return e;
    once.mark();
  }
  const dim3 grid((W - taps.n + SSIM_TW) / SSIM_TW, (H - taps.n + SSIM_TH) / SSIM_TH, P);
  ssim_planes_kernel<T, NT><<<grid, dim3(256), ssim_lds_bytes(taps.n), s>>>(x, y, H, W, xpitch, xplane, ypitch, yplane, taps, C1, C2, partials);
  return hipGetLastError();
}

hipError_t launch_ssim_planes(const void* x, const void* y, bool is_f32, int P, int H, int W, long xpitch, long xplane, long ypitch,
                              long yplane, const SsimTaps& taps, float C1, float C2, double* partials, double* out, hipStream_t s) {
  const uint8_t* xb = (const uint8_t*)x;
  const uint8_t* yb = (const uint8_t*)y;
  hipError_t e;
  if (taps.n == 11)
    e = is_f32 ? ssim_launch<float, 11>(xb, yb, P, H, W, xpitch, xplane, ypitch, yplane, taps, C1, C2, partials, s)
               : ssim_launch<uint8_t, 11>(xb, yb, P, H, W, xpitch, xplane, ypitch, yplane, taps, C1, C2, partials, s);
  else
    e = is_f32 ? ssim_launch<float, 0>(xb, yb, P, H, W, xpitch, xplane, ypitch, yplane, taps, C1, C2, partials, s)
               : ssim_launch<uint8_t, 0>(xb, yb, P, H, W, xpitch, xplane, ypitch, yplane, taps, C1, C2, partials, s);
  if (e != hipSuccess) return e;
  const long ntiles = (long)((H - taps.n + SSIM_TH) / SSIM_TH) * ((W - taps.n + SSIM_TW) / SSIM_TW);
  ssim_sum_kernel<<<dim3((unsigned)P), dim3(256), 0, s>>>(partials, ntiles, out);
  return hipGetLastError();
}

// ---- one MS-SSIM level: F.avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2)), the zero pad counted --------------------
// dst [ceil(H / 2)][ceil(W / 2)]: the window of (i, j) starts at (2 i - H % 2, 2 j - W % 2); a row / column -1 is the pad.
// The last window ends at row H - 1 / column W - 1, so nothing is read beyond the plane.
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_pad_kernel(const uint8_t* __restrict__ src, int H, int W, long spitch, long splane,
                                                           uint8_t* __restrict__ dst, int Ho, int Wo, long dpitch, long dplane) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Ho * Wo) return;
  const int i = (int)(idx / Wo), j = (int)(idx - (long)i * Wo);
  const int r0 = 2 * i - (H & 1), c0 = 2 * j - (W & 1);
  const T* a = (const T*)(src + (long)blockIdx.y * splane + (long)(r0 < 0 ? 0 : r0) * spitch);
  const T* b = (const T*)(src + (long)blockIdx.y * splane + (long)(r0 + 1) * spitch);
  const float v00 = r0 >= 0 && c0 >= 0 ? (float)a[c0] : 0.0f, v01 = r0 >= 0 ? (float)a[c0 + 1] : 0.0f;
  const float v10 = c0 >= 0 ? (float)b[c0] : 0.0f, v11 = (float)b[c0 + 1];
  ((float*)(dst + (long)blockIdx.y * dplane + (long)i * dpitch))[j] = (((v00 + v01) + v10) + v11) * 0.25f;
}

hipError_t launch_avgpool2_pad(const void* src, bool is_f32, int P, int H, int W, long spitch, long splane, void* dst, long dpitch,
                               long dplane, hipStream_t s) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const dim3 grid((unsigned)(((long)Ho * Wo + 255) / 256), (unsigned)P);
  if (is_f32)
    avgpool2_pad_kernel<float><<<grid, dim3(256), 0, s>>>((const uint8_t*)src, H, W, spitch, splane, (uint8_t*)dst, Ho, Wo, dpitch, dplane);
  else
    avgpool2_pad_kernel<uint8_t><<<grid, dim3(256), 0, s>>>((const uint8_t*)src, H, W, spitch, splane, (uint8_t*)dst, Ho, Wo, dpitch, dplane);
  return hipGetLastError();
}

}  // namespace tmk
