// ROI evaluation (utils/metrics.py:201-541 of the reference): the SSIM statistics of plane pairs in one pass, and
// the 2 x 2 padded mean of one MS-SSIM level.  C entry points: tm_ssim_planes, tm_avgpool2_pad (tm_ops.hip, which owns the
// stream-ordered scratch); the Python surface is teramind_amd.metrics.  The 3-D window of a 5-D input (tm_ssim_volumes,
// tm_avgpool2_pad3) is the second half of this file.
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
  static constexpr int BYTES = 1;
  typedef uint32_t Sq;                       // a workgroup owns at most 64 x 96 pixels of at most 255^2: below 2^32
  static __device__ __forceinline__ Raw load(const uint8_t* p, int i) { return p[i]; }
  static __device__ __forceinline__ Sq sqdiff(Raw xv, Raw yv) { return (uint32_t)((xv - yv) * (xv - yv)); }   // exact
};
template <> struct SsimPix<float> {
  typedef float Raw;
  typedef double Sq;
  static constexpr int BYTES = 4;
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

// ---- volumes: the 3-D window of `_ssim` on a 5-D input (utils/metrics.py:236-305 with conv3d) ------------------------------
// ssim_volumes_kernel: one workgroup of 256 lanes per 16 x 16 tile of the valid in-plane output (SSIM3_TW x SSIM3_TH), per
// volume; it marches along z over every plane of the volume.  The window always runs as SSIM3_TAPS = 11 taps, a shorter one
// zero-padded behind (fma(0, v, acc) = acc: the same bits as a shorter loop); the valid region is that of the real n.
//   stage   the 26 x 26 pixels of plane z the tile needs, minus the tile's shifts (cx, cy: x and y at the tile's first
//           voxel, plane 0), as fp32 into LDS; pixels outside the plane as 0.  Addresses are clamped into the tile's part
//           of the plane, no branch around a load; the loads of plane z + 1 are issued before the passes over plane z.
//           No branch around a store either: keep = 0 zeroes a pixel outside the plane, own = 0 its squared difference.
//           A pixel is OWNED by its 16 x 16 origin block (the last tile row / column also owns the border): the owner adds
//           (x - y)^2, for uint8 as an exact integer (uint32 per plane, uint64 above), for fp32 in fp64.
//   rows    item (r, g), 104 of them: input row r, 4 output columns 4 g ..: a, b, a^2, b^2, a b filtered along x, taps in
//           order from a zero accumulator, into hq[5][26][17]
//   cols    lane (col, row): its one output of the plane: the same filter along y from hq
//   depth   the lane keeps, per value, the 10 output planes whose windows are open: pend[t] has taken taps 0 .. t.  Plane z
//           closes the oldest, m = fma(w[10], v, pend[9]), moves every other one up a slot with its next tap, pend[t] =
//           fma(w[t], v, pend[t - 1]), and opens a new one, pend[0] = w[0] v: the taps in order from zero, the ring turns
//           without a copy, every index is static in ONE z body, and the 50 partial sums are registers (the compile report
//           shows the declared LDS arrays only, no scratch and no spilled register of either file).  From m: mu, sigma, cs
//           and ssim as in the plane kernel with S = (sum of the taps)^3; the lane owns ONE output per plane, so nothing is
//           added in fp32: the output goes to the lane's fp64 total.  11 - n planes of zeros past the volume close the last
//           windows of a shorter tap set.
//   sums    fp64: the lane's planes in z order, xor-butterfly over the wave, the 4 waves in order, then ssim_sum_kernel
//           over the tiles.  No atomics: two calls give the same bits.
template <typename T>
__global__ __launch_bounds__(256) void ssim_volumes_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y, int D, int H, int W,
                                                           long xpitch, long xdepth, long xvol, long ypitch, long ydepth, long yvol,
                                                           Ssim3Taps taps, float C1, float C2, double* __restrict__ partials) {
  constexpr int NW = SSIM3_TAPS, TH = SSIM3_TH, TW = SSIM3_TW;
  constexpr int RA = TH + NW - 1, CA = TW + NW - 1, RS = CA + 1, HS = TW + 1;   // RS, HS odd: as in the plane kernel
  constexpr int KL = (RA * CA + 255) / 256, OPH = 4;
  static_assert(RA * (TW / OPH) <= 256 && TW * TH == 256 && (RS & 1) && (HS & 1), "tile plan");
  __shared__ float rx[RA * RS + 1], ry[RA * RS + 1], hq[5 * RA * HS];
  __shared__ double s_red[12];
  __shared__ float s_taps[NW];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x, ty = blockIdx.y, vl = blockIdx.z;
  const int n = taps.n;
  if (tid < NW) s_taps[tid] = taps.w[tid];
  const int ox = tx * TW, oy = ty * TH;
  const int rows = min(RA, H - oy), cols = min(CA, W - ox);
  const int own_r = ty == (int)gridDim.y - 1 ? rows : TH, own_c = tx == (int)gridDim.x - 1 ? cols : TW;
  const uint8_t* xt = x + (long)vl * xvol + (long)oy * xpitch;
  const uint8_t* yt = y + (long)vl * yvol + (long)oy * ypitch;
  const float cx = (float)SsimPix<T>::load(xt, ox), cy = (float)SsimPix<T>::load(yt, ox);

  // the lane's KL pixels of a staged plane: pixel i = tid + 256 k of the RA x CA input, row-major; addresses clamped into
  // the tile's part of the plane (byte offsets from the tile's first pixel: below 2^31, the entry point checks the pitch).
  // No branch in the staging either: a pixel outside the plane is multiplied by keep = 0, one the tile does not own adds
  // own = 0 times its squared difference, and an item beyond the input stores into the spare slot behind rx / ry.
  int offx[KL], offy[KL], sidx[KL];
  float keep[KL];
  typename SsimPix<T>::Sq own[KL];
#pragma unroll
  for (int k = 0; k < KL; ++k) {
    const int i = tid + 256 * k, r = i / CA, c = i - r * CA;
    const int rr = min(r, rows - 1), cc = min(c, cols - 1) * SsimPix<T>::BYTES;
    offx[k] = rr * (int)xpitch + cc;
    offy[k] = rr * (int)ypitch + cc;
    sidx[k] = r < RA ? r * RS + c : RA * RS;
    keep[k] = r < rows && c < cols ? 1.0f : 0.0f;
    own[k] = r < own_r && c < own_c ? 1 : 0;                           // own_r <= rows, own_c <= cols
  }
  typename SsimPix<T>::Raw vx[KL], vy[KL];
  auto fetch = [&](int z) {
    const uint8_t* px = xt + (long)z * xdepth + (long)ox * SsimPix<T>::BYTES;
    const uint8_t* py = yt + (long)z * ydepth + (long)ox * SsimPix<T>::BYTES;
#pragma unroll
    for (int k = 0; k < KL; ++k) {
      vx[k] = SsimPix<T>::load(px + offx[k], 0);
      vy[k] = SsimPix<T>::load(py + offy[k], 0);
    }
  };

  // pend[t][q]: the output plane that has taken taps 0 .. t of value q so far (t = 0 .. NW - 2); static indices, one z body
  float pend[NW - 1][5];
#pragma unroll
  for (int t = 0; t < NW - 1; ++t)
#pragma unroll
    for (int q = 0; q < 5; ++q) pend[t][q] = 0.0f;
  const int col = tid & (TW - 1), row = tid / TW;                      // column pass and depth pass: the lane's one output
  const int ig = tid / RA, ir = tid - ig * RA;                         // row pass: row ir, columns ig * OPH ..
  const float S = taps.sum, d = taps.one_minus_sum, cxS = cx * S, cyS = cy * S;
  const int Do = D - n + 1, Ho = H - n + 1, Wo = W - n + 1;
  const bool valid = oy + row < Ho && ox + col < Wo;
  double t_ssim = 0.0, t_cs = 0.0, t_sq = 0.0;
  uint64_t t_sq_int = 0;
  const int Dtot = D + NW - n;                                         // NW - n planes of zeros close the last windows

  // the row pass takes its taps from vector registers (read back from LDS): the compiler packs two neighbouring outputs
  // into one v_pk_fma, and as scalar operands the dozen tap pairs that needs would not fit the scalar file next to the rest
  __syncthreads();
  float tw[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) tw[t] = s_taps[t];
  fetch(0);
#pragma unroll 1
  for (int z = 0; z < Dtot; ++z) {
    float v[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (z < D) {                                                       // uniform over the workgroup
      typename SsimPix<T>::Sq sq = 0;
#pragma unroll
      for (int k = 0; k < KL; ++k) {
        sq += own[k] * SsimPix<T>::sqdiff(vx[k], vy[k]);
        rx[sidx[k]] = ((float)vx[k] - cx) * keep[k];                   // the difference is exact for uint8
        ry[sidx[k]] = ((float)vy[k] - cy) * keep[k];
      }
      if (sizeof(typename SsimPix<T>::Sq) == 4) t_sq_int += (uint64_t)sq; else t_sq += (double)sq;
      __syncthreads();
      fetch(min(z + 1, D - 1));                                        // in flight under the passes

      if (tid < RA * (TW / OPH)) {
        const float* px = rx + ir * RS + ig * OPH;
        const float* py = ry + ir * RS + ig * OPH;
        float h[5][OPH];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
          for (int o = 0; o < OPH; ++o) h[q][o] = 0.0f;
#pragma unroll
        for (int j = 0; j < OPH + NW - 1; ++j) {
          const float a = px[j], b = py[j];
          const float p[5] = {a, b, a * a, b * b, a * b};
#pragma unroll
          for (int o = 0; o < OPH; ++o) {
            if (j - o < 0 || j - o >= NW) continue;
            const float wt = tw[j - o];
#pragma unroll
            for (int q = 0; q < 5; ++q) h[q][o] = __builtin_fmaf(wt, p[q], h[q][o]);
          }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
          for (int o = 0; o < OPH; ++o) hq[(q * RA + ir) * HS + ig * OPH + o] = h[q][o];
      }
      __syncthreads();

      const float* hc = hq + row * HS + col;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        const float wt = taps.w[j];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = __builtin_fmaf(wt, hc[(q * RA + j) * HS], v[q]);
      }
    }
    // depth: the window that started NW - 1 planes ago takes its last tap and is complete; every younger one takes its
    // next tap and moves up a slot; a new one starts from zero with tap 0.  The result lands in the slot it moves to, so
    // the ring turns without a copy.
    float m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = __builtin_fmaf(taps.w[NW - 1], v[q], pend[NW - 2][q]);
#pragma unroll
    for (int t = NW - 2; t > 0; --t)
#pragma unroll
      for (int q = 0; q < 5; ++q) pend[t][q] = __builtin_fmaf(taps.w[t], v[q], pend[t - 1][q]);
#pragma unroll
    for (int q = 0; q < 5; ++q) pend[0][q] = __builtin_fmaf(taps.w[0], v[q], 0.0f);
    const int zo = z - (NW - 1);
    if (zo >= 0 && zo < Do) {                                          // uniform
      const float m1 = m[0], m2 = m[1];
      const float mu1 = m1 + cxS, mu2 = m2 + cyS;
      const float s1 = (m[2] - m1 * m1) + d * (2.0f * cx * m1 + cx * cxS);
      const float s2 = (m[3] - m2 * m2) + d * (2.0f * cy * m2 + cy * cyS);
      const float s12 = (m[4] - m1 * m2) + d * ((cy * m1 + cx * m2) + cx * cyS);
      const float cs = (2.0f * s12 + C2) / (s1 + s2 + C2);
      const float ss = ((2.0f * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs;
      t_ssim += valid ? (double)ss : 0.0;
      t_cs += valid ? (double)cs : 0.0;
    }
  }
  double r[3] = {t_ssim, t_cs, sizeof(typename SsimPix<T>::Sq) == 4 ? (double)t_sq_int : t_sq};
  block_sum3_f64(r, s_red);
  if (tid == 0) {
    double* o = partials + ((long)vl * gridDim.y * gridDim.x + (long)ty * gridDim.x + tx) * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
  }
}

size_t ssim3_partial_doubles(int V, int H, int W, int n) {
  return (size_t)3 * V * ((H - n + SSIM3_TH) / SSIM3_TH) * ((W - n + SSIM3_TW) / SSIM3_TW);
}

hipError_t launch_ssim_volumes(const void* x, const void* y, bool is_f32, int V, int D, int H, int W, long xpitch, long xdepth, long xvol,
                               long ypitch, long ydepth, long yvol, const Ssim3Taps& taps, float C1, float C2, double* partials,
                               double* out, hipStream_t s) {
  const dim3 grid((W - taps.n + SSIM3_TW) / SSIM3_TW, (H - taps.n + SSIM3_TH) / SSIM3_TH, V);
  if (is_f32)
    ssim_volumes_kernel<float><<<grid, dim3(256), 0, s>>>((const uint8_t*)x, (const uint8_t*)y, D, H, W, xpitch, xdepth, xvol, ypitch, ydepth,
                                                          yvol, taps, C1, C2, partials);
  else
    ssim_volumes_kernel<uint8_t><<<grid, dim3(256), 0, s>>>((const uint8_t*)x, (const uint8_t*)y, D, H, W, xpitch, xdepth, xvol, ypitch,
                                                            ydepth, yvol, taps, C1, C2, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ssim_sum_kernel<<<dim3((unsigned)V), dim3(256), 0, s>>>(partials, (long)grid.x * grid.y, out);
  return hipGetLastError();
}

// ---- one 5-D MS-SSIM level: F.avg_pool3d(kernel 2, stride 2, padding (D % 2, H % 2, W % 2)), the zero pad counted ---------
// dst [ceil(D / 2)][ceil(H / 2)][ceil(W / 2)]: the window of (k, i, j) starts at (2 k - D % 2, 2 i - H % 2, 2 j - W % 2); a
// plane / row / column -1 is the pad.  The eight values are added depth-major, then row, then column, and the sum is
// multiplied by 0.125.  The last window ends at D - 1 / H - 1 / W - 1: nothing is read beyond the volume.
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_pad3_kernel(const uint8_t* __restrict__ src, int D, int H, int W, long spitch, long sdepth,
                                                            long svol, uint8_t* __restrict__ dst, int Ho, int Wo, long npl, long dpitch,
                                                            long ddepth, long dvol) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npl * Wo) return;
  const long ki = idx / Wo;
  const int j = (int)(idx - ki * Wo), k = (int)(ki / Ho), i = (int)(ki - (long)k * Ho);
  const int d0 = 2 * k - (D & 1), r0 = 2 * i - (H & 1), c0 = 2 * j - (W & 1);
  const uint8_t* base = src + (long)blockIdx.y * svol;
  float sum = 0.0f;
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dr = 0; dr < 2; ++dr) {
      const int zz = d0 + dz, rr = r0 + dr;                             // only zz, rr, c0 == -1 can fall outside
      const T* row = (const T*)(base + (long)(zz < 0 ? 0 : zz) * sdepth + (long)(rr < 0 ? 0 : rr) * spitch);
      const bool in = zz >= 0 && rr >= 0;
      const float v0 = in && c0 >= 0 ? (float)row[c0 < 0 ? 0 : c0] : 0.0f, v1 = in ? (float)row[c0 + 1] : 0.0f;
      sum = (sum + v0) + v1;
    }
  ((float*)(dst + (long)blockIdx.y * dvol + (long)k * ddepth + (long)i * dpitch))[j] = sum * 0.125f;
}

hipError_t launch_avgpool2_pad3(const void* src, bool is_f32, int V, int D, int H, int W, long spitch, long sdepth, long svol, void* dst,
                                long dpitch, long ddepth, long dvol, hipStream_t s) {
  const int Do = (D + 1) / 2, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long npl = (long)Do * Ho;
  const dim3 grid((unsigned)((npl * Wo + 255) / 256), (unsigned)V);
  if (is_f32)
    avgpool2_pad3_kernel<float><<<grid, dim3(256), 0, s>>>((const uint8_t*)src, D, H, W, spitch, sdepth, svol, (uint8_t*)dst, Ho, Wo, npl,
                                                           dpitch, ddepth, dvol);
  else
    avgpool2_pad3_kernel<uint8_t><<<grid, dim3(256), 0, s>>>((const uint8_t*)src, D, H, W, spitch, sdepth, svol, (uint8_t*)dst, Ho, Wo, npl,
                                                             dpitch, ddepth, dvol);
  return hipGetLastError();
}

}  // namespace tmk
