// Training slice: backward kernels of one ResBlock (model/MBAblocks.py:237-299,302-368) --
//   prep_bwd_kernel    backward of  y = Dropout(SiLU(RMSNorm_C(x) * w * (1 + scale) + shift))  (in_layers[0:2], out_layers[0:3])
//   conv_wgrad_kernel  dW of Conv3d(k = 3x3x3 pad 1, Z <= 4) and of the 1x1x1 skip conv
//   chan_sum_kernel    bias gradients (sum over voxels per channel)
// The data gradient of the convs (dgrad) needs no kernel of its own: a stride-1 "same" conv's dgrad is the forward conv of
// dY with the kernel flipped in every axis and cin <-> cout transposed, so it runs on conv3d_mfma / conv1_mfma with weights
// re-packed by the host (tm_op_conv_dgrad in tm_ops.hip).
// fp32 throughout (training in the reference is fp16-mixed on top of fp32 master weights; the slice checks gradients
// against torch.autograd of the fp32 oracle).  Layout: CB8 fp32 [N][Cb][Z][H][W][8] as everywhere.
#include "tm_conv_frag.h"
#include "tm_device.h"

#include <algorithm>
#include <atomic>

namespace tmk {

// ------------------------------------------------------------------------------------------------------------------
// prep backward.  Forward (per voxel v, channel c; img = patch / per_image):
//   xh = x * rstd(v),  rstd = rsqrt(mean_c x^2 + eps)          LlamaRMSNorm(dim=1), MBAblocks.py:21-43
//   n  = xh * w[c]
//   m  = n * (1 + scale[img][c]) + shift[img][c]               apply_conditions, MBAblocks.py:356-367 (optional)
//   s  = SiLU(m);  y = s * mask * drop_scale                   nn.SiLU, nn.Dropout(p) with a SUPPLIED keep mask (optional),
//                                                              or (DRAW) the mask drawn again as the forward drew it (drop_keep8)
// Backward, g = dL/dy:
//   ds = g * mask * drop_scale;  dm = ds * sig(m) * (1 + m * (1 - sig(m)))
//   dscale[img][c] += dm * n;  dshift[img][c] += dm;  dn = dm * (1 + scale)
//   dw[c] += dn * xh;  dxh = dn * w
//   dx = rstd * (dxh - xh * mean_c(dxh * xh))
// lane = voxel, the workgroup's 4 waves split the channel blocks (as prep_kernel); two passes over the channels
// (first: mean_c(dxh * xh), second: dx).  The per-channel sums (dw, dscale, dshift) are reduced in TWO STAGES so that the
// gradients are bitwise reproducible: the 64 voxels of a workgroup in registers (wave_sum), one partial per (workgroup,
// channel) STORED to a scratch slab, and prep_bwd_reduce_kernel adds the slabs of the workgroups in index order -- no float
// atomics (their sum depends on arrival order: the last bits changed from run to run).
// ------------------------------------------------------------------------------------------------------------------
struct PrepBwdArgs {
  const float* x; long x_ns;            // forward input (pre-norm), CB8 with Cb blocks
  const float* g; long g_ns;            // dL/dy, CB8
  const float* mask; long mask_ns;      // keep mask (0 / 1) CB8 or null
  float drop_scale;                     // 1 / (1 - p)
  const float* w;                       // [Cb*8] norm weight (zero in the pad slots)
  const float* scale; const float* shift; long mod_stride; int per_image;   // [img][..] or null
  float* dx; long dx_ns;
  float* part_dw;                       // [workgroups][Cb*8] partial sums of this workgroup's 64 voxels
  float* part_ds; float* part_dh;       // [workgroups][2 (image of lane 0 | the next image)][Cb*8] partial dscale / dshift, or null
  int N, Cb, Z, S; float inv_c;
  unsigned long long drop_key; uint32_t drop_site, drop_thr;    // DRAW only
};

// DRAW: the keep bits of a channel block are drawn once in pass 1 and kept (8 bits per block) for the wave's first 16 channel
// blocks (Cb <= 64, every ResBlock of the model); further blocks draw again in pass 2
template <bool DRAW>
__global__ __launch_bounds__(256) void prep_bwd_kernel(PrepBwdArgs a) {
  __shared__ float red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long vpn = (long)a.Z * a.S * a.S;
  const long vidx = (long)blockIdx.x * 64 + lane;
  const bool valid = vidx < vpn * a.N;
  const int n = valid ? (int)(vidx / vpn) : 0;
  const long off = valid ? (vidx - (long)n * vpn) * 8 : 0;
  const int img = n / a.per_image;
  const long plane = vpn * 8;
  // pass 0: rstd
  float ssq = 0.f;
  if (valid)
    for (int cb = wv; cb < a.Cb; cb += 4) {
      const float* p = a.x + (long)n * a.x_ns + (long)cb * plane + off;
      const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) ssq += v0[j] * v0[j] + v1[j] * v1[j];
    }
  red[wv][lane] = ssq;
  __syncthreads();
  const float rstd = 1.0f / sqrtf((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) * a.inv_c + TM_EPS);
  __syncthreads();
  // dxh for one channel block (recomputed in both passes: cheaper than keeping Cb * 8 values per lane)
  auto block = [&](int cb, uint32_t keep, float (&xh)[8], float (&dxh)[8], float (&dm)[8], float (&nn)[8]) {
    const float* p = a.x + (long)n * a.x_ns + (long)cb * plane + off;
    const float* gp = a.g + (long)n * a.g_ns + (long)cb * plane + off;
    const f32x4 v0 = *(const f32x4*)p, v1 = *(const f32x4*)(p + 4);
    const f32x4 g0 = *(const f32x4*)gp, g1 = *(const f32x4*)(gp + 4);
    f32x4 k0 = {1.f, 1.f, 1.f, 1.f}, k1 = {1.f, 1.f, 1.f, 1.f};
    if (!DRAW && a.mask) { const float* mp = a.mask + (long)n * a.mask_ns + (long)cb * plane + off; k0 = *(const f32x4*)mp; k1 = *(const f32x4*)(mp + 4); }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      const float xv = j < 4 ? v0[j] : v1[j - 4], gv = j < 4 ? g0[j] : g1[j - 4];
      const float kv = DRAW ? (float)((keep >> j) & 1u) : (j < 4 ? k0[j] : k1[j - 4]);
      const float wc = a.w[c];
      const float sc = a.scale ? a.scale[(long)img * a.mod_stride + c] : 0.f;
      const float sh = a.shift ? a.shift[(long)img * a.mod_stride + c] : 0.f;
      xh[j] = xv * rstd;
      nn[j] = xh[j] * wc;
      const float mm = nn[j] * (1.0f + sc) + sh;
      const float sg = 1.0f / (1.0f + expf(-mm));
      const float ds = gv * kv * a.drop_scale;
      dm[j] = ds * sg * (1.0f + mm * (1.0f - sg));
      dxh[j] = dm[j] * (1.0f + sc) * wc;
    }
  };
  // pass 1: mean_c(dxh * xh) per voxel, and the per-channel sums
  float dot = 0.f;
  unsigned long long kb_lo = 0, kb_hi = 0;
  for (int cb = wv, i = 0; cb < a.Cb; cb += 4, ++i) {
    float xh[8], dxh[8], dm[8], nn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { xh[j] = 0.f; dxh[j] = 0.f; dm[j] = 0.f; nn[j] = 0.f; }
    uint32_t keep = 0;
    if (DRAW && valid) {
      keep = drop_keep8(a.drop_key, a.drop_site, (unsigned long long)vidx, cb, a.drop_thr);
      if (i < 8) kb_lo |= (unsigned long long)keep << (8 * i);
      else if (i < 16) kb_hi |= (unsigned long long)keep << (8 * (i - 8));
    }
    if (valid) block(cb, keep, xh, dxh, dm, nn);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      dot += dxh[j] * xh[j];
      // dw[c] = sum_v dn * xh with dn = dm * (1 + scale): dxh * xh = dn * w * xh, so divide the weight back out is
      // avoided by summing dn * xh directly
      const float sc = (a.scale && valid) ? a.scale[(long)img * a.mod_stride + c] : 0.f;
      const float dwv = wave_sum(dm[j] * (1.0f + sc) * xh[j]);
      if (lane == 0) a.part_dw[(long)blockIdx.x * a.Cb * 8 + c] = dwv;
    }
    if (a.part_ds) {
      // the 64 voxels of a wave may belong to two images only at an image boundary: reduce per image of lane 0 and of
      // the last lane (per_image * vpn >= 64, or = 32: two aligned images per workgroup, the collage decoder of patch size 32)
      const int img_lo = __shfl(img, 0, 64);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cb * 8 + j;
        const float s_lo = wave_sum(img == img_lo ? dm[j] * nn[j] : 0.f), h_lo = wave_sum(img == img_lo ? dm[j] : 0.f);
        const float s_hi = wave_sum(img != img_lo ? dm[j] * nn[j] : 0.f), h_hi = wave_sum(img != img_lo ? dm[j] : 0.f);
        if (lane == 0) {
          const long pb = (long)blockIdx.x * 2 * a.Cb * 8;
          a.part_ds[pb + c] = s_lo; a.part_dh[pb + c] = h_lo;
          a.part_ds[pb + a.Cb * 8 + c] = s_hi; a.part_dh[pb + a.Cb * 8 + c] = h_hi;
        }
      }
    }
  }
  red[wv][lane] = dot;
  __syncthreads();
  const float mean_dot = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) * a.inv_c;
  if (!valid) return;
  // pass 2: dx
  for (int cb = wv, i = 0; cb < a.Cb; cb += 4, ++i) {
    float xh[8], dxh[8], dm[8], nn[8];
    uint32_t keep = 0;
    if (DRAW) keep = i < 8 ? (uint32_t)(kb_lo >> (8 * i)) & 0xFFu
                           : (i < 16 ? (uint32_t)(kb_hi >> (8 * (i - 8))) & 0xFFu
                                     : drop_keep8(a.drop_key, a.drop_site, (unsigned long long)vidx, cb, a.drop_thr));
    block(cb, keep, xh, dxh, dm, nn);
    float* dp = a.dx + (long)n * a.dx_ns + (long)cb * plane + off;
    f32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o0[j] = rstd * (dxh[j] - xh[j] * mean_dot); o1[j] = rstd * (dxh[4 + j] - xh[4 + j] * mean_dot); }
    *(f32x4*)dp = o0;
    *(f32x4*)(dp + 4) = o1;
  }
}

// stage 2: out[c] = sum over workgroups (in index order) of part[wg][c]; one thread per channel, eight independent chains
// combined in a fixed order
__global__ __launch_bounds__(64) void prep_bwd_reduce_dw_kernel(const float* part, long nwg, int C8, float* dw) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C8) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  long wg = 0;
  for (; wg + 8 <= nwg; wg += 8)
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] += part[(wg + u) * C8 + c];
  for (int u = 0; wg < nwg; ++wg, ++u) acc[u] += part[wg * C8 + c];
  dw[c] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}
// dscale / dshift[img][c]: the workgroups that hold voxels of image `img` form the index range [img V / 64, ((img + 1) V - 1) / 64]
// (V = per_image * voxels per patch >= 64): a workgroup whose first voxel belongs to `img` contributes its first slab, the
// one workgroup that starts in image img - 1 and ends in img its second slab
__global__ __launch_bounds__(64) void prep_bwd_reduce_mod_kernel(const float* part_ds, const float* part_dh, long nwg, long V, int C8,
                                                                 long mod_stride, float* dscale, float* dshift) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const long img = blockIdx.y;
  if (c >= C8) return;
  const long wa = img * V / 64, wb = ((img + 1) * V - 1) / 64;
  float s_ = 0.f, h_ = 0.f;
  for (long wg = wa; wg <= wb && wg < nwg; ++wg) {
    const long lo = wg * 64 / V;                       // image of the workgroup's first voxel
    const long pb = (wg * 2 + (lo == img ? 0 : 1)) * C8 + c;
    s_ += part_ds[pb];
    h_ += part_dh[pb];
  }
  dscale[img * mod_stride + c] = s_;
  dshift[img * mod_stride + c] = h_;
}

size_t prep_bwd_scratch_floats(int N, int Cb, int Z, int S, bool with_mod) {
  const long nwg = ((long)N * Z * S * S + 63) / 64;
  return (size_t)nwg * Cb * 8 * (with_mod ? 5 : 1);
}

hipError_t launch_prep_bwd(const float* x, long x_ns, const float* g, long g_ns, const float* mask, long mask_ns, float drop_scale,
                           const float* w, const float* scale, const float* shift, long mod_stride, int per_image, float* dx,
                           long dx_ns, float* dw, float* dscale, float* dshift, int N, int Cb, int C_real, int Z, int S,
                           float* scratch, hipStream_t s, const DropRng* rng) {
  // a 64-voxel workgroup may hold voxels of two images at most: images of 64 voxels or more, or of exactly 32 (aligned halves)
  const long vimg = (long)per_image * Z * S * S;
  if (per_image < 1 || (vimg < 64 && vimg != 32) || !scratch) return hipErrorInvalidValue;
  const long vox = (long)N * Z * S * S, nwg = (vox + 63) / 64;
  const int C8 = Cb * 8;
  float* part_dw = scratch;
  float* part_ds = scale ? scratch + nwg * C8 : nullptr;
  float* part_dh = scale ? part_ds + nwg * 2 * C8 : nullptr;
  PrepBwdArgs a{x, x_ns, g, g_ns, mask, mask_ns, drop_scale, w, scale, shift, mod_stride, per_image, dx, dx_ns, part_dw, part_ds, part_dh,
                N, Cb, Z, S, 1.0f / (float)C_real, 0ull, 0u, 0u};
  if (rng) {
    if (mask) return hipErrorInvalidValue;
    a.drop_key = rng->key; a.drop_site = rng->site; a.drop_thr = rng->thr;
    hipLaunchKernelGGL(prep_bwd_kernel<true>, dim3((unsigned)nwg), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(prep_bwd_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((C8 + 63) / 64)), dim3(64), 0, s, part_dw, nwg, C8, dw);
  if (scale) {
    const long nimg = (N + per_image - 1) / per_image;
    hipLaunchKernelGGL(prep_bwd_reduce_mod_kernel, dim3((unsigned)((C8 + 63) / 64), (unsigned)nimg), dim3(64), 0, s, part_ds, part_dh, nwg,
                       (long)per_image * Z * S * S, C8, mod_stride, dscale, dshift);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// Conv3d weight gradient:  dW[co][ci][kz][ky][kx] = sum_{n,z,y,x} dY[n][co][z][y][x] * X[n][ci][z+kz-pz][y+ky-1][x+kx-1]
// (taps 27: 3x3x3 pad 1 on Z planes; taps 1: 1x1x1).  One workgroup per (cout block of 8, cin block of 8): it walks
// every patch in 8 x 8 x Z voxel tiles, stages the dY tile and the halo'd X tile of its two channel blocks in LDS and
// accumulates.  Thread (co, ci, q): q = wave splits the taps (tap t belongs to wave t % 4).  The result is written in the
// reference's parameter layout [Cout][Cin][taps].
// ------------------------------------------------------------------------------------------------------------------
struct WgradArgs {
  const float* x; long x_ns; int Cbi;
  const float* dy; long dy_ns; int Cbo;
  float* dw;                     // [Cout][Cin][taps]
  int N, Z, S, taps, Cout, Cin;
};

__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int T = 8;                              // spatial tile
  __shared__ float xs[4][T + 2][T + 2][8];          // up to 4 z planes of the input tile (Z <= 4 here)
  __shared__ float ys[4][T][T][8];
  const int tid = threadIdx.x, co = tid & 7, ci = (tid >> 3) & 7, q = tid >> 6;
  const int cob = blockIdx.x, cib = blockIdx.y;
  const int S = a.S, Z = a.Z;
  const long plane = (long)Z * S * S * 8;
  float acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = 0.f;
  const int tiles = (S + T - 1) / T;
  for (int n = 0; n < a.N; ++n) {
    const float* xb = a.x + (long)n * a.x_ns + (long)cib * plane;
    const float* yb = a.dy + (long)n * a.dy_ns + (long)cob * plane;
    for (int ty = 0; ty < tiles; ++ty)
      for (int tx = 0; tx < tiles; ++tx) {
        __syncthreads();
        for (int i = tid; i < Z * (T + 2) * (T + 2) * 8; i += 256) {
          const int c8 = i & 7;
          int r = i >> 3;
          const int hx = r % (T + 2); r /= (T + 2);
          const int hy = r % (T + 2);
          const int z = r / (T + 2);
          const int y = ty * T + hy - 1, x = tx * T + hx - 1;
          xs[z][hy][hx][c8] = (y >= 0 && y < S && x >= 0 && x < S) ? xb[((long)(z * S + y) * S + x) * 8 + c8] : 0.f;
        }
        for (int i = tid; i < Z * T * T * 8; i += 256) {
          const int c8 = i & 7;
          int r = i >> 3;
          const int lx = r % T; r /= T;
          const int ly = r % T;
          const int z = r / T;
          const int y = ty * T + ly, x = tx * T + lx;
          ys[z][ly][lx][c8] = (y < S && x < S) ? yb[((long)(z * S + y) * S + x) * 8 + c8] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const int t = q + 4 * i;
          if (t >= a.taps) break;
          const int kz = a.taps == 1 ? 1 : t / 9, ky = a.taps == 1 ? 1 : (t / 3) % 3, kx = a.taps == 1 ? 1 : t % 3;
          float s_ = 0.f;
          for (int z = 0; z < Z; ++z) {
            const int zi = z + kz - 1;
            if (zi < 0 || zi >= Z) continue;
            for (int ly = 0; ly < T; ++ly)
#pragma unroll
              for (int lx = 0; lx < T; ++lx) s_ = fmaf(ys[z][ly][lx][co], xs[zi][ly + ky][lx + kx][ci], s_);
          }
          acc[i] += s_;
        }
      }
  }
  const int oc = cob * 8 + co, ic = cib * 8 + ci;
  if (oc < a.Cout && ic < a.Cin) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int t = q + 4 * i;
      if (t < a.taps) a.dw[((long)oc * a.Cin + ic) * a.taps + t] = acc[i];
    }
  }
}

hipError_t launch_conv_wgrad(const TV& x, const TV& dy, float* dw, int Cin, int Cout, int taps, hipStream_t s) {
  if ((taps != 27 && taps != 1) || x.Z != dy.Z || x.H != dy.H || x.N != dy.N || x.Z > 4 || x.H != x.W) return hipErrorInvalidValue;
  WgradArgs a{x.p, x.nstride, x.Cb, dy.p, dy.nstride, dy.Cb, dw, x.N, x.Z, x.H, taps, Cout, Cin};
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)dy.Cb, (unsigned)x.Cb), dim3(256), 0, s, a);
  return hipGetLastError();
}

// per-channel sum over (n, voxels) of a CB8 tensor: bias gradients.  One workgroup per channel block.
__global__ __launch_bounds__(256) void chan_sum_kernel(const float* x, long x_ns, int N, long vpn, float* out, int C, int accumulate) {
  __shared__ float red[4][8];
  const int cb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  for (long i = tid; i < (long)N * vpn; i += 256) {
    const long n = i / vpn, v = i - n * vpn;
    const float* p = x + n * x_ns + ((long)cb * vpn + v) * 8;
    const f32x4 a0 = *(const f32x4*)p, a1 = *(const f32x4*)(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] += a0[j]; s[4 + j] += a1[j]; }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { s[j] = wave_sum(s[j]); if (lane == 0) red[wv][j] = s[j]; }
  __syncthreads();
  if (tid < 8 && cb * 8 + tid < C) {
    const float v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    out[cb * 8 + tid] = accumulate ? out[cb * 8 + tid] + v : v;
  }
}
hipError_t launch_chan_sum(const TV& x, float* out, int C, hipStream_t s, int accumulate) {
  hipLaunchKernelGGL(chan_sum_kernel, dim3((unsigned)x.Cb), dim3(256), 0, s, x.p, x.nstride, x.N, (long)x.Z * x.H * x.W, out, C, accumulate);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// The same weight gradient on the matrix pipe (v_mfma_f32_32x32x2_f32).  Per tap it is a GEMM with M = cout, N = cin and
// K = voxels: a workgroup owns a 32-cout x 32-cin tile and one chunk of the list of spatial tiles (n, ty, tx); per spatial
// tile (TH x TW in plane, every z plane) it stages dY and the halo'd X of its 4 + 4 channel blocks in LDS, channel-minor
// ([voxel][32 channels]: the two half-waves of an operand read take two adjacent voxels = 64 consecutive floats, no bank
// conflict), and runs one MFMA per (tap, voxel pair).  taps 27: wave q owns the taps t = q + 4 i (7 / 7 / 7 / 6) in 7 x 16
// accumulator registers, and a (tap, z) pair whose input plane z + kz - 1 lies outside [0, Z) is skipped (wave-uniform),
// so the executed tap count is z-aware.  taps 1: the four waves split the voxel pairs and are summed through LDS in the
// order 0, 1, 2, 3.  chunks == 1 writes dW (or adds into it) directly; otherwise the partial goes to
// part[chunk][Cout][Cin][taps] and conv_wgrad_reduce_kernel adds the chunks in index order.  No atomics: the bits are a
// function of the geometry alone (conv_wgrad_chunks).  Pad channel slots of x / dY are zero and rows / columns beyond
// Cout / Cin are never written.
// ------------------------------------------------------------------------------------------------------------------
struct WgradMfmaArgs {
  const float* x; long x_ns; int Cbi;
  const float* dy; long dy_ns; int Cbo;
  float* out;                    // dW [Cout][Cin][taps] (chunks == 1) or the partials [chunk][Cout][Cin][taps]
  int N, Z, S, Cout, Cin;
  int tiles, per, accumulate;    // spatial tiles in all, tiles per chunk; accumulate: direct form adds into dW
};

template <int TAPS, int TH, int TW>
__global__ __launch_bounds__(256) void conv_wgrad_mfma_kernel(WgradMfmaArgs a) {
  constexpr int XH = TH + 2, XW = TW + 2, NA = TAPS == 27 ? 7 : 1;
  __shared__ __attribute__((aligned(16))) float ys[4096];       // [z][TH][TW][32 cout]:  Z * TH * TW <= 128
  __shared__ __attribute__((aligned(16))) float xs[7680];       // [z][XH][XW][32 cin]:   Z * XH * XW <= 240
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = a.S, Z = a.Z;
  const long plane = (long)Z * S * S * 8;
  const int tiy = (S + TH - 1) / TH, tix = (S + TW - 1) / TW;
  f32x16 acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int t0 = blockIdx.z * a.per, t1 = min(t0 + a.per, a.tiles);
  for (int tl = t0; tl < t1; ++tl) {
    const int n = tl / (tiy * tix), rem = tl - n * (tiy * tix), ty = rem / tix, tx = rem - ty * tix;
    __syncthreads();
    for (int i = tid; i < Z * XH * XW * 4; i += 256) {
      const int cbl = i & 3;
      int r = i >> 2;
      const int hx = r % XW; r /= XW;
      const int hy = r % XH;
      const int z = r / XH;
      const int y = ty * TH + hy - 1, x = tx * TW + hx - 1, cb = blockIdx.y * 4 + cbl;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (cb < a.Cbi && y >= 0 && y < S && x >= 0 && x < S) {
        const float* p = a.x + (long)n * a.x_ns + (long)cb * plane + ((long)(z * S + y) * S + x) * 8;
        v0 = *(const f32x4*)p; v1 = *(const f32x4*)(p + 4);
      }
      float* d = xs + ((z * XH + hy) * XW + hx) * 32 + cbl * 8;
      *(f32x4*)d = v0; *(f32x4*)(d + 4) = v1;
    }
    for (int i = tid; i < Z * TH * TW * 4; i += 256) {
      const int cbl = i & 3;
      int r = i >> 2;
      const int lx = r % TW; r /= TW;
      const int ly = r % TH;
      const int z = r / TH;
      const int y = ty * TH + ly, x = tx * TW + lx, cb = blockIdx.x * 4 + cbl;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (cb < a.Cbo && y < S && x < S) {
        const float* p = a.dy + (long)n * a.dy_ns + (long)cb * plane + ((long)(z * S + y) * S + x) * 8;
        v0 = *(const f32x4*)p; v1 = *(const f32x4*)(p + 4);
      }
      float* d = ys + ((z * TH + ly) * TW + lx) * 32 + cbl * 8;
      *(f32x4*)d = v0; *(f32x4*)(d + 4) = v1;
    }
    __syncthreads();
    if (TAPS == 27) {
      for (int z = 0; z < Z; ++z)
        for (int ly = 0; ly < TH; ++ly)
#pragma unroll
          for (int px = 0; px < TW / 2; ++px) {
            const int lx = 2 * px + h;
            const float av = ys[((z * TH + ly) * TW + lx) * 32 + c];
            const float* xb = xs + ((z * XH + ly) * XW + lx) * 32 + c;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
              const int t = q + 4 * i, kz = t / 9, ky = (t / 3) % 3, kx = t % 3, zi = z + kz - 1;
              if (t < 27 && zi >= 0 && zi < Z)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[(((kz - 1) * XH + ky) * XW + kx) * 32], acc[i], 0, 0, 0);
            }
          }
    } else {
      // voxel pair j of the tile belongs to wave j % 4
      for (int j = q; j < Z * TH * TW / 2; j += 4) {
        const int v = 2 * j + h, lx = v % TW, ly = (v / TW) % TH, z = v / (TW * TH);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ys[v * 32 + c], xs[((z * XH + ly + 1) * XW + lx + 1) * 32 + c], acc[0], 0, 0, 0);
      }
    }
  }
  if (TAPS == 1) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(q * 16 + r) * 64 + lane] = acc[0][r];
    __syncthreads();
    if (q == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = ((xs[r * 64 + lane] + xs[(16 + r) * 64 + lane]) + xs[(32 + r) * 64 + lane]) + xs[(48 + r) * 64 + lane];
    }
  }
  // D register r of a lane: row (cout) 8 (r / 4) + 4 h + r % 4, column (cin) c
  const int ic = blockIdx.y * 32 + c;
  float* out = a.out + (gridDim.z > 1 ? (long)blockIdx.z * a.Cout * a.Cin * TAPS : 0);
  const bool add = gridDim.z == 1 && a.accumulate;
  if (TAPS == 27) {
    // 27-tap form: through LDS, 8 cout rows at a time, so that a row of the tile leaves as one run of (cins of the tile) x 27
    // consecutive floats and not as 4-byte stores 108 bytes apart.  xs [8 rows][32 cin][27 taps]: 6912 floats.
    const int ic0 = blockIdx.y * 32, run = min(32, a.Cin - ic0) * 27;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int t = q + 4 * i;
        if (t < 27) {
#pragma unroll
          for (int k = 0; k < 4; ++k) xs[((4 * h + k) * 32 + c) * 27 + t] = acc[i][4 * g + k];
        }
      }
      __syncthreads();
      for (int row = 0; row < 8; ++row) {
        const int oc = blockIdx.x * 32 + 8 * g + row;
        if (oc >= a.Cout) break;
        float* d = out + ((long)oc * a.Cin + ic0) * 27;
        for (int e = tid; e < run; e += 256) d[e] = add ? d[e] + xs[row * 864 + e] : xs[row * 864 + e];
      }
    }
  } else if (ic < a.Cin && q == 0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int t = TAPS == 27 ? q + 4 * i : 0;
      if (t >= TAPS) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int oc = blockIdx.x * 32 + 8 * (r / 4) + 4 * h + (r % 4);
        if (oc < a.Cout) {
          float* d = out + ((long)oc * a.Cin + ic) * TAPS + t;
          *d = add ? *d + acc[i][r] : acc[i][r];
        }
      }
    }
  }
}

// The store of conv_wgrad_mfma_kernel as a function, for the slab form below (that kernel keeps its own text, so that its Z <= 4 code
// objects stay what they were): the 1x1x1 form sums its four waves through LDS in the order 0, 1, 2, 3, then the tile goes
// to dW (chunks == 1: written or added) or to this chunk's partial.  xs: the kernel's X staging array, free by now (6912 floats for 27
// taps, 4096 for one).
template <int TAPS, int NA>
__device__ __forceinline__ void wgrad_mfma_store(const WgradMfmaArgs& a, f32x16 (&acc)[NA], float* xs, int tid, int lane, int c, int h, int q) {
  if (TAPS == 1) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) xs[(q * 16 + r) * 64 + lane] = acc[0][r];
    __syncthreads();
    if (q == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = ((xs[r * 64 + lane] + xs[(16 + r) * 64 + lane]) + xs[(32 + r) * 64 + lane]) + xs[(48 + r) * 64 + lane];
    }
  }
  // D register r of a lane: row (cout) 8 (r / 4) + 4 h + r % 4, column (cin) c
  const int ic = blockIdx.y * 32 + c;
  float* out = a.out + (gridDim.z > 1 ? (long)blockIdx.z * a.Cout * a.Cin * TAPS : 0);
  const bool add = gridDim.z == 1 && a.accumulate;
  if (TAPS == 27) {
    // 27-tap form: through LDS, 8 cout rows at a time, so that a row of the tile leaves as one run of (cins of the tile) x 27
    // consecutive floats and not as 4-byte stores 108 bytes apart.  xs [8 rows][32 cin][27 taps]: 6912 floats.
    const int ic0 = blockIdx.y * 32, run = min(32, a.Cin - ic0) * 27;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int t = q + 4 * i;
        if (t < 27) {
#pragma unroll
          for (int k = 0; k < 4; ++k) xs[((4 * h + k) * 32 + c) * 27 + t] = acc[i][4 * g + k];
        }
      }
      __syncthreads();
      for (int row = 0; row < 8; ++row) {
        const int oc = blockIdx.x * 32 + 8 * g + row;
        if (oc >= a.Cout) break;
        float* d = out + ((long)oc * a.Cin + ic0) * 27;
        for (int e = tid; e < run; e += 256) d[e] = add ? d[e] + xs[row * 864 + e] : xs[row * 864 + e];
      }
    }
  } else if (ic < a.Cin && q == 0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int t = TAPS == 27 ? q + 4 * i : 0;
      if (t >= TAPS) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int oc = blockIdx.x * 32 + 8 * (r / 4) + 4 * h + (r % 4);
        if (oc < a.Cout) {
          float* d = out + ((long)oc * a.Cin + ic) * TAPS + t;
          *d = add ? *d + acc[i][r] : acc[i][r];
        }
      }
    }
  }
}

// The Z = 8 form: z is a tiled dimension.  The tile list is (n, z slab, ty, tx); a slab owns TZ = 4 output planes z0 .. z0 + 3, and the
// 27-tap form stages those 4 dY planes and the 6 X planes z0 - 1 .. z0 + 4 (planes outside [0, Z) are not read, and a (tap, z) pair
// whose X plane lies there is skipped wave-uniformly as above: no MFMA on zeros).  The 1x1x1 form has no halo in any axis: its slab is
// the voxel range of 4 planes.  Wave -> tap split, accumulators, chunking over the tile list and the store are those of the kernel
// above.  LDS: TH x TW = 4 x 4: 8 KB dY + 27 KB X;  4 x 8 (S >= 8): 16 KB dY + 45 KB X (6 x 6 x 10 voxels x 32 channels).
template <int TAPS, int TH, int TW>
__global__ __launch_bounds__(256) void conv_wgrad_mfma_slab_kernel(WgradMfmaArgs a) {
  constexpr int TZ = 4, HALO = TAPS == 27 ? 1 : 0, XH = TH + 2 * HALO, XW = TW + 2 * HALO, XP = TZ + 2 * HALO, NA = TAPS == 27 ? 7 : 1;
  constexpr int NXS = XP * XH * XW * 32, NST = TAPS == 27 ? 6912 : 4096;        // NST: what wgrad_mfma_store needs of xs
  __shared__ __attribute__((aligned(16))) float ys[TZ * TH * TW * 32];          // [zl][TH][TW][32 cout]
  __shared__ __attribute__((aligned(16))) float xs[NXS > NST ? NXS : NST];      // [zp][XH][XW][32 cin], plane zp = z - z0 + HALO
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = a.S, Z = a.Z;
  const long plane = (long)Z * S * S * 8;
  const int tiy = (S + TH - 1) / TH, tix = (S + TW - 1) / TW, slabs = (Z + TZ - 1) / TZ;
  f32x16 acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int t0 = blockIdx.z * a.per, t1 = min(t0 + a.per, a.tiles);
  for (int tl = t0; tl < t1; ++tl) {
    int rem = tl;
    const int tx = rem % tix; rem /= tix;
    const int ty = rem % tiy; rem /= tiy;
    const int z0 = (rem % slabs) * TZ, n = rem / slabs;
    __syncthreads();
    for (int i = tid; i < XP * XH * XW * 4; i += 256) {
      const int cbl = i & 3;
      int r = i >> 2;
      const int hx = r % XW; r /= XW;
      const int hy = r % XH;
      const int zp = r / XH;
      const int z = z0 + zp - HALO, y = ty * TH + hy - HALO, x = tx * TW + hx - HALO, cb = blockIdx.y * 4 + cbl;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (cb < a.Cbi && z >= 0 && z < Z && y >= 0 && y < S && x >= 0 && x < S) {
        const float* p = a.x + (long)n * a.x_ns + (long)cb * plane + ((long)(z * S + y) * S + x) * 8;
        v0 = *(const f32x4*)p; v1 = *(const f32x4*)(p + 4);
      }
      float* d = xs + ((zp * XH + hy) * XW + hx) * 32 + cbl * 8;
      *(f32x4*)d = v0; *(f32x4*)(d + 4) = v1;
    }
    for (int i = tid; i < TZ * TH * TW * 4; i += 256) {
      const int cbl = i & 3;
      int r = i >> 2;
      const int lx = r % TW; r /= TW;
      const int ly = r % TH;
      const int zl = r / TH;
      const int z = z0 + zl, y = ty * TH + ly, x = tx * TW + lx, cb = blockIdx.x * 4 + cbl;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (cb < a.Cbo && z < Z && y < S && x < S) {
        const float* p = a.dy + (long)n * a.dy_ns + (long)cb * plane + ((long)(z * S + y) * S + x) * 8;
        v0 = *(const f32x4*)p; v1 = *(const f32x4*)(p + 4);
      }
      float* d = ys + ((zl * TH + ly) * TW + lx) * 32 + cbl * 8;
      *(f32x4*)d = v0; *(f32x4*)(d + 4) = v1;
    }
    __syncthreads();
    if (TAPS == 27) {
      for (int zl = 0; zl < TZ; ++zl) {
        const int z = z0 + zl;
        if (z >= Z) break;
        for (int ly = 0; ly < TH; ++ly)
#pragma unroll
          for (int px = 0; px < TW / 2; ++px) {
            const int lx = 2 * px + h;
            const float av = ys[((zl * TH + ly) * TW + lx) * 32 + c];
            const float* xb = xs + (((zl + 1) * XH + ly) * XW + lx) * 32 + c;      // X plane z of the slab image, tap (1, 0, 0)
#pragma unroll
            for (int i = 0; i < NA; ++i) {
              const int t = q + 4 * i, kz = t / 9, ky = (t / 3) % 3, kx = t % 3, zi = z + kz - 1;
              if (t < 27 && zi >= 0 && zi < Z)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[(((kz - 1) * XH + ky) * XW + kx) * 32], acc[i], 0, 0, 0);
            }
          }
      }
    } else {
      // voxel pair j of the slab tile belongs to wave j % 4; no halo: dY and X voxel v share the index
      for (int j = q; j < TZ * TH * TW / 2; j += 4) {
        const int v = 2 * j + h;
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ys[v * 32 + c], xs[v * 32 + c], acc[0], 0, 0, 0);
      }
    }
  }
  wgrad_mfma_store<TAPS, NA>(a, acc, xs, tid, lane, c, h, q);
}


__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* part, long nw, int chunks, float* dw, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw) return;
  float s_ = part[i];
  for (int k = 1; k < chunks; ++k) s_ += part[(long)k * nw + i];
  dw[i] = accumulate ? dw[i] + s_ : s_;
}

// in-plane tile of the MFMA weight gradient: 8 x 8 up to Z = 2, 4 x 8 at Z = 3, 4 (LDS), 4 x 4 below S = 8; edge tiles are zero filled
static void wgrad_tile(int Z, int S, int& th, int& tw) {
  tw = S >= 8 ? 8 : 4;
  th = (S >= 8 && Z <= 2) ? 8 : 4;
}
// The tile list: (n, ty, tx) with every z plane in the tile up to Z = 4; at Z = 8 (the slab form) (n, z slab of 4 planes, ty, tx) with
// the 4 x 8 in-plane tile from S = 8 on (61 KB of LDS, two workgroups per CU) and 4 x 4 below.  Returns the number of tiles.
static int wgrad_tiles(int N, int Z, int S, int& th, int& tw) {
  wgrad_tile(Z, S, th, tw);
  if (Z > 4) th = 4;
  return N * ((Z + 3) / 4) * ((S + th - 1) / th) * ((S + tw - 1) / tw);
}
// Chunks of the voxel range: about 1024 workgroups in all, at most one chunk per spatial tile, at most 256, and at most 16 Mi
// floats (64 MB) of 27-tap partials, so that a narrow layer (64 -> 64: a 442 KB dW) does not spend its time writing and
// re-reading copies of dW and the partials stay within the 256 MB last-level cache.  A function of the layer geometry only,
// never of the device: the summation order, and with it every bit of dW, is the same on every box.
int conv_wgrad_chunks(int N, int Z, int S, int Cin, int Cout, int* per_out) {
  int th, tw;
  const int tiles = wgrad_tiles(N, Z, S, th, tw);
  const long ct = (long)((Cout + 31) / 32) * ((Cin + 31) / 32);
  const long cap = (16L << 20) / ((long)Cout * Cin * 27);
  int chunks = (int)std::max<long>(1, std::min<long>(std::min<long>(std::min<long>(256, tiles), 1024 / ct), cap));
  const int per = (tiles + chunks - 1) / chunks;
  chunks = (tiles + per - 1) / per;
  if (per_out) *per_out = per;
  return chunks;
}
size_t conv_wgrad_scratch_floats(int N, int Z, int S, int Cin, int Cout, int taps) {
  const int chunks = conv_wgrad_chunks(N, Z, S, Cin, Cout, nullptr);
  return chunks > 1 ? (size_t)chunks * Cout * Cin * taps : 0;
}
hipError_t launch_conv_wgrad_mfma(const TV& x, const TV& dy, float* dw, int Cin, int Cout, int taps, int accumulate, float* scratch,
                                  hipStream_t s) {
  const int S = x.H, Z = x.Z;
  if ((taps != 27 && taps != 1) || x.Z != dy.Z || x.H != dy.H || x.N != dy.N || Z < 1 || (Z > 4 && Z != 8) || x.H != x.W || dy.H != dy.W || S < 1 ||
      x.N < 1 || Cin < 1 || Cout < 1 || x.Cb != (Cin + 7) / 8 || dy.Cb != (Cout + 7) / 8)
    return hipErrorInvalidValue;
  int th, tw, per;
  const int tiles = wgrad_tiles(x.N, Z, S, th, tw);
  const int chunks = conv_wgrad_chunks(x.N, Z, S, Cin, Cout, &per);
  if (chunks > 1 && !scratch) return hipErrorInvalidValue;
  WgradMfmaArgs a{x.p, x.nstride, x.Cb, dy.p, dy.nstride, dy.Cb, chunks > 1 ? scratch : dw, x.N, Z, S, Cout, Cin, tiles, per, accumulate};
  const dim3 grid((unsigned)((Cout + 31) / 32), (unsigned)((Cin + 31) / 32), (unsigned)chunks);
#define TM_WGRAD(TAPS, TH, TW) hipLaunchKernelGGL((conv_wgrad_mfma_kernel<TAPS, TH, TW>), grid, dim3(256), 0, s, a)
#define TM_WGRAD_SLAB(TAPS, TH, TW) hipLaunchKernelGGL((conv_wgrad_mfma_slab_kernel<TAPS, TH, TW>), grid, dim3(256), 0, s, a)
  if (Z > 4) {
    if (taps == 27) { if (tw == 8) TM_WGRAD_SLAB(27, 4, 8); else TM_WGRAD_SLAB(27, 4, 4); }
    else { if (tw == 8) TM_WGRAD_SLAB(1, 4, 8); else TM_WGRAD_SLAB(1, 4, 4); }
  } else if (taps == 27) {
    if (th == 8) TM_WGRAD(27, 8, 8); else if (tw == 8) TM_WGRAD(27, 4, 8); else TM_WGRAD(27, 4, 4);
  } else {
    if (th == 8) TM_WGRAD(1, 8, 8); else if (tw == 8) TM_WGRAD(1, 4, 8); else TM_WGRAD(1, 4, 4);
  }
#undef TM_WGRAD
#undef TM_WGRAD_SLAB
  if (chunks > 1) {
    const long nw = (long)Cout * Cin * taps;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, scratch, nw, chunks, dw, accumulate);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// Conv weights packed on the device: w [Cout][Cin][taps] (reference layout) -> the bytes conv_pack_host writes for `form`: the
// plain tap order, or for CF_PAIR W1, W2 - W1, W0 - W1 per in-plane tap (plain fp32 subtractions) in the k-half image; pad slots
// zero.  role 1 packs the filter of the data gradient: flipped in every axis and cin <-> cout transposed, so the pack
// has Cin "output" channels over ceil(Cout / 8) "input" blocks.  One thread per packed float.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* w, float* out, int Cout, int Cin, int taps, int role, int form,
                                                        long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int Co = role ? Cin : Cout, Ci = role ? Cout : Cin, Cbi = (Ci + 7) / 8;
  // CF_PAIR: a tap is [2 k-halves][64 cout][4 cin] (conv_w_off, tm_conv_frag.h), every other form [64 cout][8 cin]
  const int c8 = form == CF_PAIR ? (int)(((i >> 8) & 1) * 4 + (i & 3)) : (int)(i & 7);
  const int col = form == CF_PAIR ? (int)((i >> 2) & 63) : (int)((i >> 3) & 63);
  static_assert(conv_w_off(63, 7) == 511 && conv_w_off(5, 6) == 256 + 5 * 4 + 2, "the decode above inverts conv_w_off");
  long r = i >> 9;
  const int t = (int)(r % taps); r /= taps;
  const int cb = (int)(r % Cbi), nt = (int)(r / Cbi);
  const int co = nt * 64 + col, ci = cb * 8 + c8;
  float v = 0.f;
  if (co < Co && ci < Ci) {
    // effective filter e[co][ci][u] = role ? w[ci][co][taps - 1 - u] : w[co][ci][u]
    const float* src = role ? w + ((long)ci * Cin + co) * taps : w + ((long)co * Cin + ci) * taps;
    auto e = [&](int u) { return src[role ? taps - 1 - u : u]; };
    if (form != CF_PAIR) v = e(t);
    else {
      const int k = t % 9, g = t / 9;
      const float w1 = e(9 + k);
      v = g == 0 ? w1 : __fsub_rn(e(g == 1 ? 18 + k : k), w1);
    }
  }
  out[i] = v;
}
hipError_t launch_conv_pack(const float* w, float* out, int Cout, int Cin, int form, int role, hipStream_t s) {
  if (form != CF_1X1 && form != CF_PLANES3 && form != CF_ZSKIP && form != CF_PAIR) return hipErrorInvalidValue;
  const int Co = role ? Cin : Cout, Ci = role ? Cout : Cin, taps = conv_form_taps(form);
  const long total = (long)conv_pack_floats(form, Co, (Ci + 7) / 8);
  hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, out, Cout, Cin, taps, role, form, total);
  return hipGetLastError();
}


// ==================================================================================================================
// AttnBlock training slice (model/MBAblocks.py:428-514,517-601,608-614): elementwise pieces, the per-voxel adaLN
// modulate(norm(x)) backward, and the windowed cross-attention core forward + backward.  fp32, functional (not tuned):
// every Linear of the block is a 1x1x1 conv and runs, forward and backward, on the conv kernels above.
// ==================================================================================================================

// ---- elementwise ops on flat fp32 buffers (CB8 tensors of one geometry) ----
//   0 GATE_ADD  o1 = a + b * c          x + gate * value                         (MBAblocks.py:488-489)
//   1 MUL2      o1 = a * b, o2 = a * c  d(value) = d * gate, d(gate) = d * value
//   2 GELU      o1 = gelu_tanh(a)       timm Mlp act (approx_gelu, MBAblocks.py:18)
//   3 GELU_BWD  o1 = a * gelu_tanh'(b)
//   4 SILU      o1 = silu(a)            adaLN_modulation[0] (MBAblocks.py:463)
//   5 SILU_BWD  o1 = a * silu'(b)
//   6 ADD       o1 = a + b
//   7 MUL4      o1 = 4 a                adjoint of AvgPool(1,2,2) composed from the x2 nearest upsample (and vice versa:
//   8 DIV4      o1 = a / 4              up2^T = 4 avgpool, avgpool^T = up2 / 4)
__global__ __launch_bounds__(256) void ew_kernel(int op, const float* a, const float* b, const float* c, float* o1, float* o2, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float av = a[i];
    switch (op) {
      case 0: o1[i] = av + b[i] * c[i]; break;
      case 1: o1[i] = av * b[i]; o2[i] = av * c[i]; break;
      case 2: o1[i] = gelu_tanh_f(av); break;
      case 3: {
        const float x = b[i], kB = 0.7978845608028654f, kK = 0.044715f;
        const float u = kB * (x + kK * x * x * x), th = tanhf(u);
        o1[i] = av * (0.5f * (1.0f + th) + 0.5f * x * (1.0f - th * th) * kB * (1.0f + 3.0f * kK * x * x));
        break;
      }
      case 4: o1[i] = silu_f(av); break;
      case 5: { const float x = b[i], sg = 1.0f / (1.0f + expf(-x)); o1[i] = av * sg * (1.0f + x * (1.0f - sg)); break; }
      case 6: o1[i] = av + b[i]; break;
      case 7: o1[i] = 4.0f * av; break;
      default: o1[i] = 0.25f * av; break;
    }
  }
}
hipError_t launch_ew(int op, const float* a, const float* b, const float* c, float* o1, float* o2, long n, hipStream_t s) {
  if (op < 0 || op > 8 || !a || !o1 || n < 0) return hipErrorInvalidValue;
  long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(ew_kernel, dim3((unsigned)g), dim3(256), 0, s, op, a, b, c, o1, o2, n);
  return hipGetLastError();
}

// ---- modulate(norm, x, shift, scale) backward with PER-VOXEL shift / scale (MBAblocks.py:608-614) ----
//   forward  y = RMSNorm_C(x) * w * (1 + scale) + shift         scale, shift: CB8 tensors of x's geometry
//   backward dscale = g * n (n = xh * w), dshift = g, dn = g * (1 + scale), dw[c] += sum_v dn * xh,
//            dx = rstd * (dn * w - xh * mean_c(dn * w * xh))
// Same structure as prep_bwd_kernel: lane = voxel, four waves split the channel blocks; dw through the two-stage reduction.
struct ModNormBwdArgs {
  const float* x; const float* g; const float* w; const float* scale;
  float* dx; float* dscale; float* dshift; float* part_dw;
  long ns; int N, Cb, Z, S; float inv_c;
};
__global__ __launch_bounds__(256) void modnorm_bwd_kernel(ModNormBwdArgs a) {
  __shared__ float red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long vpn = (long)a.Z * a.S * a.S;
  const long vidx = (long)blockIdx.x * 64 + lane;
  const bool valid = vidx < vpn * a.N;
  const int n = valid ? (int)(vidx / vpn) : 0;
  const long off = valid ? (vidx - (long)n * vpn) * 8 : 0;
  const long plane = vpn * 8;
  float ssq = 0.f;
  if (valid)
    for (int cb = wv; cb < a.Cb; cb += 4) {
      const float* p = a.x + (long)n * a.ns + (long)cb * plane + off;
#pragma unroll
      for (int j = 0; j < 8; ++j) ssq += p[j] * p[j];
    }
  red[wv][lane] = ssq;
  __syncthreads();
  const float rstd = 1.0f / sqrtf((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) * a.inv_c + TM_EPS);
  __syncthreads();
  float dot = 0.f;
  for (int cb = wv; cb < a.Cb; cb += 4) {
    const long o = (long)n * a.ns + (long)cb * plane + off;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      float xh = 0.f, dn = 0.f;
      if (valid) { xh = a.x[o + j] * rstd; dn = a.g[o + j] * (1.0f + a.scale[o + j]); }
      dot += dn * a.w[c] * xh;
      const float dwv = wave_sum(dn * xh);
      if (lane == 0) a.part_dw[(long)blockIdx.x * a.Cb * 8 + c] = dwv;
    }
  }
  red[wv][lane] = dot;
  __syncthreads();
  const float mean_dot = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) * a.inv_c;
  if (!valid) return;
  for (int cb = wv; cb < a.Cb; cb += 4) {
    const long o = (long)n * a.ns + (long)cb * plane + off;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      const float xh = a.x[o + j] * rstd, gv = a.g[o + j];
      a.dscale[o + j] = gv * xh * a.w[c];
      a.dshift[o + j] = gv;
      a.dx[o + j] = rstd * (gv * (1.0f + a.scale[o + j]) * a.w[c] - xh * mean_dot);
    }
  }
}
hipError_t launch_modnorm_bwd(const TV& x, const float* g, const float* w, const float* scale, float* dx, float* dscale, float* dshift,
                              float* dw, int C_real, float* scratch, hipStream_t s) {
  const long vox = (long)x.N * x.Z * x.H * x.W, nwg = (vox + 63) / 64;
  ModNormBwdArgs a{x.p, g, w, scale, dx, dscale, dshift, scratch, x.nstride, x.N, x.Cb, x.Z, x.H, 1.0f / (float)C_real};
  hipLaunchKernelGGL(modnorm_bwd_kernel, dim3((unsigned)nwg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((x.Cb * 8 + 63) / 64)), dim3(64), 0, s, scratch, nwg, x.Cb * 8, dw);
  return hipGetLastError();
}

// ---- windowed cross-attention core (MBAblocks.py:551-601, n_h = 2, one head): forward and backward ----
//   qh = RMSNorm_C(q) * qw, kh = RMSNorm_C(k) * kw;  S = qh kh^T / C;  P = softmax_j S;  o = P v        per window of
//   T = Z (S/2)^2 tokens (2 x 2 windows over (h, w), all z).  One workgroup per (patch, window), T <= 128, C <= 512.
//   Backward recomputes P:  dv = P^T do;  dP = do v^T;  dS = P (dP - rowsum(dP P)) / C;  dqh = dS kh;  dkh = dS^T qh;
//   RMSNorm backward per token (g = dqh * qw: dq = r g - q r^3 mean_c(g q));  d(qw)[c] = sum_tokens dqh q r -- per-workgroup
//   partials, reduced in index order by prep_bwd_reduce_dw_kernel.
struct AttnTrainArgs {
  const float *q, *k, *v, *qw, *kw, *dout;
  float *o;                            // forward output (BWD == false)
  float *dq, *dk, *dv, *part_qw, *part_kw;
  long ns; int C, Cb, Z, S, T;
};
constexpr int AT_CH = 16;              // channels per staged chunk
template <bool BWD>
__global__ __launch_bounds__(256) void attn_train_kernel(AttnTrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, C = a.C, tid = threadIdx.x;
  float* Pm = sm;                                  // [T][T]
  float* Dm = Pm + (BWD ? T * T : 0);              // [T][T] (backward)
  float* A = Dm + T * T;                           // [T][AT_CH] staged operand (row scaled)
  float* B = A + T * AT_CH;                        // [T][AT_CH]
  float* rq = B + T * AT_CH;                       // [T]
  float* rk = rq + T;
  float* rowdot = rk + T;                          // [T]
  float* pdot = rowdot + T;                        // [T][8] partial dots
  int* tokoff = (int*)(pdot + T * 8);              // [T]
  const int S = a.S, hs = S / 2;
  const int n = blockIdx.x >> 2, win = blockIdx.x & 3, wy = win >> 1, wx = win & 1;
  const long plane = (long)a.Z * S * S * 8;
  const long nb = (long)n * a.ns;
  if (tid < T) {
    const int z = tid / (hs * hs), r = tid - z * hs * hs, yl = r / hs, xl = r - yl * hs;
    tokoff[tid] = ((z * S + wy * hs + yl) * S + wx * hs + xl) * 8;
  }
  __syncthreads();
  auto at = [&](const float* base, int t, int c) -> float { return base[nb + (long)(c >> 3) * plane + tokoff[t] + (c & 7)]; };
  auto put = [&](float* base, int t, int c, float v) { base[nb + (long)(c >> 3) * plane + tokoff[t] + (c & 7)] = v; };
  for (int t = tid; t < 2 * T; t += 256) {
    const float* src = t < T ? a.q : a.k;
    const int tt = t < T ? t : t - T;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) { const float v = at(src, tt, c); ss += v * v; }
    (t < T ? rq : rk)[tt] = 1.0f / sqrtf(ss / (float)C + TM_EPS);
  }
  __syncthreads();
  // stage rows [T][AT_CH] of `src` for channels c0 .. c0 + AT_CH: value * rowscale[t] * colscale[c] (either may be null)
  auto stage = [&](float* dst, const float* src, int c0, const float* rs, const float* cs) {
    for (int e = tid; e < T * AT_CH; e += 256) {
      const int t = e / AT_CH, cc = e - t * AT_CH, c = c0 + cc;
      float v = 0.f;
      if (c < C) { v = at(src, t, c); if (rs) v *= rs[t]; if (cs) v *= cs[c]; }
      dst[e] = v;
    }
  };
  // M[i][j] = sum_c X[i][c] Y[j][c] over all channels (X, Y staged chunk by chunk); thread (ti, tj) owns a TT x TT tile
  const int TT = T / 16, ti = tid >> 4, tj = tid & 15;
  auto gemm_nt = [&](float* M, const float* X, const float* xr, const float* xc, const float* Y, const float* yr, const float* yc, float mul) {
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < C; c0 += AT_CH) {
      __syncthreads();
      stage(A, X, c0, xr, xc);
      stage(B, Y, c0, yr, yc);
      __syncthreads();
      for (int cc = 0; cc < AT_CH; ++cc)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < TT) {
            const float xv = A[(ti * TT + i) * AT_CH + cc];
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (j < TT) acc[i][j] = fmaf(xv, B[(tj * TT + j) * AT_CH + cc], acc[i][j]);
          }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i < TT && j < TT) M[(ti * TT + i) * T + tj * TT + j] = acc[i][j] * mul;
    __syncthreads();
  };
  // P = softmax(qh kh^T / C)
  gemm_nt(Pm, a.q, rq, a.qw, a.k, rk, a.kw, 1.0f / (float)C);
  if (tid < T) {
    float m = -INFINITY;
    for (int j = 0; j < T; ++j) m = fmaxf(m, Pm[tid * T + j]);
    float sum = 0.f;
    for (int j = 0; j < T; ++j) { const float e = expf(Pm[tid * T + j] - m); Pm[tid * T + j] = e; sum += e; }
    const float inv = 1.0f / sum;
    for (int j = 0; j < T; ++j) Pm[tid * T + j] *= inv;
  }
  __syncthreads();
  // out[r][c] = sum_k M(r, k) * Y[k][c] for every channel, M(r, k) = trans ? Mat[k][r] : Mat[r][k]; thread -> (row, channel subset)
  const int NTR = 256 / T, row = tid % T, sub = tid / T, cps = AT_CH / NTR;       // NTR in {2, 4, 8}: cps in {8, 4, 2}
  auto matmul_out = [&](const float* Mat, bool trans, const float* Y, const float* yr, const float* yc, float* out, const float* rdot_src,
                        const float* rdot_w, float* dotacc) {
    for (int c0 = 0; c0 < C; c0 += AT_CH) {
      __syncthreads();
      stage(B, Y, c0, yr, yc);
      __syncthreads();
      for (int u = 0; u < cps; ++u) {
        const int cc = sub * cps + u, c = c0 + cc;
        if (c >= C) {                                    // zero the pad slots of the last channel block (chunks of 16 cover them)
          if (c < a.Cb * 8) put(out, row, c, 0.f);
          continue;
        }
        float s_ = 0.f;
        for (int k = 0; k < T; ++k) s_ = fmaf(trans ? Mat[k * T + row] : Mat[row * T + k], B[k * AT_CH + cc], s_);
        put(out, row, c, s_);
        if (dotacc) *dotacc += s_ * rdot_w[c] * at(rdot_src, row, c);
      }
    }
    __syncthreads();
  };
  if (!BWD) {
    matmul_out(Pm, false, a.v, nullptr, nullptr, a.o, nullptr, nullptr, nullptr);
    return;
  }
  // dv = P^T dout
  matmul_out(Pm, true, a.dout, nullptr, nullptr, a.dv, nullptr, nullptr, nullptr);
  // dP = dout v^T ; dS = P (dP - rowsum(dP P)) / C
  gemm_nt(Dm, a.dout, nullptr, nullptr, a.v, nullptr, nullptr, 1.0f);
  if (tid < T) {
    float rd = 0.f;
    for (int j = 0; j < T; ++j) rd += Dm[tid * T + j] * Pm[tid * T + j];
    rowdot[tid] = rd;
  }
  __syncthreads();
  for (int e = tid; e < T * T; e += 256) { const int i = e / T; Dm[e] = Pm[e] * (Dm[e] - rowdot[i]) / (float)C; }
  __syncthreads();
  // dqh = dS kh (stored in dq for now), partial dots of g q with g = dqh * qw; then the RMSNorm backward in place
  for (int pass = 0; pass < 2; ++pass) {
    const float* Xsrc = pass == 0 ? a.q : a.k;           // the tensor being differentiated
    const float* Ysrc = pass == 0 ? a.k : a.q;           // the other operand (normalised)
    const float* xr = pass == 0 ? rq : rk; const float* yr = pass == 0 ? rk : rq;
    const float* xw = pass == 0 ? a.qw : a.kw; const float* yw = pass == 0 ? a.kw : a.qw;
    float* dX = pass == 0 ? a.dq : a.dk;
    float* part = pass == 0 ? a.part_qw : a.part_kw;
    float mydot = 0.f;
    matmul_out(Dm, pass == 1, Ysrc, yr, yw, dX, Xsrc, xw, &mydot);
    pdot[row * 8 + sub] = mydot;
    __syncthreads();
    if (tid < T) { float d = 0.f; for (int u = 0; u < NTR; ++u) d += pdot[tid * 8 + u]; rowdot[tid] = d / (float)C; }
    __syncthreads();
    // per-channel partial of d(norm weight): sum over the window's tokens of dXh[t][c] * x[t][c] * r[t]   (dXh still in dX)
    for (int c = tid; c < a.Cb * 8; c += 256) {
      float s_ = 0.f;
      if (c < C) for (int t = 0; t < T; ++t) s_ += at(dX, t, c) * at(Xsrc, t, c) * xr[t];
      part[(long)blockIdx.x * a.Cb * 8 + c] = s_;
    }
    __syncthreads();
    // dx = r g - x r^3 mean_c(g x),  g = dXh * w
    for (int e = tid; e < T * C; e += 256) {
      const int t = e / C, c = e - t * C;
      const float r = xr[t], xv = at(Xsrc, t, c);
      put(dX, t, c, r * at(dX, t, c) * xw[c] - xv * r * r * r * rowdot[t]);
    }
    __syncthreads();
  }
}
size_t attn_train_lds_bytes(int T, bool bwd) { return (size_t)((bwd ? 2 : 1) * T * T + 2 * T * AT_CH + 3 * T + T * 8 + T) * 4; }
hipError_t launch_attn_train(const TV& q, const TV& k, const TV& v, const float* qw, const float* kw, const float* dout, float* o,
                             float* dq, float* dk, float* dv, float* dqw, float* dkw, float* scratch, bool bwd, hipStream_t s) {
  const int S = q.H, T = q.Z * (S / 2) * (S / 2);
  if (q.H != q.W || (S & 1) || (T != 32 && T != 64 && T != 128) || q.C > 512 || k.nstride != q.nstride || v.nstride != q.nstride)
    return hipErrorInvalidValue;
  const long nwg = (long)q.N * 4;
  AttnTrainArgs a{q.p, k.p, v.p, qw, kw, dout, o, dq, dk, dv, scratch, scratch ? scratch + nwg * q.Cb * 8 : nullptr, q.nstride, q.C, q.Cb,
                  q.Z, S, T};
  const size_t lds = attn_train_lds_bytes(T, bwd);
  static DevOnce attr_done;
  if (attr_done.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_train_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)attn_train_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_done.mark();
  }
  if (bwd) {
    hipLaunchKernelGGL(attn_train_kernel<true>, dim3((unsigned)nwg), dim3(256), lds, s, a);
    hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((q.Cb * 8 + 63) / 64)), dim3(64), 0, s, a.part_qw, nwg, q.Cb * 8, dqw);
    hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((q.Cb * 8 + 63) / 64)), dim3(64), 0, s, a.part_kw, nwg, q.Cb * 8, dkw);
  } else {
    hipLaunchKernelGGL(attn_train_kernel<false>, dim3((unsigned)nwg), dim3(256), lds, s, a);
  }
  return hipGetLastError();
}

// ---- the same core for short windows (T = 4 / 8 / 16 tokens: the middle-block AttnBlock of rna_slc 1 and of patch size 32) ----
// One workgroup per patch, one wave per window (a patch has exactly four), VALU products.  Lane = (t, blk): t = lane % T its
// token, blk = lane / T one of the NB = 64 / T channel blocks of a staged chunk (CH = 8 NB = 128 / 64 / 32 channels at T = 4 /
// 8 / 16), so a wave stages T x CH = 512 floats of one operand per chunk whatever T is, each lane the 8 channels of one
// (token, channel block) as two float4.  The token map is the (z, h, w) one of attn_train_kernel, computed per lane; nothing is
// assumed about Z.  Pad channels (c >= C) of the last block are masked to zero on every read and written as zero.
//   r_q, r_k       r = rsq(ss / C + eps) (v_rsq_f32, 1 ulp; 1 / C is a host-rounded factor: no IEEE division anywhere).
//   P              logits of the window in LDS [T][T] (element (i, j): lane j + T (i % NB), slot i / NB), softmax per row by the
//                  lane blk == 0 of the row: max, expf(s - m), sum, v_rcp_f32 of the sum, product.
//   o / dv         lane (t, blk) owns out[t][8 channels of its block] of every chunk: sum over the window's tokens.
//   backward       dP = do v^T like the logits; D = rowsum(dP o P) by the row's lane; dS = P (dP - D) / C in LDS;
//                  dqh = dS kh (dkh = dS^T qh) by the owner lane of (t, block) into dq (dk), which also adds its part of
//                  sum_c (dqh qw q) and forms the window's d(q_norm weight) partial; then, the dot complete, the same lane
//                  reads its dqh back and writes dq = r dqh qw - q r^3 dot / C.
// Accumulation orders (what tests/train_short_cases.py derives its bounds from):
//   ss             per lane the channel blocks blk, blk + NB, .. in index order, 8 channels each in order (8 ceil(Cb / NB)
//                  additions), then log2(NB) butterfly levels over the token's lanes (xor T, 2 T, .. 32).
//   logit / dP     one fmaf chain per element over the channels in index order: C terms (pad channels add exact zeros).
//   softmax sum, D one chain over the row's T entries in index order.
//   o, dv, dqh, dkh   one fmaf chain per element over the window's T tokens in index order.
//   dot            sum_c (dqh qw q): per lane its 8 ceil(Cb / NB) channels in the order of ss, then the same butterfly.
//   dqw, dkw       per window: log2(T) butterfly levels over the token lanes (xor 1, .. T / 2); the 4 N window partials in
//                  index order by prep_bwd_reduce_dw_kernel.
// Every output element has one owner lane and one chain: no atomics, two calls give the same bits.
// LDS (static): two staged operands [T][CH + 4] and P, dP [T][T] per wave: 26,880 B (T = 16, backward) .. 17,152 B (T = 4, forward) per
// workgroup.  92 / 134 / 176 VGPRs backward at T = 4 / 8 / 16, no scratch (profiles/attn_train_short.txt).
struct AttnShortArgs {
  const float *q, *k, *v, *qw, *kw, *dout;
  float *o, *dq, *dk, *dv, *part_qw, *part_kw;     // part_*: [patch][window][Cb * 8]
  long ns, plane; int C, Cb, S; float inv_c;
};

template <int T, bool BWD>
__global__ __launch_bounds__(256) void attn_short_kernel(AttnShortArgs a) {
  constexpr int NB = 64 / T, CH = NB * 8, PS = CH + 4, NE = (T + NB - 1) / NB;
  __shared__ __attribute__((aligned(16))) float sA[4][T * PS];
  __shared__ __attribute__((aligned(16))) float sB[4][T * PS];
  __shared__ float sP[4][T * T], sD[4][BWD ? T * T : 1], sRow[4][T];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = lane % T, blk = lane / T;
  float *A = sA[wv], *B = sB[wv], *Pm = sP[wv], *Dm = sD[wv], *rowv = sRow[wv];
  const int S = a.S, hs = S / 2, C = a.C, Cb = a.Cb;
  const long nb = (long)blockIdx.x * a.ns;
  long tok;                                                  // float offset of this lane's token inside a channel block
  {
    const int z = t / (hs * hs), r = t - z * hs * hs, yl = r / hs, xl = r - yl * hs;
    tok = ((long)(z * S + (wv >> 1) * hs + yl) * S + (wv & 1) * hs + xl) * 8;
  }
  // the 8 channels of (this lane's token, channel block cb), pad channels and blocks past the tensor as zeros
  auto load8 = [&](const float* src, int cb, float (&x)[8]) {
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (cb < Cb) { const float* p = src + nb + (long)cb * a.plane + tok; v0 = *(const f32x4*)p; v1 = *(const f32x4*)(p + 4); }
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float v = j < 4 ? v0[j] : v1[j - 4]; x[j] = cb * 8 + j < C ? v : 0.f; }
  };
  auto store8 = [&](float* dst, int cb, const float (&x)[8]) {
    f32x4 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v0[j] = cb * 8 + j < C ? x[j] : 0.f; v1[j] = cb * 8 + 4 + j < C ? x[4 + j] : 0.f; }
    float* p = dst + nb + (long)cb * a.plane + tok;
    *(f32x4*)p = v0;
    *(f32x4*)(p + 4) = v1;
  };
  // sum over the NB lanes of a token
  auto token_sum = [&](float v) {
#pragma unroll
    for (int o = T; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  float rq, rk;
  {
    float sq = 0.f, sk = 0.f;
    for (int cb = blk; cb < Cb; cb += NB) {
      float x[8], y[8];
      load8(a.q, cb, x);
      load8(a.k, cb, y);
#pragma unroll
      for (int j = 0; j < 8; ++j) { sq += x[j] * x[j]; sk += y[j] * y[j]; }
    }
    rq = __builtin_amdgcn_rsqf(token_sum(sq) * a.inv_c + TM_EPS);
    rk = __builtin_amdgcn_rsqf(token_sum(sk) * a.inv_c + TM_EPS);
  }
  // dst[t][blk * 8 ..] = the chunk's values of `src` (first channel block c0b), times r and w[c] when w is given
  auto stage = [&](float* dst, const float* src, int c0b, float r, const float* w) {
    const int cb = c0b + blk;
    float x[8];
    load8(src, cb, x);
    if (w && cb < Cb) {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = x[j] * r * w[cb * 8 + j];
    }
    f32x4 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v0[j] = x[j]; v1[j] = x[4 + j]; }
    *(f32x4*)(dst + t * PS + blk * 8) = v0;
    *(f32x4*)(dst + t * PS + blk * 8 + 4) = v1;
  };
  // M[i][j] = mul * sum_c X[i][c] Y[j][c]; this lane owns j = t and the rows i = blk + u NB
  auto gemm_nt = [&](float* M, const float* X, float xr, const float* xw, const float* Y, float yr, const float* yw, float mul) {
    float acc[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) acc[u] = 0.f;
    for (int c0b = 0; c0b < Cb; c0b += NB) {
      __syncthreads();
      stage(A, X, c0b, xr, xw);
      stage(B, Y, c0b, yr, yw);
      __syncthreads();
#pragma unroll 4
      for (int cc = 0; cc < CH; cc += 4) {
        const f32x4 y = *(const f32x4*)(B + t * PS + cc);
#pragma unroll
        for (int u = 0; u < NE; ++u) {
          const int i = blk + u * NB;
          if (i < T) {
            const f32x4 x = *(const f32x4*)(A + i * PS + cc);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[u] = fmaf(x[j], y[j], acc[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NE; ++u) { const int i = blk + u * NB; if (i < T) M[i * T + t] = acc[u] * mul; }
    __syncthreads();
  };
  // out[t][c] = sum_j M(t, j) Y[j][c], M(t, j) = trans ? Mat[j][t] : Mat[t][j].  With xsrc: `out` receives dXh, the lane adds
  // its share of sum_c (dXh xw x) to `dot` and the window's partial of d(norm weight)[c] = sum_t dXh x xr goes to `part`.
  auto matmul_out = [&](const float* Mat, bool trans, const float* Y, float yr, const float* yw, float* out, const float* xsrc,
                        const float* xw, float xr, float* part, float& dot) {
    for (int c0b = 0; c0b < Cb; c0b += NB) {
      __syncthreads();
      stage(B, Y, c0b, yr, yw);
      __syncthreads();
      const int cb = c0b + blk;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int j = 0; j < T; ++j) {
        const float m = trans ? Mat[j * T + t] : Mat[t * T + j];
        const f32x4 y0 = *(const f32x4*)(B + j * PS + blk * 8), y1 = *(const f32x4*)(B + j * PS + blk * 8 + 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[c] = fmaf(m, y0[c], acc[c]); acc[4 + c] = fmaf(m, y1[c], acc[4 + c]); }
      }
      if (cb < Cb) store8(out, cb, acc);
      if (xsrc) {
        float x[8];
        load8(xsrc, cb, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float w = cb < Cb ? xw[cb * 8 + j] : 0.f;
          dot += acc[j] * w * x[j];
          float pw = acc[j] * x[j] * xr;
#pragma unroll
          for (int o = 1; o < T; o <<= 1) pw += __shfl_xor(pw, o, 64);
          if (t == 0 && cb < Cb) part[((long)blockIdx.x * 4 + wv) * Cb * 8 + cb * 8 + j] = cb * 8 + j < C ? pw : 0.f;
        }
      }
    }
    __syncthreads();
  };
  float nodot = 0.f;
  // P = softmax(qh kh^T / C)
  gemm_nt(Pm, a.q, rq, a.qw, a.k, rk, a.kw, a.inv_c);
  if (blk == 0) {
    float m = -INFINITY;
    for (int j = 0; j < T; ++j) m = fmaxf(m, Pm[t * T + j]);
    float sum = 0.f;
    for (int j = 0; j < T; ++j) { const float e = expf(Pm[t * T + j] - m); Pm[t * T + j] = e; sum += e; }
    const float inv = __builtin_amdgcn_rcpf(sum);
    for (int j = 0; j < T; ++j) Pm[t * T + j] *= inv;
  }
  __syncthreads();
  if (!BWD) {
    matmul_out(Pm, false, a.v, 1.f, nullptr, a.o, nullptr, nullptr, 0.f, nullptr, nodot);
    return;
  }
  // dv = P^T dout
  matmul_out(Pm, true, a.dout, 1.f, nullptr, a.dv, nullptr, nullptr, 0.f, nullptr, nodot);
  // dP = dout v^T;  dS = P (dP - rowsum(dP P)) / C
  gemm_nt(Dm, a.dout, 1.f, nullptr, a.v, 1.f, nullptr, 1.0f);
  if (blk == 0) {
    float rd = 0.f;
    for (int j = 0; j < T; ++j) rd += Dm[t * T + j] * Pm[t * T + j];
    rowv[t] = rd;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int i = blk + u * NB;
    if (i < T) Dm[i * T + t] = Pm[i * T + t] * (Dm[i * T + t] - rowv[i]) * a.inv_c;
  }
  __syncthreads();
  // dqh = dS kh into dq, dkh = dS^T qh into dk; then the RMSNorm backward in place, each lane on the values it wrote
  for (int pass = 0; pass < 2; ++pass) {
    const float* Xsrc = pass == 0 ? a.q : a.k;
    const float* Ysrc = pass == 0 ? a.k : a.q;
    const float xr = pass == 0 ? rq : rk, yr = pass == 0 ? rk : rq;
    const float* xw = pass == 0 ? a.qw : a.kw;
    const float* yw = pass == 0 ? a.kw : a.qw;
    float* dX = pass == 0 ? a.dq : a.dk;
    float dot = 0.f;
    matmul_out(Dm, pass == 1, Ysrc, yr, yw, dX, Xsrc, xw, xr, pass == 0 ? a.part_qw : a.part_kw, dot);
    const float md = token_sum(dot) * a.inv_c, r3 = xr * xr * xr;
    for (int cb = blk; cb < Cb; cb += NB) {
      float g[8], x[8];
      load8(dX, cb, g);
      load8(Xsrc, cb, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = xr * g[j] * xw[cb * 8 + j] - x[j] * r3 * md;
      store8(dX, cb, g);
    }
  }
}

template <int T>
static void launch_attn_short_t(const AttnShortArgs& a, int N, bool bwd, hipStream_t s) {
  if (bwd) hipLaunchKernelGGL((attn_short_kernel<T, true>), dim3((unsigned)N), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_short_kernel<T, false>), dim3((unsigned)N), dim3(256), 0, s, a);
}
hipError_t launch_attn_train_short(const TV& q, const TV& k, const TV& v, const float* qw, const float* kw, const float* dout, float* o,
                                   float* dq, float* dk, float* dv, float* dqw, float* dkw, float* scratch, bool bwd, hipStream_t s) {
  const int S = q.H, T = q.Z * (S / 2) * (S / 2);
  if (q.H != q.W || (S & 1) || (T != 4 && T != 8 && T != 16) || q.C < 1 || q.C > 512 || k.nstride != q.nstride || v.nstride != q.nstride ||
      q.N < 1 || (bwd && !scratch))
    return hipErrorInvalidValue;
  const long nwin = (long)q.N * 4;
  AttnShortArgs a{q.p, k.p, v.p, qw, kw, dout, o, dq, dk, dv, scratch, scratch ? scratch + nwin * q.Cb * 8 : nullptr, q.nstride,
                  (long)q.Z * S * S * 8, q.C, q.Cb, S, 1.0f / (float)q.C};
  if (T == 4) launch_attn_short_t<4>(a, q.N, bwd, s);
  else if (T == 8) launch_attn_short_t<8>(a, q.N, bwd, s);
  else launch_attn_short_t<16>(a, q.N, bwd, s);
  if (bwd) {
    hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((q.Cb * 8 + 63) / 64)), dim3(64), 0, s, a.part_qw, nwin, q.Cb * 8, dqw);
    hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((q.Cb * 8 + 63) / 64)), dim3(64), 0, s, a.part_kw, nwin, q.Cb * 8, dkw);
  }
  return hipGetLastError();
}

// ---- the same core for long windows (T = 256 / 512 tokens: Z = 4 / 8 at the resolution-16 AttnBlocks), fp32 MFMA ----------
// No T x T matrix exists anywhere: tokens are walked in blocks of 128 and every workgroup handles one 128-token block of
// one window against the T / 128 blocks of the other side, through one [128][132] LDS tile.  All four matrix products and
// both logit-like products (qh kh^T, do v^T) run on v_mfma_f32_32x32x2_f32.  Five kernels, launched in this order:
//
//   attn_long_norm_kernel      per voxel (64 per workgroup): qh = (q r) qw, kh = (k r) kw into scratch (CB8, pad channels 0),
//                              r = 1 / sqrt(sum_c x^2 / C + eps); the sum of squares is taken per wave over its channel
//                              blocks in index order, then (w0 + w1 + w2 + w3).
//   attn_long_stats_kernel     workgroup = (patch, window, query block).  Lane = one query (the two half-waves of a query
//                              hold complementary keys).  Pass 1: m = max_j s over all keys.  Pass 2: l = sum_j expf(s - m)
//                              and, backward only, E = sum_j expf(s - m) dP, dP = do . v.  Writes m, 1 / l and
//                              D = E / l = rowsum(dP o P) per query.  Exact two-pass softmax: nothing is rescaled.
//   attn_long_prod_kernel<R>   workgroup = (patch, window, 128-token block of the OWNING side); it alone writes its rows:
//                                R = 0  o   = P  v      owner: query block      R = 2  dv  = P^T  do    owner: key block
//                                R = 1  dqh = dS kh     owner: query block      R = 3  dkh = dS^T qh    owner: key block
//                              For every block of the other side, in index order: logits (and dP for R = 1, 3) by MFMA,
//                              p = expf(s - m) * (1 / l), dS = p (dP - D) / C with the saved m, 1 / l, D of the QUERY of the
//                              pair -- the expression of the stats kernel, no fast-math form anywhere -- into the LDS tile
//                              [own token][other token]; then out^T[c][own] += X^T[c][other] . tile^T, X staged 32 channels
//                              at a time.  dqh / dkh go to dq / dk.
//   attn_long_norm_bwd_kernel  per voxel, in place on dq / dk: g = dxh w;  dx = r g - x r^3 mean_c(g x);  partial of
//                              d(norm weight)[c] = wave_sum over the workgroup's 64 voxels of dxh x r.
//   prep_bwd_reduce_dw_kernel  the per-workgroup partials in index order (as modnorm_bwd).
//
// Accumulation orders (what tests/test_gpu_window_attn_train_long.py derives its bounds from):
//   logit / dP   one MFMA chain per element over the channel blocks in index order; step (cb, kk) adds channels
//                cb * 8 + kk and cb * 8 + 4 + kk: C terms (the pad channels of the last block add exact zeros).
//   m, l, E      per lane the 64 values of a key block in (ct, r) register order, plus the other half-wave's partial
//                (lane ^ 32); the blocks' partials are added in block order: T terms, depth 64 + 1 + T / 128.
//   o, dv, dqh, dkh   one MFMA chain per element: other-side blocks in index order, inside a block tokens u0 + kk and
//                u0 + 4 + kk per step, u0 = 0, 8, ..: T terms.
// Every element of o, dq, dk, dv has one owning workgroup and one chain: no atomics, two calls give the same bits.
// LDS (dynamic): tile 128 * 132 + X^T 32 * 132 + token offsets T + (m, 1 / l, D) 3 T floats = 88,576 B at T = 256 and
// 92,672 B at T = 512.  C <= 256 (eight 32-channel accumulator tiles per lane).
// The tile is lane-private staging, not shared state: a lane writes columns ct * 32 + 8 g + 4 h + j of its own token's row and
// reads back exactly those (u0 + 4 h + kk) -- it turns the logit accumulators' register layout into the B operand's k order;
// only X^T crosses waves.  Its 67,584 B hold the product kernels at one workgroup per CU, which the 134 - 164 VGPRs + 192 - 256
// AGPRs per lane (one wave per SIMD) do anyway: shrinking the tile alone buys no occupancy.
struct AttnLongArgs {
  const float *q, *k, *v, *qh, *kh, *dout, *qw, *kw;
  float *stats;                         // [patch][window][3][T]: m, 1 / l, D
  float *o, *dq, *dk, *dv;
  long ns, plane; int N, C, Cb, Z, S;
};
constexpr int AL_PS = 132;              // row pitch (floats) of the LDS tile and of an X^T row

// per voxel: xh = (x r) w for q (blockIdx.y = 0) and k (1)
__global__ __launch_bounds__(256) void attn_long_norm_kernel(AttnLongArgs a, float* qh, float* kh) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* x = blockIdx.y ? a.k : a.q;
  const float* w = blockIdx.y ? a.kw : a.qw;
  float* y = blockIdx.y ? kh : qh;
  const long vpn = a.plane / 8, vidx = (long)blockIdx.x * 64 + lane;
  const bool valid = vidx < vpn * a.N;
  const int n = valid ? (int)(vidx / vpn) : 0;
  const long base = (long)n * a.ns + (valid ? (vidx - (long)n * vpn) * 8 : 0);
  float ssq = 0.f;
  if (valid)
    for (int cb = wv; cb < a.Cb; cb += 4)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float v = cb * 8 + j < a.C ? x[base + (long)cb * a.plane + j] : 0.f; ssq += v * v; }
  red[wv][lane] = ssq;
  __syncthreads();
  const float r = 1.0f / sqrtf((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)a.C + TM_EPS);
  if (!valid) return;
  for (int cb = wv; cb < a.Cb; cb += 4)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      y[base + (long)cb * a.plane + j] = c < a.C ? x[base + (long)cb * a.plane + j] * r * w[c] : 0.f;
    }
}

// token t of window (wy, wx) -> float offset inside one channel block: tokens in (z, h, w) order
__device__ __forceinline__ void attn_long_tokoff(int* tokoff, int T, int S, int win) {
  const int hs = S / 2, wy = win >> 1, wx = win & 1;
  for (int t = threadIdx.x; t < T; t += 256) {
    const int z = t / (hs * hs), r = t - z * hs * hs, yl = r / hs, xl = r - yl * hs;
    tokoff[t] = ((z * S + wy * hs + yl) * S + wx * hs + xl) * 8;
  }
}
// acc[ct][r] = sum_c own[c] * other[oblk * 128 + ct * 32 + (r & 3) + 8 (r >> 2) + 4 h][c]: lane = own token, registers = the
// tokens of the other side's block.  ownp / otherb: CB8 tensors of one patch; channels >= C count as zero on both
// sides (v and dout are the caller's tensors: a NaN in a pad slot must not reach 0 * NaN).
__device__ __forceinline__ void attn_long_dots(f32x16 (&acc)[4], const float* ownp, const float* otherb, const int* tokoff, int oblk,
                                               int C, int Cb, long plane) {
  const int i32 = threadIdx.x & 31, h = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  const float* op[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) op[ct] = otherb + tokoff[oblk * 128 + ct * 32 + i32] + 4 * h;
  f32x4 wn = *(const f32x4*)(ownp + 4 * h), on[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) on[ct] = *(const f32x4*)op[ct];
  for (int cb = 0; cb < Cb; ++cb) {
    f32x4 wf = wn, of[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) of[ct] = on[ct];
    if (cb * 8 + 8 > C) {                  // the last block's pad channels: exact zeros on both sides, whatever the slots hold
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bool in = cb * 8 + 4 * h + kk < C;
        wf[kk] = in ? wf[kk] : 0.f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) of[ct][kk] = in ? of[ct][kk] : 0.f;
      }
    }
    if (cb + 1 < Cb) {
      const long po = (long)(cb + 1) * plane;
      wn = *(const f32x4*)(ownp + 4 * h + po);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) on[ct] = *(const f32x4*)(op[ct] + po);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(of[ct][kk], wf[kk], acc[ct], 0, 0, 0);
  }
}

template <int T, bool BWD>
__global__ __launch_bounds__(256) void attn_long_stats_kernel(AttnLongArgs a) {
#pragma clang fp contract(off)          // s / C - m, e * dP stay separate roundings here and in the product kernel: one P
  constexpr int NB = T / 128;
  __shared__ int tokoff[T];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i32 = lane & 31;
  const int qblk = blockIdx.x % NB, win = (blockIdx.x / NB) & 3, n = blockIdx.x / (4 * NB);
  attn_long_tokoff(tokoff, T, a.S, win);
  __syncthreads();
  const long nb = (long)n * a.ns;
  const int qt = qblk * 128 + wv * 32 + i32;
  const float invC = 1.0f / (float)a.C;
  f32x16 sa[4], da[4];
  float m = -INFINITY;
  for (int kblk = 0; kblk < NB; ++kblk) {
    attn_long_dots(sa, a.qh + nb + tokoff[qt], a.kh + nb, tokoff, kblk, a.C, a.Cb, a.plane);
    float bm = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) bm = fmaxf(bm, sa[ct][r] * invC);
    m = fmaxf(m, fmaxf(bm, __shfl_xor(bm, 32, 64)));
  }
  float l = 0.f, E = 0.f;
  for (int kblk = 0; kblk < NB; ++kblk) {
    attn_long_dots(sa, a.qh + nb + tokoff[qt], a.kh + nb, tokoff, kblk, a.C, a.Cb, a.plane);
    if (BWD) attn_long_dots(da, a.dout + nb + tokoff[qt], a.v + nb, tokoff, kblk, a.C, a.Cb, a.plane);
    float bs = 0.f, be = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = expf(sa[ct][r] * invC - m);
        bs += e;
        if (BWD) be += e * da[ct][r];
      }
    l += bs + __shfl_xor(bs, 32, 64);
    if (BWD) E += be + __shfl_xor(be, 32, 64);
  }
  if (lane < 32) {
    float* st = a.stats + ((long)n * 4 + win) * 3 * T;
    const float inv = 1.0f / l;
    st[qt] = m; st[T + qt] = inv; st[2 * T + qt] = BWD ? E * inv : 0.f;
  }
}

// ROLE 0: o = P v;  1: dqh = dS kh;  2: dv = P^T do;  3: dkh = dS^T qh   (see the header above)
template <int T, int ROLE>
__global__ __launch_bounds__(256) void attn_long_prod_kernel(AttnLongArgs a) {
#pragma clang fp contract(off)
  constexpr int NB = T / 128, PS = AL_PS;
  constexpr bool OWN_Q = ROLE < 2, NEED_DS = (ROLE & 1) != 0;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Pm = sm;                          // [128 own tokens][PS]: P or dS against the current block of the other side
  float* Xt = Pm + 128 * PS;               // [32 channels][PS]: X^T of the current block
  int* tokoff = (int*)(Xt + 32 * PS);      // [T]
  float* st = (float*)(tokoff + T);        // [3][T]: m, 1 / l, D of every query of the window
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i32 = lane & 31, h = lane >> 5;
  const int blk = blockIdx.x % NB, win = (blockIdx.x / NB) & 3, n = blockIdx.x / (4 * NB);
  attn_long_tokoff(tokoff, T, a.S, win);
  for (int i = tid; i < 3 * T; i += 256) st[i] = a.stats[((long)n * 4 + win) * 3 * T + i];
  __syncthreads();
  const long nb = (long)n * a.ns;
  const int C = a.C, Cb = a.Cb;
  const int ownloc = wv * 32 + i32, ownt = blk * 128 + ownloc, ownoff = tokoff[ownt];
  const float invC = 1.0f / (float)C;
  const float* s_own = (OWN_Q ? a.qh : a.kh) + nb + ownoff;       // logits: own . other
  const float* s_oth = (OWN_Q ? a.kh : a.qh) + nb;
  const float* d_own = (OWN_Q ? a.dout : a.v) + nb + ownoff;      // dP: do . v
  const float* d_oth = (OWN_Q ? a.v : a.dout) + nb;
  const float* X = (ROLE == 0 ? a.v : ROLE == 1 ? a.kh : ROLE == 2 ? a.dout : a.qh) + nb;
  float* out = (ROLE == 0 ? a.o : ROLE == 1 ? a.dq : ROLE == 2 ? a.dv : a.dk) + nb;
  f32x16 sa[4], da[4], oc[8];
#pragma unroll
  for (int tI = 0; tI < 8; ++tI)
#pragma unroll
    for (int r = 0; r < 16; ++r) oc[tI][r] = 0.f;
  const int su = tid & 127, scb = tid >> 7;                        // X staging: token su of the block, channel blocks scb, scb + 2
  float* prow = Pm + ownloc * PS;
  const float* pfrag = prow + 4 * h;                               // B operand: tile[own][other0 + 4h ..]
  const float* xfrag = Xt + i32 * PS + 4 * h;                      // A operand: X^T[channel][other0 + 4h ..]
  for (int oblk = 0; oblk < NB; ++oblk) {
    attn_long_dots(sa, s_own, s_oth, tokoff, oblk, C, Cb, a.plane);
    if (NEED_DS) attn_long_dots(da, d_own, d_oth, tokoff, oblk, C, Cb, a.plane);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int qi = OWN_Q ? ownt : oblk * 128 + ct * 32 + 8 * g + 4 * h + j;     // the query of this pair
          const float p = expf(sa[ct][4 * g + j] * invC - st[qi]) * st[T + qi];
          pk[j] = NEED_DS ? p * (da[ct][4 * g + j] - st[2 * T + qi]) * invC : p;
        }
        *(f32x4*)(prow + ct * 32 + 8 * g + 4 * h) = pk;
      }
    const float* xsrc = X + tokoff[oblk * 128 + su];
    for (int c0 = 0; c0 < C; c0 += 32) {
      __syncthreads();                                             // X^T free (the tile needs no barrier: lane-private, see header)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int cb = c0 / 8 + scb + 2 * half;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (cb < Cb) { v0 = *(const f32x4*)(xsrc + (long)cb * a.plane); v1 = *(const f32x4*)(xsrc + (long)cb * a.plane + 4); }
        float* d = Xt + ((scb + 2 * half) * 8) * PS + su;
        d[0 * PS] = v0[0]; d[1 * PS] = v0[1]; d[2 * PS] = v0[2]; d[3 * PS] = v0[3];
        d[4 * PS] = v1[0]; d[5 * PS] = v1[1]; d[6 * PS] = v1[2]; d[7 * PS] = v1[3];
      }
      __syncthreads();
      const int tI = c0 / 32;
#pragma unroll
      for (int cc = 0; cc < 8; ++cc)
        if (cc == tI) {
#pragma unroll 4
          for (int u0 = 0; u0 < 128; u0 += 8) {
            const f32x4 af = *(const f32x4*)(xfrag + u0), bf = *(const f32x4*)(pfrag + u0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) oc[cc] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bf[kk], oc[cc], 0, 0, 0);
          }
        }
    }
    __syncthreads();                                               // X^T consumed before the next block restages it
  }
  // lane = own token; accumulator quad g of tile tI = channels tI * 32 + 8 g + 4 h .. + 3; pad channels are written as zeros
#pragma unroll
  for (int tI = 0; tI < 8; ++tI)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cb = tI * 4 + g, c = cb * 8 + 4 * h;
      if (cb < Cb)
        *(f32x4*)(out + ownoff + (long)cb * a.plane + 4 * h) = f32x4{c < C ? oc[tI][4 * g] : 0.f, c + 1 < C ? oc[tI][4 * g + 1] : 0.f,
                                                                    c + 2 < C ? oc[tI][4 * g + 2] : 0.f, c + 3 < C ? oc[tI][4 * g + 3] : 0.f};
    }
}

// per voxel (64 per workgroup, a wave per channel block): the RMSNorm backward in place on dx (holding dxh), q (y = 0) / k (1)
__global__ __launch_bounds__(256) void attn_long_norm_bwd_kernel(AttnLongArgs a, float* part_q, float* part_k) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* x = blockIdx.y ? a.k : a.q;
  const float* w = blockIdx.y ? a.kw : a.qw;
  float* dx = blockIdx.y ? a.dk : a.dq;
  float* part = blockIdx.y ? part_k : part_q;
  const long vpn = a.plane / 8, vidx = (long)blockIdx.x * 64 + lane;
  const bool valid = vidx < vpn * a.N;
  const int n = valid ? (int)(vidx / vpn) : 0;
  const long base = (long)n * a.ns + (valid ? (vidx - (long)n * vpn) * 8 : 0);
  float ssq = 0.f;
  if (valid)
    for (int cb = wv; cb < a.Cb; cb += 4)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float v = cb * 8 + j < a.C ? x[base + (long)cb * a.plane + j] : 0.f; ssq += v * v; }
  red[wv][lane] = ssq;
  __syncthreads();
  const float r = 1.0f / sqrtf((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)a.C + TM_EPS);
  __syncthreads();
  float dot = 0.f;
  for (int cb = wv; cb < a.Cb; cb += 4)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      float g = 0.f, xv = 0.f;
      if (valid && c < a.C) { g = dx[base + (long)cb * a.plane + j]; xv = x[base + (long)cb * a.plane + j]; }
      dot += g * w[c] * xv;
      const float pw = wave_sum(g * xv * r);
      if (lane == 0) part[(long)blockIdx.x * a.Cb * 8 + c] = pw;
    }
  red[wv][lane] = dot;
  __syncthreads();
  const float mean_dot = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)a.C;
  if (!valid) return;
  for (int cb = wv; cb < a.Cb; cb += 4)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cb * 8 + j;
      const long o = base + (long)cb * a.plane + j;
      dx[o] = c < a.C ? r * dx[o] * w[c] - x[o] * r * r * r * mean_dot : 0.f;
    }
}

size_t attn_train_long_scratch_floats(int N, int Cb, int Z, int S, bool bwd) {
  const size_t vox = (size_t)N * Z * S * S;                         // qh, kh; m, 1 / l, D; the two norm-weight partials
  return 2 * vox * Cb * 8 + 3 * vox + (bwd ? 2 * ((vox + 63) / 64) * Cb * 8 : 0);
}
template <int T>
static hipError_t launch_attn_train_long_t(AttnLongArgs a, float* dqw, float* dkw, float* scratch, bool bwd, hipStream_t s) {
  const size_t vox = (size_t)a.N * a.Z * a.S * a.S, nv = (vox + 63) / 64;
  const int Cp = a.Cb * 8;
  float *qh = scratch, *kh = qh + vox * Cp, *part_q = kh + vox * Cp + 3 * vox, *part_k = part_q + nv * Cp;
  a.qh = qh; a.kh = kh; a.stats = kh + vox * Cp;
  const size_t lds = ((size_t)(128 + 32) * AL_PS + 4 * T) * sizeof(float);
  static DevOnce attr_done;
  if (attr_done.need()) {
    const void* f[4] = {(const void*)attn_long_prod_kernel<T, 0>, (const void*)attn_long_prod_kernel<T, 1>,
                        (const void*)attn_long_prod_kernel<T, 2>, (const void*)attn_long_prod_kernel<T, 3>};
    for (const void* fn : f) {
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) return e;
    }
    attr_done.mark();
  }
  const dim3 gv((unsigned)nv, 2), gw((unsigned)(a.N * 4 * (T / 128)));
  hipLaunchKernelGGL(attn_long_norm_kernel, gv, dim3(256), 0, s, a, qh, kh);
  if (!bwd) {
    hipLaunchKernelGGL((attn_long_stats_kernel<T, false>), gw, dim3(256), 0, s, a);
    hipLaunchKernelGGL((attn_long_prod_kernel<T, 0>), gw, dim3(256), lds, s, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((attn_long_stats_kernel<T, true>), gw, dim3(256), 0, s, a);
  hipLaunchKernelGGL((attn_long_prod_kernel<T, 1>), gw, dim3(256), lds, s, a);
  hipLaunchKernelGGL((attn_long_prod_kernel<T, 2>), gw, dim3(256), lds, s, a);
  hipLaunchKernelGGL((attn_long_prod_kernel<T, 3>), gw, dim3(256), lds, s, a);
  hipLaunchKernelGGL(attn_long_norm_bwd_kernel, gv, dim3(256), 0, s, a, part_q, part_k);
  hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((Cp + 63) / 64)), dim3(64), 0, s, part_q, (long)nv, Cp, dqw);
  hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((Cp + 63) / 64)), dim3(64), 0, s, part_k, (long)nv, Cp, dkw);
  return hipGetLastError();
}
hipError_t launch_attn_train_long(const TV& q, const TV& k, const TV& v, const float* qw, const float* kw, const float* dout, float* o,
                                  float* dq, float* dk, float* dv, float* dqw, float* dkw, float* scratch, bool bwd, hipStream_t s) {
  const int S = q.H, T = q.Z * (S / 2) * (S / 2);
  if (q.H != q.W || (S & 1) || (T != 256 && T != 512) || q.C > 256 || k.nstride != q.nstride || v.nstride != q.nstride || !scratch)
    return hipErrorInvalidValue;
  AttnLongArgs a{q.p, k.p, v.p, nullptr, nullptr, dout, qw, kw, nullptr, o, dq, dk, dv, q.nstride, q.plane(), q.N, q.C, q.Cb, q.Z, S};
  return T == 256 ? launch_attn_train_long_t<256>(a, dqw, dkw, scratch, bwd, s) : launch_attn_train_long_t<512>(a, dqw, dkw, scratch, bwd, s);
}


// ==================================================================================================================
// Small dense pieces of the training path that are not convs over the patch volume: the Linears over [tokens][features]
// rows (time embedding, ResBlock.emb_layers, the gene-gene AttnBlock of model/unet_ours.py:277-323) and that block's
// row-wise RMSNorm / softmax.  fp32 VALU, deterministic (no split-K, fixed-order reductions).
// ==================================================================================================================

// C[b](m, n) = alpha * sum_k A[b](m, k) * B[b](k, n) (+ bias) (+ C): every operand through element strides, so the same kernel
// serves y = x W^T, dx = dy W, dW = dy^T x, q q^T, P v and their transposes.  64 x 64 tile per workgroup, 4 x 4 per thread.
struct GemmArgs {
  const float *A, *B, *bias; float* C;
  int M, N, K;
  long sam, sak, sbk, sbn, scm, scn, sab, sbb, scb;
  int bias_mode;      // 0 none, 1 bias[n], 2 bias[m]
  int accumulate;     // C += ...
  float alpha;
};
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmArgs a) {
  __shared__ float As[16][65], Bs[16][65];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const float* A = a.A + (long)blockIdx.z * a.sab;
  const float* B = a.B + (long)blockIdx.z * a.sbb;
  float* Cp = a.C + (long)blockIdx.z * a.scb;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < a.K; k0 += 16) {
    for (int e = tid; e < 16 * 64; e += 256) {
      const int kk = e >> 6, r = e & 63;
      const int k = k0 + kk;
      As[kk][r] = (k < a.K && m0 + r < a.M) ? A[(long)(m0 + r) * a.sam + (long)k * a.sak] : 0.f;
      Bs[kk][r] = (k < a.K && n0 + r < a.N) ? B[(long)k * a.sbk + (long)(n0 + r) * a.sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { av[i] = As[kk][ty * 4 + i]; bv[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
      if (m >= a.M || n >= a.N) continue;
      float v = acc[i][j] * a.alpha;
      if (a.bias_mode == 1) v += a.bias[n];
      else if (a.bias_mode == 2) v += a.bias[m];
      float* c = Cp + (long)m * a.scm + (long)n * a.scn;
      *c = a.accumulate ? *c + v : v;
    }
}
hipError_t launch_gemm_f32(const float* A, const float* B, const float* bias, float* C, int M, int N, int K, const long* st, int batch,
                           int bias_mode, int accumulate, float alpha, hipStream_t s) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1 || batch < 1 || (bias_mode && !bias)) return hipErrorInvalidValue;
  GemmArgs a{A, B, bias, C, M, N, K, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], bias_mode, accumulate, alpha};
  hipLaunchKernelGGL(gemm_f32_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64), (unsigned)batch), dim3(256), 0, s, a);
  return hipGetLastError();
}

// Row-wise ops on [rows][D] fp32 (one wave per row, four rows per workgroup):
//   0 RMSNORM      y = x * rsqrt(mean_d x^2 + eps) * w                                  (LlamaRMSNorm dim=-1, MBAblocks.py:35-43)
//   1 RMSNORM_BWD  dx = r (g w - xh mean_d(g w xh)),  part[wg][d] = sum over the workgroup's rows of g * xh
//   2 SOFTMAX      y = softmax_d(x)
//   3 SOFTMAX_BWD  dx = y_saved * (g - sum_d g y_saved)      (x = the saved probabilities)
__global__ __launch_bounds__(256) void rows_kernel(int op, const float* x, const float* w, const float* g, float* y, float* part, long rows,
                                                   int D) {
  extern __shared__ float sh[];                      // op 1: [4][D] per-row products
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long r = (long)blockIdx.x * 4 + wv;
  const bool live = r < rows;
  const float* xr = x + (live ? r : 0) * D;
  if (op == 0 || op == 1) {
    float ss = 0.f;
    if (live) for (int d = lane; d < D; d += 64) ss += xr[d] * xr[d];
    ss = wave_sum(ss);
    const float rstd = 1.0f / sqrtf(ss / (float)D + TM_EPS);
    if (op == 0) {
      if (live) for (int d = lane; d < D; d += 64) y[r * D + d] = xr[d] * rstd * w[d];
      return;
    }
    float dot = 0.f;
    if (live) for (int d = lane; d < D; d += 64) dot += g[r * D + d] * w[d] * xr[d] * rstd;
    dot = wave_sum(dot) / (float)D;
    for (int d = lane; d < D; d += 64) {
      float pv = 0.f;
      if (live) {
        const float xh = xr[d] * rstd, gv = g[r * D + d];
        y[r * D + d] = rstd * (gv * w[d] - xh * dot);
        pv = gv * xh;
      }
      sh[wv * D + d] = pv;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) part[(long)blockIdx.x * D + d] = (sh[d] + sh[D + d]) + (sh[2 * D + d] + sh[3 * D + d]);
    return;
  }
  if (!live) return;
  if (op == 2) {
    float m = -INFINITY;
    for (int d = lane; d < D; d += 64) m = fmaxf(m, xr[d]);
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.f;
    for (int d = lane; d < D; d += 64) sum += expf(xr[d] - m);
    sum = wave_sum(sum);
    for (int d = lane; d < D; d += 64) y[r * D + d] = expf(xr[d] - m) / sum;
  } else {
    float dot = 0.f;
    for (int d = lane; d < D; d += 64) dot += g[r * D + d] * xr[d];
    dot = wave_sum(dot);
    for (int d = lane; d < D; d += 64) y[r * D + d] = xr[d] * (g[r * D + d] - dot);
  }
}
hipError_t launch_rows(int op, const float* x, const float* w, const float* g, float* y, float* dw, float* scratch, long rows, int D,
                       hipStream_t s) {
  if (op < 0 || op > 3 || !x || !y || rows < 1 || D < 1 || D > (op == 1 ? 4096 : 8192)) return hipErrorInvalidValue;   // op 1: 4 * D floats of LDS
  if ((op <= 1 && !w) || ((op == 1 || op == 3) && !g) || (op == 1 && (!dw || !scratch))) return hipErrorInvalidValue;
  const long nwg = (rows + 3) / 4;
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)nwg), dim3(256), op == 1 ? (size_t)4 * D * sizeof(float) : 0, s, op, x, w, g, y, scratch, rows, D);
  if (op == 1) hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3((unsigned)((D + 63) / 64)), dim3(64), 0, s, scratch, nwg, D, dw);
  return hipGetLastError();
}


// ==================================================================================================================
// Optimizer step of the reference's training loop (experiment.py:207-219, 394-414): torch.nn.utils.clip_grad_norm_ over all
// parameters, then torch.optim.Adam(lr, weight_decay) -- on one flat fp32 arena of parameters / gradients / moments.
// ==================================================================================================================

// part[wg] = sum of squares of this workgroup's grid-stride share, then one thread adds the partials in index order
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* x, long n, float* part) {
  __shared__ float red[4];
  float s_ = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s_ = fmaf(x[i], x[i], s_);
  s_ = wave_sum(s_);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s_;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
hipError_t launch_sumsq(const float* x, long n, float* out, float* scratch, int nwg, hipStream_t s) {
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)nwg), dim3(256), 0, s, x, n, scratch);
  hipLaunchKernelGGL(prep_bwd_reduce_dw_kernel, dim3(1), dim3(64), 0, s, scratch, (long)nwg, 1, out);
  return hipGetLastError();
}

// torch.optim.Adam._single_tensor_adam (amsgrad off, maximize off):  g' = g * gscale + wd * p;  m = m + (g' - m)(1 - b1);
// v = b2 v + (1 - b2) g'^2;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2_sqrt, float gscale) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float pv = p[i];
    const float gv = fmaf(wd, pv, g[i] * gscale);
    const float mv = m[i] + (gv - m[i]) * (1.0f - b1);
    const float vv = b2 * v[i] + (1.0f - b2) * gv * gv;
    m[i] = mv; v[i] = vv;
    p[i] = pv - (lr / bc1) * (mv / (sqrtf(vv) / bc2_sqrt + eps));
  }
}
hipError_t launch_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd, int step,
                       float gscale, hipStream_t s) {
  if (!p || !g || !m || !v || n < 1 || step < 1) return hipErrorInvalidValue;
  const float bc1 = 1.0f - powf(b1, (float)step), bc2 = 1.0f - powf(b2, (float)step);
  long grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)grid), dim3(256), 0, s, p, g, m, v, n, lr, b1, b2, eps, wd, bc1, sqrtf(bc2), gscale);
  return hipGetLastError();
}

// ==================================================================================================================
// Rank-ordered sum of the data-parallel gradient exchange (train_dist.GradExchange): parts [W][n] -> out [n],
//   out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...      plain fp32 adds in slice order, starting from slice 0's value
// One owner thread per element, no atomics: the bits depend on (parts, W) alone.  HBM bound, (W + 1) * 4 bytes per element: a
// thread owns four consecutive floats, issues the 16-byte loads of up to eight slices before the first add (8 x 16 B in flight
// per lane), then stores 16 bytes; the grid is sized to the chip and strides over n.  The 16-byte accesses ask for 4-byte
// alignment only (slice k starts at parts + k n, which is 16-byte aligned for every k only when n % 4 == 0: the exchange's
// shards are, train_dist.shard_layout); gfx950 serves dword-aligned dwordx4 global accesses.  The last n % 4 elements are
// summed one float at a time by the first threads of workgroup 0.
// ==================================================================================================================
typedef float rs_f4 __attribute__((ext_vector_type(4)));
typedef rs_f4 rs_f4u __attribute__((aligned(4)));

template <int G>
__device__ __forceinline__ rs_f4 rank_sum_group(const float* p, long n, rs_f4 acc, bool first) {
  rs_f4 r[G];
#pragma unroll
  for (int j = 0; j < G; ++j) r[j] = *(const rs_f4u*)(p + (long)j * n);
  acc = first ? r[0] : acc + r[0];
#pragma unroll
  for (int j = 1; j < G; ++j) acc = acc + r[j];
  return acc;
}

__device__ __forceinline__ rs_f4 rank_sum_rest(int g, const float* p, long n, rs_f4 acc, bool first) {
  switch (g) {                                                       // g is uniform over the grid: a scalar branch
    case 1: return rank_sum_group<1>(p, n, acc, first);
    case 2: return rank_sum_group<2>(p, n, acc, first);
    case 3: return rank_sum_group<3>(p, n, acc, first);
    case 4: return rank_sum_group<4>(p, n, acc, first);
    case 5: return rank_sum_group<5>(p, n, acc, first);
    case 6: return rank_sum_group<6>(p, n, acc, first);
    default: return rank_sum_group<7>(p, n, acc, first);
  }
}

__global__ __launch_bounds__(256) void rank_sum_kernel(const float* __restrict__ parts, float* __restrict__ out, int W, long n) {
  const long nv = n >> 2, stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
    const float* p = parts + 4 * v;
    rs_f4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; W - k >= 8; k += 8) acc = rank_sum_group<8>(p + (long)k * n, n, acc, k == 0);
    if (W - k) acc = rank_sum_rest(W - k, p + (long)k * n, n, acc, k == 0);
    *(rs_f4u*)(out + 4 * v) = acc;
  }
  if (blockIdx.x == 0 && (long)threadIdx.x < (n & 3)) {
    const long i = 4 * nv + threadIdx.x;
    float s_ = parts[i];
    for (int k = 1; k < W; ++k) s_ += parts[(long)k * n + i];
    out[i] = s_;
  }
}

// workgroups that fill the chip: 8 of 256 threads per compute unit (one wave of each on every SIMD twice over), cached per device
static long rank_sum_chip_grid() {
  static std::atomic<int> cus[128];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 128) return 8 * 256;
  int c = cus[d].load();
  if (!c) {
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || c < 1) c = 256;
    cus[d].store(c);
  }
  return 8L * c;
}

hipError_t launch_rank_sum(const float* parts, float* out, int W, long n, hipStream_t s) {
  if (!parts || !out || W < 1 || W > 64 || n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const long need = ((n >> 2) + 255) / 256;
  const long grid = std::max<long>(1, std::min<long>(need, rank_sum_chip_grid()));
  hipLaunchKernelGGL(rank_sum_kernel, dim3((unsigned)grid), dim3(256), 0, s, parts, out, W, n);
  return hipGetLastError();
}

}  // namespace tmk
