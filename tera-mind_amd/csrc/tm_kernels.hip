// Hand-written gfx950 (CDNA4) kernels of the Tera-MIND denoising hot path.
//
// Layout "CB8": fp32 [N][Cb][Z][H][W][8] -- channel blocks of 8 so that (a) an MFMA operand
// fragment (8 channels of one voxel) is one 32-byte piece, (b) a row of voxels is contiguous
// for coalesced HBM traffic, (c) a channel concat is a list of block ranges.
//
// Kernels (reference op each one replaces is cited at its definition):
//   conv3d_mfma / conv1_mfma   implicit-GEMM Conv3d on v_mfma_f32_32x32x2_f32 (exact fp32)
//   prep_kernel                concat + collage/up/down gather + RMSNorm(C) + modulate + SiLU
//   conv_direct_kernel         small convs (stem, head, RNA path) on VALU
//   (gene-gene and windowed attention kernels: tm_attn.hip)
//   time_embed / emb_all       timestep embedding MLP and all ResBlock emb_layers at once
//   (sampler_step / pad_patchify live in tm_sampler.hip: built with -ffp-contract=off)
#include "tm_conv_pair.h"

#include <stdlib.h>
#include <string.h>

#include <type_traits>

namespace tmk {

// NZI selects the z structure of the k x 3 x 3 kernel:
//   NZI = 2  3x3x3, pad (1,1,1), Z == 2: the z-skip form above (18 of 27 taps per output plane)
//   NZI = 1  1x3x3, pad (0,1,1): in-plane conv, any Z   (RNA pyramid, model/unet_ours.py:290-295)
//   NZI = 3  3x3x3 over three staged planes zo + zi + zoff: zoff = 0 is valid-in-z (Zin = Zout + 2: down_z,
//            model/MBAblocks.py:472-474), zoff = -1 with planes outside [0, Zin) zero is pad (1,1,1) for any Z
//            (the ResBlock convs of the z_size 4 / 8 configs, rna_slc 8 / 16)
//   UPS (with NZI = 2)  the same 3x3x3 conv applied to a nearest-x2 UPSAMPLED input (ResBlock(up=True): Upsample then
//            in_layers, model/MBAblocks.py:254-258, blocks.py:362-371), computed on the LOW-resolution tensor: output voxel
//            (2y + py, 2x + px) sees only the 2 x 2 low-resolution voxels (y + py - 1 .. y + py, x + px - 1 .. x + px), so
//            each of the four phases (py, px) is a conv with 2 x 2 in-plane taps whose weights are the sums of the 3 x 3
//            taps that land on the same source voxel (packed per phase by conv_pack_host, CF_ZSKIP_UPS): 8 instead of 18 taps per
//            output plane and a quarter of the input bytes; the zero padding of the upsampled tensor maps onto the zero
//            halo of the low-resolution tile.  Same sums, different association (weights are added before the products).
template <int NZI, int WM, int TW, bool UPS = false>
struct C3Geo {
  static constexpr int TW_ = TW;
  static constexpr int MV = 4 * WM * 32;                         // voxels per workgroup
  static constexpr int TR = (MV / TW < TW) ? (MV / TW) : TW;     // tile rows (<= plane size S == TW or 2*TW)
  static constexpr int NPB = MV / (TR * TW);                     // patches per workgroup
  static constexpr int HR = TR + 2, HC = TW + 2;
  static constexpr int XV = NPB * NZI * HR * HC;                 // halo voxels
  static constexpr int XPIECES = XV * 2;                         // 16-byte pieces
  static constexpr int PX = (XPIECES + 255) / 256;
  static constexpr int TZ = UPS ? 4 : 9;                         // in-plane taps
  static constexpr int NTAP = TZ * NZI;                          // taps staged per channel block
  static constexpr int WFLOATS = NTAP * 512;
  static constexpr int WPIECES = WFLOATS / 4;
  static constexpr int PW = (WPIECES + 255) / 256;
  static constexpr int TAPS_TOTAL = (NZI == 1) ? 9 : 3 * TZ;     // taps per channel block in the packed weights
  // channel blocks per stage: the 9-tap in-plane form (and the 8-tap upsampled form) has half the MFMAs per block of the
  // 18-tap z-skip form, so it stages two blocks per barrier pair to keep the same MFMA phase length
  static constexpr int KB = (NZI == 1 || UPS) ? 2 : 1;
  static constexpr int LDS_BYTES = KB * (WFLOATS + XV * 8) * 4;
};

template <int NZI, int WM, int TW, bool UPS = false>
__global__ __launch_bounds__(256, 2) void conv3d_mfma(ConvArgs a) {
  using G = C3Geo<NZI, WM, TW, UPS>;
  static_assert(!UPS || NZI == 2, "the upsampled-input form exists for the z-skip conv only");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int KB = G::KB;
  float* lw = lds;                                               // [KB][NTAP][512]
  float* lx = lds + KB * G::WFLOATS;                             // [KB][XV][8]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;

  const int S = a.S;
  const ConvTile t = conv_tile_of<TW, G::TR, UPS, true>(a);       // UPS: with the output phase of this workgroup
  const int nt = t.nt, pg = t.pg, zo = t.zo, tr = t.tr, tc = t.tc, py = t.py, px = t.px;

  // ---- per-thread staging descriptors (constant over the K loop) ----
  long xoff[G::PX];
#pragma unroll
  for (int k = 0; k < G::PX; ++k) {
    const int i = tid + k * 256;
    long off = -1;
    if (i < G::XPIECES) {
      const int half = i & 1;
      int v = i >> 1;
      const int hc = v % G::HC; v /= G::HC;
      const int hr = v % G::HR; v /= G::HR;
      const int zi = v % NZI;
      const int ps = v / NZI;
      const int zs = (NZI == 2) ? zi : zo + zi + a.zoff;         // source plane
      const int n = pg * G::NPB + ps;
      const int y = tr * G::TR + hr - 1, x = tc * TW + hc - 1;
      if (n < a.N && y >= 0 && y < S && x >= 0 && x < S && (NZI == 2 || (zs >= 0 && zs < a.Zin)))
        off = (long)n * a.x_nstride + ((long)(zs * S + y) * S + x) * 8 + half * 4;
    }
    xoff[k] = off;
  }
  // weights: the staged taps of this (n-tile, cblk) are contiguous; NZI == 2 starts at kz = 1 - zo
  const int tap0 = (NZI == 2) ? (1 - zo) * G::TZ : 0;
  const float* wsrc = a.w + (((long)(UPS ? (py * 2 + px) * a.ntile : 0) + nt) * a.Cbi * G::TAPS_TOTAL + tap0) * 512 + tid * 4;
  const long w_cb_stride = G::TAPS_TOTAL * 512;

  // ---- per-lane fragment addresses ----
  int xb[WM];
  int on[WM], ooff[WM];
#pragma unroll
  for (int mt = 0; mt < WM; ++mt) {
    const int v = (wv * WM + mt) * 32 + i32;
    const int ps = v / (G::TR * TW);
    const int rem = v - ps * (G::TR * TW);
    const int r = rem / TW, c = rem - r * TW;
    xb[mt] = ((ps * NZI * G::HR + r) * G::HC + c) * 8 + 4 * h;
    const int n = pg * G::NPB + ps;
    on[mt] = n;
    const int y = tr * G::TR + r, x = tc * TW + c;
    if (n < a.N) {
      if (UPS) ooff[mt] = ((zo * 2 * S + 2 * y + py) * 2 * S + 2 * x + px) * 8;
      else if (a.flags & EPI_UP2) ooff[mt] = ((zo * 2 * S + 2 * y) * 2 * S + 2 * x) * 8;
      else ooff[mt] = ((zo * S + y) * S + x) * 8;
    } else ooff[mt] = -1;
  }
  const int wb = i32 * 8 + 4 * h;

  f32x16 acc[2][WM];
  clear_acc(acc);

  f32x4 xr[KB][G::PX], wr[KB][G::PW];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_stage = [&](int st) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int cb = st * KB + kb;
      const bool live = KB == 1 || cb < a.Cbi;                   // a missing second block contributes zeros
      const float* xp = a.x + (long)cb * a.x_plane;
#pragma unroll
      for (int k = 0; k < G::PX; ++k) xr[kb][k] = (live && xoff[k] >= 0) ? *(const f32x4*)(xp + xoff[k]) : zero4;
      const float* wp = wsrc + (long)cb * w_cb_stride;
#pragma unroll
      for (int k = 0; k < G::PW; ++k)
        if (G::WPIECES % 256 == 0 || tid + k * 256 < G::WPIECES) wr[kb][k] = live ? *(const f32x4*)(wp + k * 1024) : zero4;
    }
  };

  const int nst = (a.Cbi + KB - 1) / KB;
  load_stage(0);
  for (int st = 0; st < nst; ++st) {
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int k = 0; k < G::PX; ++k)
        if (tid + k * 256 < G::XPIECES) *(f32x4*)(lx + kb * G::XV * 8 + (tid + k * 256) * 4) = xr[kb][k];
#pragma unroll
      for (int k = 0; k < G::PW; ++k)
        if (G::WPIECES % 256 == 0 || tid + k * 256 < G::WPIECES) *(f32x4*)(lw + kb * G::WFLOATS + (tid + k * 256) * 4) = wr[kb][k];
    }
    __syncthreads();
    if (st + 1 < nst) load_stage(st + 1);

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int zi = 0; zi < NZI; ++zi) {
#pragma unroll
        for (int ky = 0; ky < (UPS ? 2 : 3); ++ky) {
#pragma unroll
          for (int kx = 0; kx < (UPS ? 2 : 3); ++kx) {
            const int tap = UPS ? zi * 4 + ky * 2 + kx : zi * 9 + ky * 3 + kx;
            const int xd = kb * G::XV * 8 + ((zi * G::HR + ky + py) * G::HC + kx + px) * 8;
            f32x4 wf[2], xf[WM];
            wf[0] = *(const f32x4*)(lw + kb * G::WFLOATS + tap * 512 + wb);
            wf[1] = *(const f32x4*)(lw + kb * G::WFLOATS + tap * 512 + 256 + wb);
#pragma unroll
            for (int mt = 0; mt < WM; ++mt) xf[mt] = *(const f32x4*)(lx + xb[mt] + xd);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
              for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int mt = 0; mt < WM; ++mt)
                  acc[ct][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[ct][kk], xf[mt][kk], acc[ct][mt], 0, 0, 0);
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }
  conv_epilogue<WM>(a, acc, nt, h, on, ooff, 2 * S);
}

// ---- pair form of the 3x3x3 pad-1 conv at Z == 2 (fp32) ----
// With W0, W1, W2 the kz = 0, 1, 2 slices of the filter and X0, X1 the two input planes (`*` = in-plane 3 x 3 conv summed over
// cin) the z structure is a 2 x 2 block Toeplitz product, Y0 = W1*X0 + W2*X1, Y1 = W0*X0 + W1*X1: four in-plane products in
// the z-skip form above (36 taps per plane pair).  Three are enough:
//   P1 = W1 * (X0 + X1)    P2 = (W2 - W1) * X1    P3 = (W0 - W1) * X0        Y0 = P1 + P2    Y1 = P1 + P3
// (27 taps per plane pair, a quarter fewer MFMAs).  The weight slices are differenced once at pack time
// (conv_pack_host, CF_PAIR: W1, W2 - W1, W0 - W1, nine taps each), the two planes are added while staging.  Products and
// accumulation are fp32 as everywhere; the z association differs from F.conv3d's, like the in-plane association of UPS.
// One workgroup owns an in-plane tile of MV voxels, BOTH output planes and 64 couts.  HALF = 0: 128 voxels, wave = 32 voxels x
// 64 couts (3 x 2 accumulators); HALF = 1: 64 voxels, wave = 32 voxels x 32 couts (small launches).  Every output element
// sees the same order in both -- cin block outer, then product, tap, k -- so the two tiles give identical bits.
// LDS images (tm_conv_frag.h): the weights of a tap and every staged X plane are two k-half arrays of 16-byte slots,
// [2][64 couts][4] and [2][XV halo positions][4], and the lane -> voxel map follows the tile width (conv_lane_voxel), so that
// each 16-lane group of a ds_read_b128 fragment read meets sixteen different slots: 4 LDS cycles per read, not 8.
// FUSE (HALF = 0, 64 couts, one cout tile): the wave holds every channel of its 32 voxels, so the ResBlock mid-section (RMSNorm
// over channels -> modulate -> SiLU, zpair_norm_epilogue) runs on each output plane in place of the plain epilogue and the
// second conv's input is written instead of the conv output.  The K loop is the same code; layers that do not fuse run <.., false>.
template <int HALF, int TW>
struct ZPGeo {
  static constexpr int TW_ = TW;
  static constexpr int MV = HALF ? 64 : 128;                     // in-plane voxels per workgroup (2 MV outputs)
  static constexpr int TR = (MV / TW < TW) ? (MV / TW) : TW;     // tile rows
  static constexpr int NPB = MV / (TR * TW);                     // patches per workgroup
  static constexpr int HR = TR + 2, HW = TW + 2;                 // halo rows and columns
  static constexpr int HC = conv_halo_pitch(TW);                 // row pitch of the LDS image (tm_conv_frag.h: HW, at TW = 8 12)
  static constexpr int PS = conv_halo_patch(TW, HR);             // rows of a patch (HR * HC, at TW = 4 four more)
  static constexpr int XV = NPB * PS;                            // rows (halo positions) of ONE staged plane, [2 k-halves][XV][4]
  static constexpr int XPIECES = conv_stage_items(XV);           // staging items (16-byte pieces) per plane
  static constexpr int PX = (XPIECES + 255) / 256;
  static constexpr int WFLOATS = 27 * 512;                       // three 9-tap slots of the LDS-DMA weight ring
  static constexpr int LDS_BYTES = (WFLOATS + 3 * XV * 8) * 4;  // weights + the planes X0 + X1, X1, X0
};
// The constant part of a fragment address of the two z-pair kernels (floats; the lane's part is wb / xb below): tap `tap` of the
// weight area, 32-cout sub-tile ct; window position (ky, kx) of staged plane p.  Shared with tm_conv_frag_addrs.
TM_HD constexpr int zp_wtap(int tap, int ct) { return tap * 512 + conv_w_off(ct * 32, 0); }
template <class G>
TM_HD constexpr int zp_xtap(int p, int ky, int kx) { return p * G::XV * 8 + conv_frag_off(ky * G::HC + kx, 0, G::XV); }

template <int HALF, int TW, bool FUSE = false>
__global__ __launch_bounds__(256, 2) void conv3d_zpair(ConvArgs a) {
  static_assert(!FUSE || HALF == 0, "the fused mid-section needs every cout of a voxel in one wave");
  using G = ZPGeo<HALF, TW>;
  constexpr int NC = HALF ? 1 : 2;                               // 32-cout sub-tiles per wave
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lw = lds;                                               // [27][2 k-halves][64][4]
  float* lx = lds + G::WFLOATS;                                  // [3][2 k-halves][XV][4]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;

  const int S = a.S;
  const ConvTile t = conv_tile_of<TW, G::TR, false, false>(a);
  const int nt = t.nt, pg = t.pg, tr = t.tr, tc = t.tc;

  // ---- per-thread staging descriptors: the z = 0 piece of a halo position (the z = 1 piece is one plane further) ----
  long xoff[G::PX];
#pragma unroll
  for (int k = 0; k < G::PX; ++k) {
    const int i = tid + k * 256;
    long off = -1;
    if (i < G::XPIECES) {
      const int half = conv_stage_half(i);
      int v = conv_stage_row(i);
      const int ps = v / G::PS; v -= ps * G::PS;                 // ps == NPB: past the image, nothing is stored
      const int hr = v / G::HC, hc = v % G::HC;                  // (rows from HR and columns from HW of the pitches are never read)
      const int n = pg * G::NPB + ps;
      const int y = tr * G::TR + hr - 1, x = tc * TW + hc - 1;
      if (ps < G::NPB && hr < G::HR && hc < G::HW && n < a.N && y >= 0 && y < S && x >= 0 && x < S)
        off = (long)n * a.x_nstride + ((long)y * S + x) * 8 + half * 4;
    }
    xoff[k] = off;
  }
  const long zplane = (long)S * S * 8;

  // ---- per-lane fragment addresses ----
  const int vt = HALF ? (wv & 1) : wv;                           // 32-voxel tile of this wave
  const int ct0 = HALF ? (wv >> 1) : 0;                          // its first 32-cout sub-tile
  int xb, on[1], ooff0[1], ooff1[1];
  {
    const ConvLane l = conv_lane_of<G::TR, TW, G::PS, G::HC, G::XV>(vt * 32 + conv_lane_voxel(TW, i32), h, 0, 0);
    xb = l.xb;
    const int n = pg * G::NPB + l.ps;
    on[0] = n;
    const int y = tr * G::TR + l.r, x = tc * TW + l.c;
    if (n < a.N) {
      if (a.flags & EPI_UP2) { ooff0[0] = (2 * y * 2 * S + 2 * x) * 8; ooff1[0] = ooff0[0] + 4 * S * S * 8; }
      else { ooff0[0] = (y * S + x) * 8; ooff1[0] = ooff0[0] + S * S * 8; }
    } else { ooff0[0] = -1; ooff1[0] = -1; }
  }
  const int wb = conv_w_off(ct0 * 32 + i32, 4 * h);

  f32x16 acc[3][NC];
  clear_acc(acc);

  // ---- weights: global -> LDS by LDS-DMA (`buffer_load_dwordx4 ... offen lds`), no staging registers ----
  // The packed weights of a (cout tile, cin block) ARE the LDS image, product by product, so lw is a ring of three 9-tap slots
  // (18 432 B = 18 wave-instructions of 1 KiB; wave w issues pieces w, w + 4, ..: five for waves 0 and 1, four for 2 and 3).
  // Slot p is refilled with product p of the NEXT cin block once every wave has finished product p of this one:
  //   B0 | X -> LDS | B1 | P1 + pieces of W3(cb) | B2 | P2 + pieces of W1(cb+1) | vmcnt | B3 | P3 + pieces of W2(cb+1)
  // W1 / W2 of a block are retired by the vmcnt(0) in front of B0 and first read behind B1; W3 has P1 and P2 to land and is
  // retired by a counted wait in front of B3: at least the four W1 pieces every wave issued behind it may stay in flight.
  // The pieces are inline asm (M0 = LDS address of the piece, set in the statement that uses it): hipcc does not count them,
  // so it neither drains them at a barrier nor waits for them in front of the fragment reads of the other slots.
  const unsigned lw_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lw;
  const rsrc_words wrs = weight_rsrc<false>(a.w + (long)nt * a.Cbi * G::WFLOATS, a.Cbi * G::WFLOATS * 4);
  const int wvo = lane * 16;
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  auto issue_piece = [&](int cb, int p, int k) __attribute__((always_inline)) {   // piece k of this wave of slot p's 18
    lds_dma_piece<0, 18>(lw_lds, p * 9 * 512, (cb * 27 + p * 9) * 512, k, wvu, wvo, wrs);
  };

  f32x4 xr[2][G::PX];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int cb) {
    const float* xp = a.x + (long)cb * a.x_plane;
#pragma unroll
    for (int k = 0; k < G::PX; ++k) {
      xr[0][k] = xoff[k] >= 0 ? *(const f32x4*)(xp + xoff[k]) : zero4;
      xr[1][k] = xoff[k] >= 0 ? *(const f32x4*)(xp + xoff[k] + zplane) : zero4;
    }
  };

  load_x(0);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int k = 0; k < 5; ++k) issue_piece(0, p, k);
  // one cin block; MORE = another block follows (the last block is its own instantiation: no branch around a piece)
  auto stage = [&](int cb, auto more_c) __attribute__((always_inline)) {
    constexpr bool more = decltype(more_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // X(cb) in registers; this wave's pieces of W1(cb), W2(cb) landed
    __builtin_amdgcn_s_barrier();                                // B0: every wave is through P3(cb - 1): lx and slot 2 are free
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < G::PX; ++k)
      if (conv_stage_row(tid + k * 256) < G::XV) {
        float* d = lx + conv_frag_off(conv_stage_row(tid + k * 256), conv_stage_half(tid + k * 256), G::XV);
        *(f32x4*)(d) = xr[0][k] + xr[1][k];
        *(f32x4*)(d + G::XV * 8) = xr[1][k];
        *(f32x4*)(d + 2 * G::XV * 8) = xr[0][k];
      }
    __builtin_amdgcn_s_waitcnt(0xC07F);                          // lgkmcnt(0) only
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();                                // B1
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (more) load_x(cb + 1);

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      if (p > 0) {
        // B2: slot 0 is free.  B3: slot 1 is free, and W3(cb) has landed -- in the last block nothing was issued behind it
        if (p == 2) { if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int tap = p * 9 + ky * 3 + kx;
          f32x4 wf[NC];
#pragma unroll
          for (int ct = 0; ct < NC; ++ct) wf[ct] = *(const f32x4*)(lw + zp_wtap(tap, ct) + wb);
          const f32x4 xf = *(const f32x4*)(lx + zp_xtap<G>(p, ky, kx) + xb);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int ct = 0; ct < NC; ++ct)
              acc[p][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[ct][kk], xf[kk], acc[p][ct], 0, 0, 0);
          // one piece behind each of the first five taps: W3(cb) under P1, W1(cb + 1) under P2, W2(cb + 1) under P3
          if (ky * 3 + kx < 5) {
            if (p == 0) issue_piece(cb, 2, ky * 3 + kx);
            else if (more) issue_piece(cb + 1, p - 1, ky * 3 + kx);
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };
  for (int cb = 0; cb + 1 < a.Cbi; ++cb) stage(cb, std::true_type{});
  stage(a.Cbi - 1, std::false_type{});
  // Y0 = P1 + P2, Y1 = P1 + P3: one epilogue per output plane (bias, residual, pad slots as in every other form)
  f32x16 o[NC][1];
  const int nte = HALF ? 2 * nt + ct0 : nt;                      // conv_epilogue counts cout blocks in units of its own tile
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) o[ct][0] = acc[0][ct] + acc[1][ct];
  if constexpr (FUSE) zpair_norm_epilogue(a, o, h, on[0], ooff0[0]);
  else conv_epilogue<1, NC>(a, o, nte, h, on, ooff0, 2 * S);
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) o[ct][0] = acc[0][ct] + acc[2][ct];
  if constexpr (FUSE) zpair_norm_epilogue(a, o, h, on[0], ooff1[0]);
  else conv_epilogue<1, NC>(a, o, nte, h, on, ooff1, 2 * S);
}

// ---- pair form of the upsampled-input conv (fp32, Z == 2): ResBlock(up=True)'s first conv ----
// The UPS form of conv3d_mfma runs, per output phase (py, px), a 2 x 2 in-plane window on each of the two z taps of each output
// plane: four in-plane products per plane pair, 16 tap-products.  The pair identity above is linear in the weights, so it
// commutes with the pre-summing of the phase weights: with V0, V1, V2 the kz slices of the PHASE weights (the CF_ZSKIP_UPS pack's
// sums) the kernel computes P1 = V1 * (X0 + X1), P2 = (V2 - V1) * X1, P3 = (V0 - V1) * X0 on the low-resolution planes, 12
// tap-products per plane pair, and stores Y0 = P1 + P2, Y1 = P1 + P3 at (2 y + py, 2 x + px) of the two output planes.
// Weights: conv_pack_host (CF_PAIR_UPS), per (phase, cout tile, cin block) 12 taps x 512 floats in the order the kernel consumes
// them (product, wy, wx) -- the same size as the z-skip UPS pack.  Staging of X is conv3d_zpair's (the two planes added in
// registers, three LDS planes).  The weights come by the same LDS-DMA pieces, but a block's 12 taps are only 24 KiB, so the ring
// is two whole-block slots and a cin block costs two barriers, not four:
//   vmcnt(0) | B0 | X(cb) -> LDS | B1 | 12 taps from slot cb & 1, with X(cb + 1) -> registers and the six pieces each wave owns of
//   W(cb + 1) -> slot (cb + 1) & 1 behind the first six taps
// Slot (cb + 1) & 1 was last read in block cb - 1, which every wave left before B0; a wave's own pieces of W(cb) are retired by
// its vmcnt(0) in front of B0 and everybody's are visible behind it.  LDS: 2 x 24 576 B of weights + 3 X planes (at most 23 040 B,
// the 8-wide tile at pitch 12) = 72 192 B at most: two workgroups per CU.
// Tiles, wave layout and accumulation order per output element (cin block, product,
// tap, k) are conv3d_zpair's, so HALF = 0 and 1 give identical bits.
template <int HALF, int TW>
struct ZPUGeo : ZPGeo<HALF, TW> {
  static constexpr int WSLOT = 12 * 512;                         // floats of one (phase, cout tile, cin block)
  static constexpr int LDS_BYTES = (2 * WSLOT + 3 * ZPGeo<HALF, TW>::XV * 8) * 4;   // the two-slot ring + the planes X0 + X1, X1, X0
};

template <int HALF, int TW>
__global__ __launch_bounds__(256, 2) void conv3d_zpair_ups(ConvArgs a) {
  using G = ZPUGeo<HALF, TW>;
  constexpr int NC = HALF ? 1 : 2;
  constexpr int WSLOT = G::WSLOT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lw = lds;                                               // [2][12][2 k-halves][64][4]
  float* lx = lds + 2 * WSLOT;                                   // [3][2 k-halves][XV][4]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;

  const int S = a.S;                                             // the LOW-resolution plane; the output plane is 2 S
  const ConvTile t = conv_tile_of<TW, G::TR, true, false>(a);
  const int nt = t.nt, pg = t.pg, tr = t.tr, tc = t.tc, py = t.py, px = t.px;

  long xoff[G::PX];
#pragma unroll
  for (int k = 0; k < G::PX; ++k) {
    const int i = tid + k * 256;
    long off = -1;
    if (i < G::XPIECES) {
      const int half = conv_stage_half(i);
      int v = conv_stage_row(i);
      const int ps = v / G::PS; v -= ps * G::PS;                 // ps == NPB: past the image, nothing is stored
      const int hr = v / G::HC, hc = v % G::HC;                  // (rows from HR and columns from HW of the pitches are never read)
      const int n = pg * G::NPB + ps;
      const int y = tr * G::TR + hr - 1, x = tc * TW + hc - 1;
      if (ps < G::NPB && hr < G::HR && hc < G::HW && n < a.N && y >= 0 && y < S && x >= 0 && x < S)
        off = (long)n * a.x_nstride + ((long)y * S + x) * 8 + half * 4;
    }
    xoff[k] = off;
  }
  const long zplane = (long)S * S * 8;

  const int vt = HALF ? (wv & 1) : wv;
  const int ct0 = HALF ? (wv >> 1) : 0;
  int xb, on[1], ooff0[1], ooff1[1];
  {
    const ConvLane l = conv_lane_of<G::TR, TW, G::PS, G::HC, G::XV>(vt * 32 + conv_lane_voxel(TW, i32), h, py, px);
    xb = l.xb;                                                   // the phase's window starts at (y + py - 1, x + px - 1)
    const int n = pg * G::NPB + l.ps;
    on[0] = n;
    const int y = tr * G::TR + l.r, x = tc * TW + l.c;
    if (n < a.N) { ooff0[0] = ((2 * y + py) * 2 * S + 2 * x + px) * 8; ooff1[0] = ooff0[0] + 4 * S * S * 8; }
    else { ooff0[0] = -1; ooff1[0] = -1; }
  }
  const int wb = conv_w_off(ct0 * 32 + i32, 4 * h);

  f32x16 acc[3][NC];
  clear_acc(acc);

  const unsigned lw_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lw;
  const rsrc_words wrs = weight_rsrc<false>(a.w + ((long)(py * 2 + px) * a.ntile + nt) * a.Cbi * WSLOT, a.Cbi * WSLOT * 4);
  const int wvo = lane * 16;
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  // piece k (0..5) of this wave: 256 floats at j = 4 k + wave of the block's 24
  auto issue_piece = [&](int cb, int k) __attribute__((always_inline)) {
    lds_dma_piece<0, 24>(lw_lds, (cb & 1) * WSLOT, cb * WSLOT, k, wvu, wvo, wrs);
  };

  f32x4 xr[2][G::PX];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int cb) {
    const float* xp = a.x + (long)cb * a.x_plane;
#pragma unroll
    for (int k = 0; k < G::PX; ++k) {
      xr[0][k] = xoff[k] >= 0 ? *(const f32x4*)(xp + xoff[k]) : zero4;
      xr[1][k] = xoff[k] >= 0 ? *(const f32x4*)(xp + xoff[k] + zplane) : zero4;
    }
  };

  load_x(0);
#pragma unroll
  for (int k = 0; k < 6; ++k) issue_piece(0, k);
  auto stage = [&](int cb, auto more_c) __attribute__((always_inline)) {
    constexpr bool more = decltype(more_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // X(cb) in registers; this wave's pieces of W(cb) landed
    __builtin_amdgcn_s_barrier();                                // B0: every wave is through block cb - 1
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < G::PX; ++k)
      if (conv_stage_row(tid + k * 256) < G::XV) {
        float* d = lx + conv_frag_off(conv_stage_row(tid + k * 256), conv_stage_half(tid + k * 256), G::XV);
        *(f32x4*)(d) = xr[0][k] + xr[1][k];
        *(f32x4*)(d + G::XV * 8) = xr[1][k];
        *(f32x4*)(d + 2 * G::XV * 8) = xr[0][k];
      }
    __builtin_amdgcn_s_waitcnt(0xC07F);                          // lgkmcnt(0) only
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();                                // B1
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (more) load_x(cb + 1);
    const float* lwc = lw + (cb & 1) * WSLOT;

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int ky = 0; ky < 2; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 2; ++kx) {
          const int tap = p * 4 + ky * 2 + kx;
          f32x4 wf[NC];
#pragma unroll
          for (int ct = 0; ct < NC; ++ct) wf[ct] = *(const f32x4*)(lwc + zp_wtap(tap, ct) + wb);
          const f32x4 xf = *(const f32x4*)(lx + zp_xtap<G>(p, ky, kx) + xb);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int ct = 0; ct < NC; ++ct)
              acc[p][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[ct][kk], xf[kk], acc[p][ct], 0, 0, 0);
          if (more && tap < 6) issue_piece(cb + 1, tap);         // one piece of W(cb + 1) behind each of the first six taps
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };
  for (int cb = 0; cb + 1 < a.Cbi; ++cb) stage(cb, std::true_type{});
  stage(a.Cbi - 1, std::false_type{});
  f32x16 o[NC][1];
  const int nte = HALF ? 2 * nt + ct0 : nt;
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) o[ct][0] = acc[0][ct] + acc[1][ct];
  conv_epilogue<1, NC>(a, o, nte, h, on, ooff0, 0);
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) o[ct][0] = acc[0][ct] + acc[2][ct];
  conv_epilogue<1, NC>(a, o, nte, h, on, ooff1, 0);
}

// ---- x-quad form of the 3x3x3 pad-1 conv at Z == 2 (fp32): the pair form in z composed with Winograd F(4,3) along x ----
// F(4,3) gives four neighbouring outputs of a 3-tap filter g with six products instead of twelve: with d0..d5 the inputs at
// columns 4j - 1 .. 4j + 4 (zero outside the plane),
//   T0 = (4 d0 - 5 d2) + d4           U0 = g0 / 4                               (T: while staging; U: at pack time,
//   T1 = (d3 + d4) - 4 (d1 + d2)      U1 = -((g0 + g1) + g2) / 6                 conv_pack_host, CF_XQUAD)
//   T2 = 4 (d1 - d2) - (d3 - d4)      U2 = -((g0 - g1) + g2) / 6
//   T3 = 2 (d3 - d1) + (d4 - d2)      U3 = (g0 / 24 + g1 / 12) + g2 / 6
//   T4 = 2 (d1 - d3) + (d4 - d2)      U4 = (g0 / 24 - g1 / 12) + g2 / 6
//   T5 = (4 d1 - 5 d3) + d5           U5 = g2
//   A_q = sum over cin, ky of U_q[ky] T_q[y + ky - 1][j];  s = A1 + A2, d = A1 - A2, s' = A3 + A4, d' = A3 - A4
//   out[4j] = (A0 + s) + s'   out[4j + 1] = d + 2 d'   out[4j + 2] = s + 4 s'   out[4j + 3] = (d + 8 d') + A5.
// The identity is linear in the weights, so it applies to each of the three z products of the pair form (V = W1, W2 - W1, W0 - W1
// on X0 + X1, X1, X0): per (product, ky) six transform positions per group replace three taps per voxel, 54 tap-products per
// eight outputs, 6.75 per output against the pair form's 13.5.  A_q(p) is accumulated on the MFMA exactly as a tap is.  ORDER OF
// SUMS of every output, in both tiles: cin block, product, ky, k inside an accumulator A_q(p); then the output transform exactly
// as written above; then Y(z0) = P(1) + P(2), Y(z1) = P(1) + P(3); then the epilogue.  So HALF = 0 and 1 give identical bits.
// A workgroup owns MG four-column groups, both output planes and 32 couts (a 64-cout ring of two product slots would pass the
// 64 KiB an LDS-DMA destination must stay below).  A wave owns 32 groups x 32 couts and three of the six q (3 products x 3 q = 9
// accumulators); wave & 1 is the q half, wave >> 1 the group tile.  HALF = 0: 8 waves, 128 groups (1024 output voxels), one
// workgroup per CU; HALF = 1 (launches that do not fill the chip): 4 waves, 64 groups.  After the K loop the q halves exchange one
// tile per product through LDS (d one way, s' the other); half 0 finishes columns 0 and 2, half 1 columns 1 and 3.
// LDS: the weight ring [2 product slots][18 taps (ky, q)][2 k-halves][32 couts][4] = 36 864 B first (LDS-DMA destinations below
// 64 KiB), then per product six q-planes [2 k-halves][XP][4] of XP = NPB x HR x TW/4 group positions (no x halo).  The planes end
// past 64 KiB, so a lane keeps one hidden base per product (16-byte slots: every fragment read is one ds_read_b128 with a
// 16-bit offset).  At TW = 8 a wave's 32 groups span two patches 20 rows apart: the lanes of the first ds_read_b128 group take
// the first patch, the others the second (conv_lane_voxel's TW = 16 table), so each group reads sixteen consecutive rows.
//
// PIPE = 0, the four-barrier schedule.  The weights are a ring of two PRODUCT slots (the 18 taps (ky, q) of one product of a cin
// block) filled by LDS-DMA, one tap per piece, the pieces dealt round the waves: product n = 3 cb + p reads slot n & 1, the pieces
// of product n + 1 go out behind its first taps into the slot every wave left at the barrier in front of product n, and a wave
// retires its own with the vmcnt(0) in front of the next product's barrier.  The X planes are three sets of six q-planes, one
// set per product of the block, all transformed and stored in one phase.  A cin block costs four barriers:
//   vmcnt(0) | B0 | T(cb) -> LDS | B1 | P1, X(cb + 1) -> registers | vmcnt(0) | B2 | P2 | vmcnt(0) | B3 | P3
// B0: X(cb) is in registers, this wave's pieces of product 3 cb landed, and every wave is through block cb - 1, so the planes and
// the other slot are free.  B1 (lgkmcnt(0) in front): the planes are visible; the loads of X(cb + 1) go out behind it, under P1.
// B2, B3: everybody's pieces of the product are visible and the slot of the product before is free.  The last cin block is its
// own instantiation of the block body: no branch round a piece or a load.
//
// PIPE = 1, the pipelined schedule (same pack, tiles, lane maps, accumulators and epilogue): the X planes are a ring of TWO SETS
// of six q-planes, and no phase is left in which the matrix pipe must idle.  The products of a block run in the order X0, X1,
// X0 + X1 (pack products 2, 1, 0: the accumulator families are independent, and inside one the order stays cin block, ky, k, so
// no bit of any output changes); the running count n = 3 cb + i gives both the weight slot and the plane set, n & 1.  While
// product n is multiplied, in its first taps (between a tap's fragment reads and its MFMAs, where the pieces of the weight ring
// go out as well), the staging threads transform and store the planes of product n + 1 into the other set: X1 under X0's product; then X0 += X1 in place (no temporaries) and the sum under X1's, two planes per tap, after
// which the registers take the loads of block cb + 1 (X0 first); X0(cb + 1) under the sum's.  The one barrier in front of each
// product publishes its weight slot and its plane set: a wave arrives with lgkmcnt(0) for its own stores and the vmcnt that
// covers its own pieces -- vmcnt(12) in front of the sum's product, where the twelve X loads issued behind the pieces may stay
// in flight (every wave that loads issues exactly twelve: the addresses of items outside the plane are clamped, not branched
// around), vmcnt(0) elsewhere.  Three barriers per cin block:
//   [ pieces(0), X(0) -> registers, T(X0) -> set 0 ]   then per block   vmcnt | lgkmcnt(0) | B | P(X0), T(X1) | .. | B | P(X1),
//   T(X0 + X1), X(cb + 1) -> registers | vmcnt(12) | lgkmcnt(0) | B | P(X0 + X1), T(X0(cb + 1))
// LDS: 36 864 B of ring + 12 q-planes, not less than the exchange area behind the K loop (NW x 3 x 4 KiB): 98 304 B in both
// large tiles (one workgroup per CU, as before), 64 512 B (<1,16>) and 67 584 B (<1,8>) in the small ones: two per CU.
//
// THE TAIL (both schedules, all tiles; nothing of the large tile's tail is covered by another workgroup, so it is kept short).
// The kernel has an epilogue of its own with conv_epilogue's arithmetic in its order -- (acc + bias) -> GELU flag -> res + -- and
// its addresses, res_half's (z, y >> 1, x >> 1) included; a gate is refused by the launcher.  Behind the K loop, where the X and
// fragment registers are dead, a wave requests the four bias quads and the eight residual quads of its z = 0 outputs, then
// passes the exchange (each half names the tile it sends acc[p][2], so that it is dead behind the send in both halves), whose
// barriers are bare s_barriers with lgkmcnt(0) alone: no wait for the loads in flight.  The z = 1 quads of column pair 0 go out
// behind the sends into the sent tiles' registers, those of pair 1 behind the columns into the received tiles': all sixteen are
// requested before the first output is formed (144 accumulator + 48 received + 64 residual registers would not fit at once).
// The requests are unconditional -- a lane without a voxel or a cout block reads element 0 of the tensor, a launch without a
// residual element 0 of the bias -- so the tail is one straight line and every wait is the counted vmcnt of its own quad.  An
// address is a per-lane term (patch, row, group, q half, k half) plus a uniform one (cout block, plane, column pair).  The
// outputs are formed for every lane in the residual's registers; the sixteen guarded stores follow and wait for nothing
// (profiles/fp32_xquad_tail.txt: the stamps of the tail, and the groupings of the requests that spill).
template <int HALF, int TW, int PIPE = 0>
struct XQGeo {
  static constexpr int TW_ = TW;
  static constexpr int NW = HALF ? 4 : 8;                        // waves per workgroup
  static constexpr int MG = 16 * NW;                             // four-column groups per workgroup
  static constexpr int GW = TW / 4;                              // groups per tile row
  static constexpr int TR = (MG / GW < TW) ? (MG / GW) : TW;     // tile rows
  static constexpr int NPB = MG / (TR * GW);                     // patches per workgroup
  static constexpr int HR = TR + 2;
  static constexpr int XP = NPB * HR * GW;                       // group positions of one q-plane (y halo only)
  static constexpr int XITEMS = XP * 2;                          // staging items: (position, half block), one per thread
  static_assert(XP % 8 == 0, "whole groups of eight staging items (tm_conv_frag.h)");
  static constexpr int WTAP = 256;                               // floats of one tap of 32 couts
  static constexpr int WSLOT = 18 * WTAP;                        // floats of one product of a (cout tile, cin block)
  static constexpr int KP = (18 + NW - 1) / NW;                  // LDS-DMA pieces (one tap each) of a slot per wave, at most
  static constexpr int XSET = 6 * XP * 8;                        // floats of the six q-planes of one product
  static constexpr int NSET = PIPE ? 2 : 3;                      // sets in LDS: the ring of two | the three products of a block
  static constexpr int XCH = NW * 3 * 1024;                      // floats of the exchange area behind the K loop
  static constexpr int LDS_BYTES = (2 * WSLOT + NSET * XSET > XCH ? 2 * WSLOT + NSET * XSET : XCH) * 4;
  static_assert(2 * WSLOT * 4 <= 65536 && LDS_BYTES <= 160 * 1024, "LDS-DMA destinations below 64 KiB, the CU's LDS");
  static_assert(!PIPE || !HALF || LDS_BYTES <= 80 * 1024, "two workgroups of the small tile per CU");
};
// plane q of the input transform from the six columns of a group (the one statement of T0 .. T5, for both schedules)
template <class V>
TM_HD V xq_transform(int q, const V (&d)[6]) {
  switch (q) {
    case 0: return (4.f * d[0] - 5.f * d[2]) + d[4];
    case 1: return (d[3] + d[4]) - 4.f * (d[1] + d[2]);
    case 2: return 4.f * (d[1] - d[2]) - (d[3] - d[4]);
    case 3: return 2.f * (d[3] - d[1]) + (d[4] - d[2]);
    case 4: return 2.f * (d[1] - d[3]) + (d[4] - d[2]);
    default: return (4.f * d[1] - 5.f * d[3]) + d[5];
  }
}
// the lane's group (0 .. 31 of the wave's tile) and the float offset of tap (ky, q) in a product slot
TM_HD constexpr int xq_lane_group(int tw, int i32) { return tw == 8 ? conv_lane_voxel(16, i32) : i32; }
// The constant part of conv3d_xquad's X fragment address (floats) inside a product's six planes: row ky of q-plane q.
template <class G>
TM_HD constexpr int xq_xtap(int q, int ky) { return q * G::XP * 8 + conv_frag_off(ky * G::GW, 0, G::XP); }
// The base of a lane's X fragments (floats behind the weight ring) in plane set `set` (the product's own, or the ring's set of the
// pipelined schedule) for q half qh, lxb = the lane's conv_lane_of offset; and of a staging item's slot in plane q of a set
template <class G>
TM_HD constexpr int xq_xfrag(int set, int qh, int lxb) { return set * G::XSET + 3 * qh * G::XP * 8 + lxb; }
template <class G>
TM_HD constexpr int xq_xstage(int set, int q, int item) {
  return set * G::XSET + q * G::XP * 8 + conv_frag_off(conv_stage_row(item), conv_stage_half(item), G::XP);
}

template <int HALF, int TW, int PIPE>
__global__ __launch_bounds__(HALF ? 256 : 512, 2) void conv3d_xquad(ConvArgs a) {
  using G = XQGeo<HALF, TW, PIPE>;
  static_assert(G::XITEMS <= 64 * G::NW, "one staging item per thread");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lw = lds;                                               // the weight ring; the X planes follow at float 2 * WSLOT

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;

  const int S = a.S;
  const ConvTile t = conv_tile_of<TW, G::TR, false, false>(a);   // a.ntile counts 32-cout tiles here
  // split K (a.ksplit 1 | 2 | 4): the split index is the slowest term of the swizzled block index, so it arrives on top of the
  // patch group.  Split ks owns cin blocks [cb0, cb0 + nkb) of this (voxel tile, cout tile): x and the weight resource start at
  // cb0, the K loop runs nkb blocks and the raw sums go to partial ks.  All of it is wave-uniform: scalar registers only
  const int pgs = (a.N + G::NPB - 1) / G::NPB;
  const int ks = __builtin_amdgcn_readfirstlane(a.ksplit > 1 ? (t.pg >= pgs) + (t.pg >= 2 * pgs) + (t.pg >= 3 * pgs) : 0);
  const int cb0 = __builtin_amdgcn_readfirstlane((ks * a.Cbi) >> (a.ksplit >> 1));
  const int nkb = __builtin_amdgcn_readfirstlane((((ks + 1) * a.Cbi) >> (a.ksplit >> 1)) - cb0);
  a.x += (long)cb0 * a.x_plane;
  a.y += ks * a.part_stride;
  const int nt = t.nt, pg = t.pg - ks * pgs, tr = t.tr, tc = t.tc;

  // ---- staging descriptor: this thread's (row, group, half block); xoff addresses column 4j of plane 0 ----
  long xoff = -1;
  bool okl = false, okr = false;                                 // columns 4j - 1 and 4j + 4 lie inside the plane
  if (tid < G::XITEMS) {
    const int half = conv_stage_half(tid);
    int v = conv_stage_row(tid);
    const int j = v % G::GW; v /= G::GW;
    const int hr = v % G::HR;
    const int ps = v / G::HR;
    const int n = pg * G::NPB + ps;
    const int y = tr * G::TR + hr - 1, x = tc * TW + 4 * j;
    if (n < a.N && y >= 0 && y < S) {
      xoff = (long)n * a.x_nstride + ((long)y * S + x) * 8 + half * 4;
      okl = x > 0;
      okr = x + 4 < S;
    }
  }
  const long zplane = (long)S * S * 8;
  int xw = 2 * G::WSLOT + xq_xstage<G>(0, 0, tid);
  asm volatile("" : "+v"(xw));

  // ---- per-lane fragment addresses ----
  const int gt = wv >> 1;                                        // 32-group tile of this wave
  const int qh = wv & 1;                                         // its q half: q = 3 qh .. 3 qh + 2
  int xb[3], on[1], ooff0;                                       // ooff0: column 4j of plane 0 (or -1)
  {
    const ConvLane l = conv_lane_of<G::TR, G::GW, G::HR * G::GW, G::GW, G::XP>(gt * 32 + xq_lane_group(TW, i32), h, 0, 0);
#pragma unroll
    for (int p = 0; p < 3; ++p) {                                // one hidden base per product, in 16-byte slots (PIPE: [0], of set 0)
      xb[p] = (2 * G::WSLOT + xq_xfrag<G>(p, qh, l.xb)) / 4;
      asm volatile("" : "+v"(xb[p]));
    }
    const int n = pg * G::NPB + l.ps;
    on[0] = n;
    const int y = tr * G::TR + l.r, x = tc * TW + 4 * l.c;
    ooff0 = n < a.N ? (y * S + x) * 8 : -1;
  }
  const int wb = 3 * qh * G::WTAP + conv_frag_off(i32, h, 32);

  f32x16 acc[3][3];
  clear_acc(acc);

  const unsigned lw_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lw;
  const rsrc_words wrs = weight_rsrc<true>(a.w + ((long)nt * a.Cbi + cb0) * 3 * G::WSLOT, nkb * 3 * G::WSLOT * 4);
  const int wvo = lane * 16;
  const int wvu = __builtin_amdgcn_readfirstlane(wv);
  // piece k of this wave of product n: tap j = NW k + wave of the product's 18
  auto issue_piece = [&](int n, int k) __attribute__((always_inline)) {
    lds_dma_piece<4, 18, G::NW>(lw_lds, (n & 1) * G::WSLOT, n * G::WSLOT, k, wvu, wvo, wrs);
  };

  f32x4 xr[2][6];                                                // [plane][column 4j - 1 .. 4j + 4]
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int cb) {
    const float* xp = a.x + (long)cb * a.x_plane;
#pragma unroll
    for (int z = 0; z < 2; ++z) {
      const float* b = xp + xoff + z * zplane;
      xr[z][0] = okl ? *(const f32x4*)(b - 8) : zero4;
#pragma unroll
      for (int c = 0; c < 4; ++c) xr[z][1 + c] = xoff >= 0 ? *(const f32x4*)(b + 8 * c) : zero4;
      xr[z][5] = okr ? *(const f32x4*)(b + 32) : zero4;
    }
  };
  // the six transform planes of one product from its six columns
  auto put_t = [&](int p, const f32x4 (&d)[6]) __attribute__((always_inline)) {
    float* o = lds + xw + p * G::XSET;
#pragma unroll
    for (int q = 0; q < 6; ++q) *(f32x4*)(o + q * G::XP * 8) = xq_transform(q, d);
  };

  if constexpr (PIPE) {
  // ---- the pipelined schedule (header comment): product i of a block is pack product 2 - i, in slot and plane set n & 1 ----
  const bool stg = tid < G::XITEMS;
  const bool ldw = __builtin_amdgcn_readfirstlane(wv * 64 < G::XITEMS);   // this wave has staging items: it loads X
  // every load is issued, whatever the item: exactly twelve per loading wave, which the counted vmcnt relies on
  auto load_xc = [&](int cb) __attribute__((always_inline)) {
    const float* xp = a.x + (long)cb * a.x_plane + (xoff >= 0 ? xoff : 0);
#pragma unroll
    for (int z = 0; z < 2; ++z) {                                // X0's six first: the next block's first product needs only them
      const float* b = xp + z * zplane;
      xr[z][0] = *(const f32x4*)(okl ? b - 8 : b);
#pragma unroll
      for (int c = 0; c < 4; ++c) xr[z][1 + c] = *(const f32x4*)(b + 8 * c);
      xr[z][5] = *(const f32x4*)(okr ? b + 32 : b);
    }
  };
  // ... and the columns outside the plane become zero where the plane is first used, a product later: a select behind the load
  // would wait for it on the spot
  auto mask_x = [&](int z) __attribute__((always_inline)) {
    xr[z][0] = okl ? xr[z][0] : zero4;
#pragma unroll
    for (int c = 0; c < 4; ++c) xr[z][1 + c] = xoff >= 0 ? xr[z][1 + c] : zero4;
    xr[z][5] = okr ? xr[z][5] : zero4;
#pragma unroll
    for (int c = 0; c < 6; ++c) asm volatile("" : "+v"(xr[z][c]));   // all six HERE, in front of the product's pieces: a wait for a
  };                                                                 // column at its first use further on would wait for those too
  int xw4 = xw / 4;                                              // in 16-byte slots, as xb: the set is a run-time term, and behind a
  asm volatile("" : "+v"(xw4));                                  // float index the store would lose its alignment and be split
  auto put_q = [&](int q, const f32x4 (&d)[6], int set) __attribute__((always_inline)) {
    ((f32x4*)lds)[xw4 + set * (G::XSET / 4) + q * G::XP * 2] = xq_transform(q, d);
  };
  constexpr int LOADTAP = G::KP > 3 ? G::KP - 1 : 2;             // the X loads go out behind the last piece and the last plane of the sum
  static_assert(LOADTAP < 9, "inside the product");

#pragma unroll
  for (int k = 0; k < G::KP; ++k) lds_dma_piece<4, 18, G::NW>(lw_lds, 0, 2 * G::WSLOT, k, wvu, wvo, wrs);   // product 0: X0's of block 0
  if (ldw) load_xc(0);
  else {
#pragma unroll
    for (int c = 0; c < 12; ++c) xr[c / 6][c % 6] = zero4;
  }
  mask_x(0);
  if (stg) {
#pragma unroll
    for (int q = 0; q < 6; ++q) put_q(q, xr[0], 0);
  }
  auto block = [&](int cb, auto more_c) __attribute__((always_inline)) {
    constexpr bool more = decltype(more_c)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int n = cb * 3 + i, par = n & 1;
      const int p = 2 - i;                                       // pack product and accumulator family: X0, X1, X0 + X1
      const bool follows = i < 2 || more;                        // product n + 1 exists: pack product (i == 2 ? 2 of the next block : p - 1)
      // this wave's pieces of product n landed (the X loads issued behind them may stay in flight), its planes of it stored;
      // behind the barrier everybody's are visible, and slot and set of product n - 1 are free
      if (i == 2 && more && ldw) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xC07F);                        // lgkmcnt(0) only
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      const float* lwc = lw + par * G::WSLOT + wb;
      const int xbn = xb[0] + par * (G::XSET / 4);
      const int nsrc = (i == 2 ? cb * 3 + 5 : cb * 3 + p - 1) * G::WSLOT;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {                            // (q counts from the wave's 3 qh: in both bases)
          const int tap = ky * 3 + q;
          const f32x4 wf = *(const f32x4*)(lwc + (ky * 6 + q) * G::WTAP);
          const f32x4 xf = ((const f32x4*)lds)[xbn + xq_xtap<G>(q, ky) / 4];
          // between the tap's fragment reads and its MFMAs (behind the MFMAs the stores and the pieces held the next tap's reads
          // back until those had issued: 2 - 6 % slower at the op level, profiles/fp32_xquad_pipe.txt section 2)
          if (follows) {
            if (tap == 0 && i != 1) mask_x(i == 0 ? 1 : 0);      // X1 of this block | X0 of the next, loaded a product ago or more
            if (i == 1) {                                        // X0 + X1 in place, two planes in each of the first three taps
              if (tap == 0) {
#pragma unroll
                for (int c = 0; c < 6; ++c) xr[0][c] = xr[0][c] + xr[1][c];
              }
              if (tap < 3 && stg) { put_q(2 * tap, xr[0], par ^ 1); put_q(2 * tap + 1, xr[0], par ^ 1); }
            } else if (tap < 6 && stg) {
              put_q(tap, i == 0 ? xr[1] : xr[0], par ^ 1);       // X1 of this block | X0 of the next
            }
            if (tap < G::KP) lds_dma_piece<4, 18, G::NW>(lw_lds, (par ^ 1) * G::WSLOT, nsrc, tap, wvu, wvo, wrs);
            if (i == 1 && more && tap == LOADTAP && ldw) load_xc(cb + 1);
          }
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[kk], xf[kk], acc[p][q], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };
  for (int cb = 0; cb + 1 < nkb; ++cb) block(cb, std::true_type{});
  block(nkb - 1, std::false_type{});
  } else {
  load_x(0);
#pragma unroll
  for (int k = 0; k < G::KP; ++k) issue_piece(0, k);
  // one cin block; MORE = another block follows (the last block is its own instantiation: no branch around a piece)
  auto stage = [&](int cb, auto more_c) __attribute__((always_inline)) {
    constexpr bool more = decltype(more_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // X(cb) in registers; this wave's pieces of product 3 cb landed
    __builtin_amdgcn_s_barrier();                                // B0: every wave is through block cb - 1: the planes and the other slot are free
    asm volatile("" ::: "memory");
    if (tid < G::XITEMS) {
      put_t(2, xr[0]);                                           // X0 first: its registers then take X0 + X1 (no temporaries)
#pragma unroll
      for (int c = 0; c < 6; ++c) xr[0][c] = xr[0][c] + xr[1][c];
      put_t(0, xr[0]);
      put_t(1, xr[1]);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);                          // lgkmcnt(0) only
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();                                // B1
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (more) load_x(cb + 1);

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const int n = cb * 3 + p;
      if (p > 0) {                                               // B2, B3: this wave's pieces of product n landed, everybody's are visible
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // behind the barrier, and the slot of product n - 1 is free
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
      const float* lwc = lw + (n & 1) * G::WSLOT + wb;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {                            // (q counts from the wave's 3 qh: in both bases)
          const f32x4 wf = *(const f32x4*)(lwc + (ky * 6 + q) * G::WTAP);
          const f32x4 xf = ((const f32x4*)lds)[xb[p] + xq_xtap<G>(q, ky) / 4];
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) acc[p][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[kk], xf[kk], acc[p][q], 0, 0, 0);
          if (ky * 3 + q < G::KP && (p < 2 || more)) issue_piece(n + 1, ky * 3 + q);   // a piece of product n + 1 behind each of the first taps
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };
  for (int cb = 0; cb + 1 < nkb; ++cb) stage(cb, std::true_type{});
  stage(nkb - 1, std::false_type{});
  }

  // ---- the q halves exchange through LDS (free behind the barrier: nothing of the K loop is read or in flight any more):
  // half 0 (A0, A1, A2) hands d = A1 - A2 over and takes s' = A3 + A4, half 1 (A3, A4, A5) the reverse; a tile is
  // [16 registers / 4][64 lanes] float4, three tiles per wave
  const int qhu = __builtin_amdgcn_readfirstlane(qh);
  // ---- the tail's loads go out HERE, ahead of the exchange (header comment): bias, and the residual of the z = 0 outputs.  An
  // address is one per-lane term plus one uniform term (cout block, plane z, column pair); with res_half, (z, y >> 1, x >> 1) of
  // x = 4 c + 2 par + qh is half_res_off of column 4 c plus z (S / 2)^2 + par voxels
  const bool okv = ooff0 >= 0;
  const long yl = okv ? (long)on[0] * a.y_nstride + ooff0 + qh * 8 + 4 * h : 0;
  const long rl = okv ? (long)on[0] * a.res_nstride + (a.res_ls ? half_res_off(ooff0, a.res_ls) : ooff0 + qh * 8) + 4 * h : 0;
  const long rplane = a.res_ls ? a.y_plane >> 2 : a.y_plane;
  const int rz = a.res_ls ? S * S * 2 : S * S * 8, rp = a.res_ls ? 8 : 16;
  const float* rsrc = a.res ? a.res : a.bias;                    // no residual: the same sixteen requests, of the bias' element 0 (cached),
                                                                 // so that one straight-line tail serves both and every wait is counted
  f32x4 bv[4], rv[2][2][4];                                      // rv[z][par][g]: column 2 par + qh of plane z, cout block 4 nt + g
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int cob = nt * 4 + g;
    bv[g] = *(const f32x4*)(a.bias + (long)(cob < a.Cob ? cob : 0) * 8 + 4 * h);
  }
  auto load_res = [&](int z, int par) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cob = nt * 4 + g;
      const long uni = (long)cob * rplane + z * rz + par * rp;
      rv[z][par][g] = *(const f32x4*)(rsrc + (cob < a.Cob && okv && a.res ? rl + uni : 0));
    }
  };
  load_res(0, 0);
  load_res(0, 1);
#pragma unroll
  for (int p = 0; p < 3; ++p) {                                  // acc[p][0] = A0 | d', [1] = s | A5, [2] = d | s': the tile it sends,
    if (qhu) {                                                   // dead behind the send in BOTH halves (registers for the residual)
      const f32x16 sp = acc[p][0] + acc[p][1];
      acc[p][0] = acc[p][0] - acc[p][1];
      acc[p][1] = acc[p][2];
      acc[p][2] = sp;
    } else {
      const f32x16 s = acc[p][1] + acc[p][2];
      acc[p][2] = acc[p][1] - acc[p][2];
      acc[p][1] = s;
    }
    asm volatile("" : "+v"(acc[p][0]), "+v"(acc[p][1]), "+v"(acc[p][2]));
  }
  // every wave is through the K loop (its fragment reads have fed their MFMAs, no piece is in flight behind the last block)
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x16& tl = acc[p][2];
      const f32x4 v = {tl[4 * i], tl[4 * i + 1], tl[4 * i + 2], tl[4 * i + 3]};
      *(f32x4*)(lds + ((wv * 3 + p) * 4 + i) * 256 + lane * 4) = v;
    }
  load_res(1, 0);                                                // into the sent tiles' registers
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);                            // lgkmcnt(0) only: this wave's tiles are in LDS
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  f32x16 got[3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v = *(const f32x4*)(lds + (((wv ^ 1) * 3 + p) * 4 + i) * 256 + lane * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) got[p][4 * i + e] = v[e];
    }
  // half 0: column 0 = (A0 + s) + s', column 2 = s + 4 s';  half 1: column 1 = d + 2 d', column 3 = (d + 8 d') + A5
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    f32x16 c0, c1;
    if (qhu) {
      c0 = got[p] + 2.f * acc[p][0];
      c1 = (got[p] + 8.f * acc[p][0]) + acc[p][1];
    } else {
      c0 = (acc[p][0] + acc[p][1]) + got[p];
      c1 = acc[p][1] + 4.f * got[p];
    }
    acc[p][0] = c0;
    acc[p][1] = c1;
    asm volatile("" : "+v"(acc[p][0]), "+v"(acc[p][1]));         // formed HERE, not sunk into the guarded stores below
  }
  load_res(1, 1);                                                // into got's: all sixteen quads are requested before the first output
  // conv_epilogue's arithmetic in its order, (acc + bias) -> GELU -> res +, formed for every lane in the residual's registers (the
  // waits for the loads stand in code every lane runs, counted per quad), then the sixteen stores, which wait for nothing
#pragma unroll
  for (int z = 0; z < 2; ++z)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      f32x16 o = acc[0][par] + acc[1 + z][par];
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v;
        v[0] = o[4 * g + 0] + bv[g][0];
        v[1] = o[4 * g + 1] + bv[g][1];
        v[2] = o[4 * g + 2] + bv[g][2];
        v[3] = o[4 * g + 3] + bv[g][3];
        if (a.flags & EPI_GELU) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = gelu_tanh_hw(v[j]);
        }
        if (a.res) v = rv[z][par][g] + v;
        rv[z][par][g] = v;
        asm volatile("" : "+v"(rv[z][par][g]));                  // formed HERE: sunk into the guarded stores, its wait would count them
      }
    }
#pragma unroll
  for (int z = 0; z < 2; ++z)
#pragma unroll
    for (int par = 0; par < 2; ++par)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cob = nt * 4 + g;
        const long uni = (long)cob * a.y_plane + z * (S * S * 8) + par * 16;
        if (cob < a.Cob && okv) *(f32x4*)(a.y + yl + uni) = rv[z][par][g];
      }
}

// The second pass of a split x-quad launch: y = res + gelu?(((p0 + p1) + p2) + p3 + bias), conv_epilogue's arithmetic in its
// order over the raw sums of the ksplit partials (slices of y's own geometry, part_stride floats apart).  One float4 per lane,
// read and written by that lane alone, so res == y (the skip conv's output updated in place) is legal; it touches what the
// unsplit kernel's guarded stores touch: every lane of blocks [0, Cob) of patches [0, N).  No atomics: the sum has one order.
// The zero vector is the bias a split launch hands the conv kernel's tail.
constexpr int XQ_ZERO_FLOATS = 4096;
__device__ float xq_zero_bias[XQ_ZERO_FLOATS];
__global__ __launch_bounds__(256) void xquad_split_reduce(const float* part, long part_stride, int ksplit, const float* bias, const float* res,
                                                          long res_nstride, float* y, long y_nstride, long per_n4, int plane4, long total4,
                                                          int flags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long n = i / per_n4, rem = i - n * per_n4;               // rem: float4 index inside the patch's Cob blocks
  const long off = n * y_nstride + rem * 4;
  f32x4 v = *(const f32x4*)(part + off);
  for (int k = 1; k < ksplit; ++k) v = v + *(const f32x4*)(part + k * part_stride + off);
  v = v + *(const f32x4*)(bias + (rem / plane4) * 8 + (rem & 1) * 4);
  if (flags & EPI_GELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = gelu_tanh_hw(v[j]);
  }
  if (res) v = *(const f32x4*)(res + n * res_nstride + rem * 4) + v;
  *(f32x4*)(y + off) = v;
}

// ---- 1x1x1 conv / Linear over voxels (flat voxel tiles, KC channel blocks per stage) ----
// Replaces the skip_connection Conv3d(k=1) (model/MBAblocks.py:220-224) and every nn.Linear
// of AttnBlock / Attention / Mlp applied to '(z h w) c' tokens (model/MBAblocks.py:465,
// 538-544; timm Mlp fc1/fc2).
// WN = cout tiles of 32 per wave: 2 (64-cout workgroup tile) or 4 (128-cout tile: half the activation bytes per
// FLOP -- at 64 couts this kernel is bound by the L2 -> LDS staging rate, not by the matrix pipe)
template <int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv1_mfma(ConvArgs a) {
  constexpr int MV = 4 * WM * 32;
  constexpr int KC = 4;
  constexpr int XP = KC * MV * 2 / 256;       // x pieces per thread
  constexpr int NT64 = WN / 2;                // 64-cout weight tiles per workgroup
  constexpr int WP = NT64 * KC * 64 * 2 / 256;
  __shared__ __attribute__((aligned(16))) float lds[NT64 * KC * 512 + KC * MV * 8];
  float* lw = lds;                            // [NT64][KC][64][8]
  float* lx = lds + NT64 * KC * 512;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int i32 = lane & 31, h = lane >> 5;
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int nt = bid % a.ntile;
  const int mtile = bid / a.ntile;
  const long VPN = (long)a.Z * a.S * a.S;      // voxels per n
  const long vtot = VPN * a.N;

  long xoff[XP];
  int xkc[XP];
#pragma unroll
  for (int k = 0; k < XP; ++k) {
    const int i = tid + k * 256;
    const int half = i & 1;
    const int v = (i >> 1) % MV;
    xkc[k] = (i >> 1) / MV;
    const long vg = (long)mtile * MV + v;
    long off = -1;
    if (vg < vtot) {
      const long n = vg / VPN;
      off = n * a.x_nstride + (vg - n * VPN) * 8 + half * 4;
    }
    xoff[k] = off;
  }
  // piece i = tid + k*256 of the weight stage: 64-cout tile i / (KC*128), then [KC][64][2] inside it
  const float* wsrc = a.w + (long)nt * NT64 * a.Cbi * 512;

  int xb[WM], on[WM], ooff[WM];
#pragma unroll
  for (int mt = 0; mt < WM; ++mt) {
    const int v = (wv * WM + mt) * 32 + i32;
    xb[mt] = v * 8 + 4 * h;
    const long vg = (long)mtile * MV + v;
    if (vg < vtot) {
      const long n = vg / VPN;
      on[mt] = (int)n;
      ooff[mt] = (int)((vg - n * VPN) * 8);
    } else { on[mt] = 0; ooff[mt] = -1; }
  }
  const int wb = i32 * 8 + 4 * h;

  f32x16 acc[WN][WM];
#pragma unroll
  for (int ct = 0; ct < WN; ++ct)
#pragma unroll
    for (int mt = 0; mt < WM; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][mt][r] = 0.f;

  f32x4 xr[XP], wr[WP];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_stage = [&](int cb0) {
#pragma unroll
    for (int k = 0; k < XP; ++k) {
      const int cb = cb0 + xkc[k];
      xr[k] = (xoff[k] >= 0 && cb < a.Cbi) ? *(const f32x4*)(a.x + (long)cb * a.x_plane + xoff[k]) : zero4;
    }
#pragma unroll
    for (int k = 0; k < WP; ++k) {
      const int i = tid + k * 256;
      const int t64 = i / (KC * 128), j = i - t64 * (KC * 128);
      const int cb = cb0 + j / 128;
      wr[k] = (cb < a.Cbi) ? *(const f32x4*)(wsrc + ((long)t64 * a.Cbi + cb0) * 512 + j * 4) : zero4;
    }
  };

  load_stage(0);
  for (int cb0 = 0; cb0 < a.Cbi; cb0 += KC) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < XP; ++k) *(f32x4*)(lx + (tid + k * 256) * 4) = xr[k];
#pragma unroll
    for (int k = 0; k < WP; ++k) *(f32x4*)(lw + (tid + k * 256) * 4) = wr[k];
    __syncthreads();
    if (cb0 + KC < a.Cbi) load_stage(cb0 + KC);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      f32x4 wf[WN], xf[WM];
#pragma unroll
      for (int ct = 0; ct < WN; ++ct) wf[ct] = *(const f32x4*)(lw + (ct >> 1) * (KC * 512) + kc * 512 + (ct & 1) * 256 + wb);
#pragma unroll
      for (int mt = 0; mt < WM; ++mt) xf[mt] = *(const f32x4*)(lx + kc * MV * 8 + xb[mt]);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int ct = 0; ct < WN; ++ct)
#pragma unroll
          for (int mt = 0; mt < WM; ++mt)
            acc[ct][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[ct][kk], xf[mt][kk], acc[ct][mt], 0, 0, 0);
    }
  }
  conv_epilogue<WM, WN>(a, acc, nt, h, on, ooff, 0);
}

// ---- launch-size rule and launcher of the MFMA convs ----
// A launch of `vox` voxels and `tiles` tile columns (cout tiles, x 4 phases for the upsampled forms) takes its large tile where
// 256-voxel workgroups of it still make 512: below that, smaller workgroups fill more CUs.
static bool conv_fills_chip(long vox, long tiles) { return (vox / 256) * tiles >= 512; }

// The instantiation of conv1_mfma a 1x1x1 launch of `vox` voxels and `ntile` 64-cout tiles runs: 1 = <1, 2> (128 voxels x 64
// couts per workgroup), 2 = <2, 2> (256 x 64), 3 = <2, 4> (256 x 128: pairs of cout tiles, so ntile must be even).
// tile_variant 0 chooses by launch size: 256-voxel tiles from 512 workgroups of them, the 128-cout tile where those still make
// 512; 1 and 2 force the voxel tile (2 keeps the size rule for the cout tile); 3 forces the 128-cout tile whatever the size
// and is refused (0) on an odd ntile.
int conv1_form(long vox, int ntile, int tile_variant) {
  if (tile_variant == 3) return (ntile & 1) == 0 ? 3 : 0;
  const int variant = tile_variant ? tile_variant : (conv_fills_chip(vox, ntile) ? 2 : 1);
  if (variant == 2 && (ntile & 1) == 0 && conv_fills_chip(vox, ntile / 2)) return 3;
  return variant == 2 ? 2 : 1;
}

// The workgroups an x-quad launch of `ovox` output voxels and `ntile` 64-cout tiles would have in its large tile, and whether it is
// one of the launches in which the small tile is the faster one: planes of 64 x 64 and up with eight large workgroups per CU or
// more (what was measured: the S = 64 levels at 128 patches, whose K loops of 8 and 12 cin blocks are the shortest of the step)
static long xquad_large_wgs(long ovox, int ntile) { return (ovox / 1024) * 2 * ntile; }
static bool xquad_many_wgs(long ovox, int ntile, int S) { return S >= 64 && xquad_large_wgs(ovox, ntile) >= 2048; }

// Split K of the x-quad form (tm_kernels.h has the statement).  A launch below 256 large workgroups takes the small tile, of
// ceil(ovox / 512) * ceil(Cout / 32) workgroups; where those are fewer than XQUAD_SPLIT_WGS, K-ranges of a tile go to
// different workgroups (profiles/fp32_xquad_splitk.txt: the factors measured at the launches of the step).  The factor is 2
// however few the workgroups are: 4 never beat 2
int xquad_ksplit(long ovox, int Cout, int Cbi, int S, bool res_half) {
  if (!xquad_split_on() || res_half || S < 8 || xquad_large_wgs(ovox, (Cout + 63) / 64) >= 256) return 1;
  const long small = (ovox + 511) / 512 * ((Cout + 31) / 32);
  return small < XQUAD_SPLIT_WGS && Cbi / 2 >= XQUAD_SPLIT_FLOOR ? 2 : 1;
}

int conv_tile(int form, long ovox, int ntile, int S, int tile_variant) {
  if (S == 4) return 1;                        // 4 x 4 planes: several patches per workgroup of the small tile
  // x-quad: the large tile is 1024 voxels x 32 couts on eight waves, one workgroup per CU, whose head and tail nothing covers: taken
  // where it still gives every CU one workgroup, except at S >= 64 from 2048 large workgroups on (the S = 64 levels at 128
  // patches): there the small tile, two workgroups per CU that cover each other's head and tail, wins by 6 - 7 % at the op
  // level; at 512 workgroups of S = 64 and at 1024 of S = 32 the two tie (profiles/fp32_xquad_tail.txt section 3)
  if (form == CF_XQUAD)
    return tile_variant ? (tile_variant == 2 ? 2 : 1) : (xquad_large_wgs(ovox, ntile) >= 256 && !xquad_many_wgs(ovox, ntile, S) ? 2 : 1);
  const long tiles = (form == CF_ZSKIP_UPS || form == CF_PAIR_UPS) ? 4L * ntile : ntile;
  const int variant = tile_variant ? tile_variant : (conv_fills_chip(ovox, tiles) ? 2 : 1);
  return variant == 2 ? 2 : 1;
}

// The schedule of conv3d_xquad a launch takes where the caller forces none: the pipelined one (PIPE = 1) in the instantiations
// <half, tw> where it won at the op level (profiles/fp32_xquad_pipe.txt), and in the small tile <1, 16> of a launch that takes it
// for its many workgroups (`many`: xquad_many_wgs), where only the pipelined schedule beats the large tile by the rule
// (profiles/fp32_xquad_tail.txt section 3); TM_CONV_XQUAD_PIPE=0 (read once) keeps the four-barrier schedule everywhere.  The
// form and the pack are the same in both, so conv_pick_form does not see the switch.
static bool xquad_pipe_default(bool half, int tw, bool many) {
  static const bool on = [] {
    const char* v = getenv("TM_CONV_XQUAD_PIPE");
    return !(v && atoi(v) == 0);
  }();
  return on && tw == 16 && (!half || many);    // <0, 8> ties or loses by 2 %, the small tiles of the small launches lose 6 - 16 %
}

// One k x 3 x 3 launch: KERN over the tiles of geometry G (TW x TR voxels of NPB patches, LDS_BYTES of dynamic LDS), `factor`
// workgroups per (patch group, tile, cout tile): output planes and / or the four phases.
template <void (*KERN)(ConvArgs), class G, int BLOCK = 256>
static hipError_t launch_tiled(const ConvArgs& a, long factor, hipStream_t s) {
  static DevOnce attr_once;
  if (attr_once.need()) {
    hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_once.mark();
  }
  const long tiles = (long)(a.S / G::TW_) * (a.S / G::TR);
  const long pgs = (a.N + G::NPB - 1) / G::NPB;
  hipLaunchKernelGGL(KERN, dim3((unsigned)(pgs * tiles * factor * a.ntile)), dim3(BLOCK), G::LDS_BYTES, s, a);
  return hipGetLastError();
}
// f(TW) with the tile width of a plane of S = 8 .. 128 as a compile-time constant
template <int MAXTW, class F>
static hipError_t with_tile_width(int S, F f) {
  if constexpr (MAXTW >= 32)
    if (S >= 32) return f(std::integral_constant<int, 32>{});
  if (S >= 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 8>{});
}
template <int NZI, bool UPS>
static hipError_t launch_c3(const ConvArgs& a, bool large, hipStream_t s) {
  const long factor = UPS ? 4L * a.Z : a.Z;
  if (a.S == 4) return launch_tiled<conv3d_mfma<NZI, 1, 4, UPS>, C3Geo<NZI, 1, 4, UPS>>(a, factor, s);
  return with_tile_width<32>(a.S, [&](auto tw) {
    constexpr int TW = decltype(tw)::value;
    return large ? launch_tiled<conv3d_mfma<NZI, 2, TW, UPS>, C3Geo<NZI, 2, TW, UPS>>(a, factor, s)
                 : launch_tiled<conv3d_mfma<NZI, 1, TW, UPS>, C3Geo<NZI, 1, TW, UPS>>(a, factor, s);
  });
}

hipError_t launch_conv_mfma(const ConvLaunch& L, hipStream_t s) {
  ConvArgs a;
  a.x = L.x.p; a.x_nstride = L.x.nstride; a.x_plane = L.x.plane();
  a.w = L.w.w; a.bias = L.w.bias;
  a.y = L.y.p; a.y_nstride = L.y.nstride; a.y_plane = L.y.plane(); a.Cob = L.y.Cb;
  a.res = L.res ? L.res->p : nullptr; a.res_nstride = L.res ? L.res->nstride : 0;
  a.gate = L.gate ? L.gate->p : nullptr; a.gate_nstride = L.gate ? L.gate->nstride : 0;
  const int form = L.w.form;
  if (L.w.taps != conv_form_taps(form)) return hipErrorInvalidValue;
  if (L.gate_half) {
    int ls = 0;
    while ((1 << ls) < L.y.H) ++ls;
    if (!L.gate || form != CF_1X1 || (1 << ls) != L.y.H || L.y.H != L.y.W || ls < 1) return hipErrorInvalidValue;
    a.gate_ls = ls;
  }
  a.N = L.x.N; a.S = L.x.H; a.Z = L.x.Z; a.Cbi = L.w.Cbi; a.ntile = L.w.ntile; a.flags = L.flags;
  if (L.x.Cb != L.w.Cbi || L.x.H != L.x.W) return hipErrorInvalidValue;
  if (L.fuse_norm) {             // the pair form's 128-voxel tile at 64 couts only; everything else is refused before any device call
    if (form != CF_PAIR || L.zmode != ZM_PAD1 || L.x.Z != 2 || L.w.Cout != 64 || L.w.ntile != 1 || L.res || L.gate || L.flags ||
        !L.norm_w || !L.mod_scale || !L.mod_shift || L.per_image < 1)
      return hipErrorInvalidValue;
    if (conv_tile(form, (long)L.x.N * 2 * L.x.H * L.x.H, 1, L.x.H, L.tile_variant) != 2) return hipErrorInvalidValue;
    if (!L.a2.p || L.a2.Cb != 8 || L.a2.N != L.x.N || L.a2.Z != 2 || L.a2.H != L.x.H || L.a2.W != L.x.H) return hipErrorInvalidValue;
    if (L.y.Cb != 8 || L.y.Z != 2 || L.y.H != L.x.H) return hipErrorInvalidValue;       // y carries the geometry only
    a.y = L.a2.p; a.y_nstride = L.a2.nstride; a.y_plane = L.a2.plane();
    a.norm_w = L.norm_w; a.mod_scale = L.mod_scale; a.mod_shift = L.mod_shift; a.mod_stride = L.mod_stride;
    a.per_image = L.per_image; a.inv_c = L.inv_c;
  }
  if (L.y.Cb > L.w.ntile * 8 || L.y.N != L.x.N) return hipErrorInvalidValue;
  const long vox = (long)a.N * a.Z * a.S * a.S;
  if (form == CF_1X1) {
    if (L.flags & EPI_UP2) return hipErrorInvalidValue;
    if (L.y.H != L.x.H || L.y.Z != L.x.Z) return hipErrorInvalidValue;
    const int form1 = conv1_form(vox, a.ntile, L.tile_variant);
    if (form1 == 3) {
      const long mt = (vox + 255) / 256;                  // 128-cout x 256-voxel workgroups
      a.ntile /= 2;
      hipLaunchKernelGGL((conv1_mfma<2, 4>), dim3((unsigned)(mt * a.ntile)), dim3(256), 0, s, a);
    } else if (form1 == 2) {
      const long mt = (vox + 255) / 256;
      hipLaunchKernelGGL((conv1_mfma<2, 2>), dim3((unsigned)(mt * a.ntile)), dim3(256), 0, s, a);
    } else if (form1 == 1) {
      const long mt = (vox + 127) / 128;
      hipLaunchKernelGGL((conv1_mfma<1, 2>), dim3((unsigned)(mt * a.ntile)), dim3(256), 0, s, a);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
  }
  // ---- k x 3 x 3 kernels: what each form takes; zmode is the caller's statement and must agree with the form ----
  const int S = a.S;
  const bool z2 = L.x.Z == 2 && L.y.Z == 2, up2 = (L.flags & EPI_UP2) != 0;
  a.Zin = L.x.Z; a.zoff = 0;
  switch (form) {
    case CF_INPLANE:               // 1x3x3 at any Z, or 3x3x3 pad 1 on ONE plane: only the centre z slice meets data
      if (L.zmode == ZM_PAD1 ? (L.x.Z != 1 || L.y.Z != 1) : (L.zmode != ZM_INPLANE || L.y.Z != L.x.Z)) return hipErrorInvalidValue;
      break;
    case CF_PLANES3:               // 3x3x3 valid in z, or pad 1 (planes outside [0, Zin) zero) at any Z but the 2 of CF_ZSKIP
      if (L.zmode == ZM_PAD1 ? (L.y.Z != L.x.Z || L.x.Z == 2) : (L.zmode != ZM_VALID || L.y.Z != L.x.Z - 2)) return hipErrorInvalidValue;
      if (L.zmode == ZM_PAD1) a.zoff = -1;
      break;
    case CF_ZSKIP: case CF_PAIR:   // 3x3x3 pad 1 over two planes
      if (L.zmode != ZM_PAD1 || !z2) return hipErrorInvalidValue;
      break;
    case CF_XQUAD:                 // ... with Winograd along x: planes of at least 8 x 8; its own epilogue (bias, GELU flag
      if (L.zmode != ZM_PAD1 || !z2 || L.x.H < 8 || up2 || L.gate) return hipErrorInvalidValue;   // and residual): no gate
      break;
    case CF_ZSKIP_UPS: case CF_PAIR_UPS:   // 3x3x3 pad 1 of the nearest-x2 upsampled x, on the low-resolution x
      if (L.zmode != ZM_UPS || !z2 || up2 || L.res || L.gate) return hipErrorInvalidValue;
      break;
    default: return hipErrorInvalidValue;
  }
  a.Z = L.y.Z;
  if (S != 4 && S != 8 && S != 16 && S != 32 && S != 64 && S != 128) return hipErrorInvalidValue;
  if ((up2 || L.zmode == ZM_UPS) ? (L.y.H != 2 * S) : (L.y.H != S)) return hipErrorInvalidValue;
  if (L.res_half) {
    int ls = 0;
    while ((1 << ls) < L.y.H) ++ls;
    if (!L.res || (1 << ls) != L.y.H || L.y.H != L.y.W || ls < 1 || up2) return hipErrorInvalidValue;
    a.res_ls = ls;
  }
  // the form is the layer's (fixed at pack time); the tile follows the launch size
  const bool large = conv_tile(form, (long)a.N * a.Z * a.S * a.S, a.ntile, S, L.tile_variant) == 2;
  switch (form) {
    case CF_INPLANE: return launch_c3<1, false>(a, large, s);
    case CF_PLANES3: return launch_c3<3, false>(a, large, s);
    case CF_ZSKIP: return launch_c3<2, false>(a, large, s);
    case CF_ZSKIP_UPS: return launch_c3<2, true>(a, large, s);
    case CF_PAIR:
      if (S == 4) return launch_tiled<conv3d_zpair<1, 4, false>, ZPGeo<1, 4>>(a, 1, s);   // 4 patches per workgroup (8 would not
      return with_tile_width<32>(S, [&](auto tw) {                                        // leave LDS for two workgroups per CU)
        constexpr int TW = decltype(tw)::value;
        if (L.fuse_norm) return launch_tiled<conv3d_zpair<0, TW, true>, ZPGeo<0, TW>>(a, 1, s);   // the 128-voxel tile: checked above
        return large ? launch_tiled<conv3d_zpair<0, TW, false>, ZPGeo<0, TW>>(a, 1, s)
                     : launch_tiled<conv3d_zpair<1, TW, false>, ZPGeo<1, TW>>(a, 1, s);
      });
    case CF_PAIR_UPS:
      if (S == 4) return launch_tiled<conv3d_zpair_ups<1, 4>, ZPUGeo<1, 4>>(a, 4, s);
      return with_tile_width<32>(S, [&](auto tw) {
        constexpr int TW = decltype(tw)::value;
        return large ? launch_tiled<conv3d_zpair_ups<0, TW>, ZPUGeo<0, TW>>(a, 4, s)
                     : launch_tiled<conv3d_zpair_ups<1, TW>, ZPUGeo<1, TW>>(a, 4, s);
      });
    default: {   // CF_XQUAD
      a.ntile = (L.w.Cout + 31) / 32;                          // the kernel's cout tiles are of 32 (the pack holds 2 * ntile of them)
      if (L.xquad_sched < -1 || L.xquad_sched > 1) return hipErrorInvalidValue;
      // split K: the conv writes raw sums (a bias of zeros, no residual, no flags) into the partials, the reduction finishes y
      const int ksp = L.xquad_ksplit;
      if (ksp != 1) {
        if ((ksp != 2 && ksp != 4) || ksp > a.Cbi || !L.part || L.res_half || L.y.Cb * 8 > XQ_ZERO_FLOATS) return hipErrorInvalidValue;
        float* zeros = nullptr;
        if (hipError_t e = hipGetSymbolAddress((void**)&zeros, HIP_SYMBOL(xq_zero_bias)); e != hipSuccess) return e;
        a.ksplit = ksp; a.part_stride = (long)L.y.N * L.y.nstride;
        a.y = L.part; a.bias = zeros; a.res = nullptr; a.res_nstride = 0; a.flags = 0;
      }
      const hipError_t e = with_tile_width<16>(S, [&](auto tw) {
        constexpr int TW = decltype(tw)::value;
        if (L.xquad_sched < 0 ? xquad_pipe_default(!large, TW, xquad_many_wgs((long)a.N * a.Z * a.S * a.S, L.w.ntile, S)) : L.xquad_sched == 1)
          return large ? launch_tiled<conv3d_xquad<0, TW, 1>, XQGeo<0, TW, 1>, 64 * XQGeo<0, TW, 1>::NW>(a, ksp, s)
                       : launch_tiled<conv3d_xquad<1, TW, 1>, XQGeo<1, TW, 1>, 64 * XQGeo<1, TW, 1>::NW>(a, ksp, s);
        return large ? launch_tiled<conv3d_xquad<0, TW, 0>, XQGeo<0, TW, 0>, 64 * XQGeo<0, TW, 0>::NW>(a, ksp, s)
                     : launch_tiled<conv3d_xquad<1, TW, 0>, XQGeo<1, TW, 0>, 64 * XQGeo<1, TW, 0>::NW>(a, ksp, s);
      });
      if (e != hipSuccess || ksp == 1) return e;
      const int plane4 = (int)(L.y.plane() / 4);
      const long per_n4 = (long)L.y.Cb * plane4, total4 = per_n4 * L.y.N;
      hipLaunchKernelGGL(xquad_split_reduce, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, L.part, a.part_stride, ksp, L.w.bias,
                         L.res ? L.res->p : nullptr, L.res ? L.res->nstride : 0, L.y.p, L.y.nstride, per_n4, plane4, total4, L.flags);
      return hipGetLastError();
    }
  }
}

// ---- the lane -> LDS address maps of the three LDS-DMA conv kernels, evaluated on the host (no device call) ----
// The same functions the kernels address with (tm_conv_frag.h, conv_lane_of, zp_wtap / zp_xtap / xq_xtap), composed as the
// kernels compose them: out[lane] = byte address inside the workgroup's dynamic LDS of what lane `lane` of wave wv reads or
// stores, -1 for a lane that stores nothing.  what 0: the weight fragment of tap (p, ky, kx) and 32-cout sub-tile `sub` (slot 0
// of a ring); 1: the X fragment of (p, ky, kx), `sub` = the output phase 2 py + px of the upsampled form; 2: the staging store
// into plane p of the thread's item ky (its k-th of PX).
template <class G, int HALF, int TW, bool UPS>
static int zpair_frag_addrs(int what, int wv, int p, int ky, int kx, int sub, int* out) {
  constexpr int NC = HALF ? 1 : 2, KW = UPS ? 2 : 3;
  constexpr int lx = G::LDS_BYTES / 4 - 3 * G::XV * 8;           // the X planes close the allocation
  if (p < 0 || p > 2) return -1;
  if (what == 2 ? (ky < 0 || ky >= G::PX) : (ky < 0 || ky >= KW || kx < 0 || kx >= KW)) return -1;
  if (what == 0 ? (sub < 0 || sub >= NC) : what == 1 ? (sub < 0 || sub > (UPS ? 3 : 0)) : false) return -1;
  const int vt = HALF ? (wv & 1) : wv, ct0 = HALF ? (wv >> 1) : 0;
  for (int lane = 0; lane < 64; ++lane) {
    const int i32 = lane & 31, h = lane >> 5;
    int a = -1;
    if (what == 0) a = zp_wtap(UPS ? p * 4 + ky * 2 + kx : p * 9 + ky * 3 + kx, sub) + conv_w_off(ct0 * 32 + i32, 4 * h);
    else if (what == 1)
      a = lx + zp_xtap<G>(p, ky, kx) + conv_lane_of<G::TR, TW, G::PS, G::HC, G::XV>(vt * 32 + conv_lane_voxel(TW, i32), h, sub >> 1, sub & 1).xb;
    else {
      const int i = wv * 64 + lane + ky * 256;
      if (conv_stage_row(i) < G::XV) a = lx + p * G::XV * 8 + conv_frag_off(conv_stage_row(i), conv_stage_half(i), G::XV);
    }
    out[lane] = a < 0 ? -1 : a * 4;
  }
  return 0;
}
// conv3d_xquad: kx is the wave's q (0 .. 2), in what 2 the q-plane (0 .. 5), ky 0.
// set: the plane set of an X fragment or a staging store: the product's own in the four-barrier schedule, the ring's set (0 | 1)
// in the pipelined one
template <int HALF, int TW, int PIPE>
static int xquad_frag_addrs(int what, int wv, int p, int ky, int q, int set, int* out) {
  using G = XQGeo<HALF, TW, PIPE>;
  if (wv >= G::NW || p < 0 || p > 2 || q < 0 || q >= (what == 2 ? 6 : 3) || ky < 0 || ky > (what == 2 ? 0 : 2)) return -1;
  if (set < 0 || set >= G::NSET) return -1;
  const int gt = wv >> 1, qh = wv & 1;
  for (int lane = 0; lane < 64; ++lane) {
    const int i32 = lane & 31, h = lane >> 5, tid = wv * 64 + lane;
    int a = -1;
    if (what == 0) a = 3 * qh * G::WTAP + conv_frag_off(i32, h, 32) + (ky * 6 + q) * G::WTAP;
    else if (what == 1)
      a = 2 * G::WSLOT + xq_xtap<G>(q, ky) +
          xq_xfrag<G>(set, qh, conv_lane_of<G::TR, G::GW, G::HR * G::GW, G::GW, G::XP>(gt * 32 + xq_lane_group(TW, i32), h, 0, 0).xb);
    else if (tid < G::XITEMS)
      a = 2 * G::WSLOT + xq_xstage<G>(set, q, tid);
    out[lane] = a < 0 ? -1 : a * 4;
  }
  return 0;
}
int conv_xquad_lds_bytes(int half, int tw, int sched) {
  if (half < 0 || half > 1 || (tw != 8 && tw != 16) || sched < 0 || sched > 1) return -1;
  if (sched) return half ? (tw == 8 ? XQGeo<1, 8, 1>::LDS_BYTES : XQGeo<1, 16, 1>::LDS_BYTES) : (tw == 8 ? XQGeo<0, 8, 1>::LDS_BYTES : XQGeo<0, 16, 1>::LDS_BYTES);
  return half ? (tw == 8 ? XQGeo<1, 8, 0>::LDS_BYTES : XQGeo<1, 16, 0>::LDS_BYTES) : (tw == 8 ? XQGeo<0, 8, 0>::LDS_BYTES : XQGeo<0, 16, 0>::LDS_BYTES);
}
int conv_frag_addrs(int kernel, int half, int tw, int what, int wv, int p, int ky, int kx, int sub, int* out) {
  const bool xq = kernel == 4 || kernel == 5;
  if (!out || kernel < 0 || kernel > 5 || kernel == 2 || kernel == 3 || half < 0 || half > 1 || what < 0 || what > 2 || wv < 0 || wv > (xq ? 7 : 3)) return -1;
  if (kernel == 4 && tw == 8) return half ? xquad_frag_addrs<1, 8, 0>(what, wv, p, ky, kx, p, out) : xquad_frag_addrs<0, 8, 0>(what, wv, p, ky, kx, p, out);
  if (kernel == 4 && tw == 16) return half ? xquad_frag_addrs<1, 16, 0>(what, wv, p, ky, kx, p, out) : xquad_frag_addrs<0, 16, 0>(what, wv, p, ky, kx, p, out);
  // the pipelined schedule: sub = the plane set (0 for a weight fragment: slot 0 of the ring)
  if (kernel == 5 && what == 0 && sub != 0) return -1;
  if (kernel == 5 && tw == 8) return half ? xquad_frag_addrs<1, 8, 1>(what, wv, p, ky, kx, sub, out) : xquad_frag_addrs<0, 8, 1>(what, wv, p, ky, kx, sub, out);
  if (kernel == 5 && tw == 16) return half ? xquad_frag_addrs<1, 16, 1>(what, wv, p, ky, kx, sub, out) : xquad_frag_addrs<0, 16, 1>(what, wv, p, ky, kx, sub, out);
  if (xq) return -1;
#define TM_FRAG(H, T)                                                                                              \
  if (half == H && tw == T) {                                                                                      \
    if (kernel == 0) return zpair_frag_addrs<ZPGeo<H, T>, H, T, false>(what, wv, p, ky, kx, sub, out);              \
    if (kernel == 1) return zpair_frag_addrs<ZPUGeo<H, T>, H, T, true>(what, wv, p, ky, kx, sub, out);              \
  }
  TM_FRAG(1, 4) TM_FRAG(0, 8) TM_FRAG(1, 8) TM_FRAG(0, 16) TM_FRAG(1, 16) TM_FRAG(0, 32) TM_FRAG(1, 32)
#undef TM_FRAG
  return -1;                                                     // no such instantiation
}

// ==========================================================================================
// prep: gather (concat / collage / nearest-up / avg-down) + LlamaRMSNorm over C + modulate +
// SiLU, written as the activated conv input.  Replaces th.cat + to_collage
// (model/unet_ours.py:325-341,384,418), LlamaRMSNorm(dim=1) (model/MBAblocks.py:21-43), the
// scale/shift of apply_conditions (:356-367), modulate (:608-614), nn.SiLU and
// Upsample / Downsample (model/blocks.py:362-371,389-403) as they occur in ResBlock._forward
// (:254-261) and AttnBlock._forward (:484-489).
// 64 voxels per workgroup (lane = voxel: 2 KB contiguous per wave load), the 4 waves split
// the channel blocks and combine their sums of squares through LDS.
// ==========================================================================================
struct PrepArgs { PrepLaunch L; };
struct PrepDropArgs { PrepLaunch L; DropRng r; };
__device__ __forceinline__ DropRng rng_of(const PrepArgs&) { return DropRng{0ull, 0u, 0u}; }
__device__ __forceinline__ DropRng rng_of(const PrepDropArgs& a) { return a.r; }

// CACHED: the voxel's channel blocks owned by this wave (<= 8) stay in registers between the
// sum-of-squares pass and the apply pass, so every source byte is read from HBM once.
// DRAW (NSUB 1, fp32 out; args PrepDropArgs): the training dropout keep mask is drawn here (drop_keep8, one Philox pair per
// channel block) instead of read from drop_mask.  Its own instantiations: the inference ones compile as without it.
// WV > 4, the wide resident form (NSUB 1, CACHED, fp32 sources and fp32 out; launch_prep picks it for 33..160 channel blocks):
// WV waves split the channel blocks of the 64 voxels, NCW blocks each, so that up to 1280 channels stay in registers and every
// source byte is read once.  All of a wave's loads are issued before the first use, unconditionally (a block past the end re-reads
// the wave's last real one, an invalid lane reads voxel 0).  The sum of squares keeps the four-wave form's association -- four
// chains over the blocks r, r + 4, r + 8, ... in ascending order from 0.f, then c0 + c1 + c2 + c3: every wave leaves the 8-term sum
// (sumsq8) of each of its blocks in LDS and waves 0..3 form the chains -- so the result is bit-identical to prep_kernel<1, false>.
// sumsq8 is one function so that every form hands the compiler the same expression to contract; that it does contract it the
// same way in the rolled loop, the cached loop and the store to LDS is held by tests/test_gpu_prep_wide.py (bit equality of the
// forms), not by the language: a compiler that splits them shows there first.
__device__ __forceinline__ float sumsq8(const f32x4& a0, const f32x4& a1) {
  return a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2] + a0[3] * a0[3] + a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2] + a1[3] * a1[3];
}
template <int NSUB, bool CACHED, bool DRAW = false, class Args = PrepArgs, int WV = 4, int NCW = 8>
__global__ __launch_bounds__(WV * 64) void prep_kernel(Args pa) {
  constexpr bool WIDE = WV > 4;
  static_assert(!WIDE || (NSUB == 1 && CACHED && !DRAW && WV * NCW >= 4), "the wide form is a cached NSUB 1 form");
  const PrepLaunch& L = pa.L;
  const DropRng R = rng_of(pa);
  __shared__ float red[4][NSUB][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = WIDE ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int S = L.S, Z = L.Z;
  const long vpn = (long)Z * S * S;
  const long vidx = (long)blockIdx.x * 64 + lane;
  const bool valid = vidx < vpn * L.N;
  int n = 0, z = 0, y = 0, x = 0;
  if (valid) {
    n = (int)(vidx / vpn);
    int rem = (int)(vidx - (long)n * vpn);
    z = rem / (S * S); rem -= z * S * S;
    y = rem / S; x = rem - y * S;
  }
  // source offsets
  long soff[3][NSUB];
  long splane[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k >= L.nsrc) { splane[k] = 0; continue; }
    int Ss = S;
    if (L.resample == RS_UP2) Ss = S / 2;
    if (L.resample == RS_DOWN2 || L.resample == RS_PICK2) Ss = S * 2;
    splane[k] = (long)Z * Ss * Ss * 8;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      // the voxel's coordinates in the source plane, then (collage) half a source patch down / right into the neighbour
      int ns = n, ys = y, xs = x;
      if (L.resample == RS_UP2) { ys = y >> 1; xs = x >> 1; }
      if (L.resample == RS_DOWN2) { ys = 2 * y + (sub >> 1); xs = 2 * x + (sub & 1); }
      if (L.resample == RS_PICK2) { ys = 2 * y; xs = 2 * x; }
      if (L.src[k].collage) {
        const int q1 = L.p1 - 1, q2 = L.p2 - 1;
        const int bi = n / (q1 * q2);
        const int q = n - bi * q1 * q2;
        int i = q / q2, j = q - i * q2;
        ys += Ss / 2; if (ys >= Ss) { ys -= Ss; i += 1; }
        xs += Ss / 2; if (xs >= Ss) { xs -= Ss; j += 1; }
        ns = bi * L.p1 * L.p2 + i * L.p2 + j;
      }
      soff[k][sub] = (long)ns * L.src[k].nstride + ((long)(z * Ss + ys) * Ss + xs) * 8;
    }
  }
  // this wave owns the virtual (concatenated) channel blocks gb = wv, wv + 4, wv + 8, ...
  const int cb0 = L.src[0].Cb, cb01 = cb0 + ((L.nsrc > 1) ? L.src[1].Cb : 0);
  const int cbtot = cb01 + ((L.nsrc > 2) ? L.src[2].Cb : 0);
  // 8 channels of one voxel of the virtual (concatenated) block gb: fp32 sources (32 bytes) or, with src_h, 16-bit
  // sources (16 bytes; offsets and strides are in elements either way)
  auto load8 = [&](int gb, int sub, f32x4& a0, f32x4& a1) {
    const int k = (gb >= cb0) + (gb >= cb01);
    const int cb = gb - (k == 0 ? 0 : (k == 1 ? cb0 : cb01));
    const long off = soff[k][sub] + (long)cb * splane[k];
    if (L.src_h) {
      const uint16_t* p = (const uint16_t*)L.src[k].p + off;
      if (L.h_f16) {
        typedef _Float16 f16x8_s __attribute__((ext_vector_type(8)));
        const f16x8_s v = *(const f16x8_s*)p;
        a0 = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        a1 = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
      } else {
        typedef __bf16 bf16x8_s __attribute__((ext_vector_type(8)));
        const bf16x8_s v = *(const bf16x8_s*)p;
        a0 = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        a1 = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
      }
    } else {
      const float* p = L.src[k].p + off;
      a0 = *(const f32x4*)p; a1 = *(const f32x4*)(p + 4);
    }
  };
  constexpr int NC = CACHED ? NCW : 1;
  f32x4 c0[NC], c1[NC];            // CACHED only (NSUB == 1)

  float rstd[NSUB];
#pragma unroll
  for (int sub = 0; sub < NSUB; ++sub) rstd[sub] = 1.f;
  if (L.norm_w || CACHED) {
    float ssq[NSUB];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) ssq[sub] = 0.f;
    if constexpr (WIDE) {
      __shared__ float bsum[PREP_WIDE_MAX_CB][64];
      const int glast = wv < cbtot ? cbtot - 1 - ((cbtot - 1 - wv) % WV) : 0;    // the wave's last real block
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const int gb = min(wv + WV * i, glast);
        const int k = (gb >= cb0) + (gb >= cb01);              // wave-uniform
        const int cb = gb - (k == 0 ? 0 : (k == 1 ? cb0 : cb01));
        const float* sp = k == 0 ? L.src[0].p : (k == 1 ? L.src[1].p : L.src[2].p);
        const float* p = sp + (k == 0 ? soff[0][0] : (k == 1 ? soff[1][0] : soff[2][0])) +
                         (long)cb * (k == 0 ? splane[0] : (k == 1 ? splane[1] : splane[2]));
        c0[i] = *(const f32x4*)p; c1[i] = *(const f32x4*)(p + 4);
      }
      if (L.norm_w) {
#pragma unroll
        for (int i = 0; i < NC; ++i)
          if (wv + WV * i < cbtot) bsum[wv + WV * i][lane] = sumsq8(c0[i], c1[i]);
        __syncthreads();
        if (wv < 4)
          for (int gb = wv; gb < cbtot; gb += 4) ssq[0] += bsum[gb][lane];
      }
    } else if (valid) {
      if (CACHED) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          const int gb = wv + 4 * i;
          if (gb < cbtot) {
            load8(gb, 0, c0[i], c1[i]);
            ssq[0] += sumsq8(c0[i], c1[i]);
          }
        }
      } else {
        for (int gb = wv; gb < cbtot; gb += 4) {
#pragma unroll
          for (int sub = 0; sub < NSUB; ++sub) {
            f32x4 a0, a1;
            load8(gb, sub, a0, a1);
            ssq[sub] += sumsq8(a0, a1);
          }
        }
      }
    }
    if (L.norm_w) {
      if (!WIDE || wv < 4) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) red[wv][sub][lane] = ssq[sub];
      }
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub) {
        const float t = red[0][sub][lane] + red[1][sub][lane] + red[2][sub][lane] + red[3][sub][lane];
        rstd[sub] = 1.0f / sqrtf(t * L.inv_c + TM_EPS);
      }
    }
  }
  if (!valid) return;
  const long oplane = vpn * 8;
  const long oin = ((long)(z * S + y) * S + x) * 8;
  const int img = n / L.per_image;
  auto emit = [&](int gb, int i) {
    float wn[8], sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { wn[j] = 1.f; sc[j] = 0.f; sh[j] = 0.f; }
    if (L.norm_w) {
#pragma unroll
      for (int j = 0; j < 8; ++j) wn[j] = L.norm_w[gb * 8 + j];
    }
    if (L.mod == MOD_IMAGE) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sc[j] = L.mod_scale[(long)img * L.mod_stride + gb * 8 + j];
        sh[j] = L.mod_shift[(long)img * L.mod_stride + gb * 8 + j];
      }
    } else if (L.mod == MOD_VOXEL) {
      const long mo = !L.mod_half ? (long)n * L.mod_stride + (long)gb * oplane + oin
                                  : (long)n * L.mod_stride + (long)gb * (oplane >> 2) +
                                        ((long)(z * (S >> 1) + (y >> 1)) * (S >> 1) + (x >> 1)) * 8;
      if (L.mod_scale_h) {
        if (L.h_f16) {
          typedef _Float16 f16x8_m __attribute__((ext_vector_type(8)));
          const f16x8_m scb = *(const f16x8_m*)(L.mod_scale_h + mo), shb = *(const f16x8_m*)(L.mod_shift_h + mo);
#pragma unroll
          for (int j = 0; j < 8; ++j) { sc[j] = (float)scb[j]; sh[j] = (float)shb[j]; }
        } else {
          typedef __bf16 bf16x8_m __attribute__((ext_vector_type(8)));
          const bf16x8_m scb = *(const bf16x8_m*)(L.mod_scale_h + mo), shb = *(const bf16x8_m*)(L.mod_shift_h + mo);
#pragma unroll
          for (int j = 0; j < 8; ++j) { sc[j] = (float)scb[j]; sh[j] = (float)shb[j]; }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { sc[j] = L.mod_scale[mo + j]; sh[j] = L.mod_shift[mo + j]; }
      }
    }
    float o[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { o[j] = 0.f; r[j] = 0.f; }
    uint32_t keep = 0;
    if (DRAW) keep = drop_keep8(R.key, R.site, (unsigned long long)vidx, gb, R.thr);
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      f32x4 a0, a1;
      if (CACHED) { a0 = c0[i]; a1 = c1[i]; }
      else load8(gb, sub, a0, a1);
      const float xv[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = xv[j];
        r[j] += v;
        if (L.norm_w) v = wn[j] * (v * rstd[sub]);
        if (L.mod != MOD_NONE) v = v * (1.0f + sc[j]) + sh[j];
        // SiLU on the hardware exp2 / rcp (1 ulp each, ~3e-7 relative on the result) in fp32 too: libm expf + an IEEE division
        // are ~30 VALU instructions per element of an otherwise HBM-bound pass (configs[1] fp32: 55.22 -> 54.63 ms same box)
        if (L.act) v = silu_h16(v);
        if (DRAW) v *= (float)((keep >> j) & 1u) * L.drop_scale;
        else if (L.drop_mask) v *= L.drop_mask[(long)n * L.drop_ns + (long)gb * oplane + oin + j] * L.drop_scale;
        o[j] += v;
      }
    }
    if (NSUB == 4) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { o[j] *= 0.25f; r[j] *= 0.25f; }
    }
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    const long eo = (long)gb * oplane + oin;
    if (L.out_h) {
      if (L.h_f16) {
        f16x8 ob;
#pragma unroll
        for (int j = 0; j < 8; ++j) ob[j] = (_Float16)o[j];
        *(f16x8*)(L.out_h + (long)n * L.out_h_nstride + eo) = ob;
      } else {
        bf16x8 ob;
#pragma unroll
        for (int j = 0; j < 8; ++j) ob[j] = (__bf16)o[j];
        *(bf16x8*)(L.out_h + (long)n * L.out_h_nstride + eo) = ob;
      }
    } else if (L.out) {
      float* op = L.out + (long)n * L.out_nstride + eo;
      *(f32x4*)op = f32x4{o[0], o[1], o[2], o[3]};
      *(f32x4*)(op + 4) = f32x4{o[4], o[5], o[6], o[7]};
    }
    if (L.raw) {
      float* rp = L.raw + (long)n * L.raw_nstride + eo;
      *(f32x4*)rp = f32x4{r[0], r[1], r[2], r[3]};
      *(f32x4*)(rp + 4) = f32x4{r[4], r[5], r[6], r[7]};
    }
    if (L.raw_h) {
      if (L.h_f16) {
        f16x8 rb;
#pragma unroll
        for (int j = 0; j < 8; ++j) rb[j] = (_Float16)r[j];
        *(f16x8*)(L.raw_h + (long)n * L.raw_h_nstride + eo) = rb;
      } else {
        bf16x8 rb;
#pragma unroll
        for (int j = 0; j < 8; ++j) rb[j] = (__bf16)r[j];
        *(bf16x8*)(L.raw_h + (long)n * L.raw_h_nstride + eo) = rb;
      }
    }
  };
  if (CACHED) {
#pragma unroll
    for (int i = 0; i < NC; ++i)
      if (wv + WV * i < cbtot) emit(wv + WV * i, i);
  } else {
    for (int gb = wv; gb < cbtot; gb += 4) emit(gb, 0);
  }
  if (L.pad_blocks && wv == 0) {
    for (int pb = 0; pb < L.pad_blocks; ++pb) {
      if (L.out_h) *(uint4*)(L.out_h + (long)n * L.out_h_nstride + (long)(cbtot + pb) * oplane + oin) = uint4{0u, 0u, 0u, 0u};
      if (L.raw_h) *(uint4*)(L.raw_h + (long)n * L.raw_h_nstride + (long)(cbtot + pb) * oplane + oin) = uint4{0u, 0u, 0u, 0u};
    }
  }
}

// The 0 / 1 keep mask the two drawing kernels use, written as an fp32 CB8 tensor [N][Cb][Z][S][S][8] (pad channels c >= C: 0).
// One thread per (voxel, channel block).  Tests and debugging only.
__global__ __launch_bounds__(256) void dropout_mask_kernel(float* mask, long vox, int Cb, int C, long plane_vox,
                                                           unsigned long long key, uint32_t site, uint32_t thr) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= vox * Cb) return;
  const long v = t % vox;                           // consecutive threads: consecutive voxels of one channel block
  const int cb = (int)(t / vox);
  const long n = v / plane_vox, r = v - n * plane_vox;
  const uint32_t keep = drop_keep8(key, site, (unsigned long long)v, cb, thr);
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (8 * cb + j < C && ((keep >> j) & 1u)) ? 1.f : 0.f;
  float* p = mask + ((n * Cb + cb) * plane_vox + r) * 8;
  *(f32x4*)p = f32x4{o[0], o[1], o[2], o[3]};
  *(f32x4*)(p + 4) = f32x4{o[4], o[5], o[6], o[7]};
}
hipError_t launch_dropout_mask(float* mask, int N, int C, int Z, int S, unsigned long long key, uint32_t site, uint32_t thr,
                               hipStream_t s) {
  const int Cb = (C + 7) / 8;
  const long pv = (long)Z * S * S, vox = (long)N * pv;
  if (vox * Cb == 0) return hipSuccess;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((vox * Cb + 255) / 256)), dim3(256), 0, s, mask, vox, Cb, C, pv, key, site, thr);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// prep_h16_kernel: the same operation for the 16-bit activation stream (16-bit CB8 sources -> 16-bit CB8 output, resample
// SAME / UP2), the form every block-input pass of the 16-bit modes takes.  HBM-bound byte work: 2 B read + 2 B written per
// element (+ 4 B for a per-voxel modulation).  Differences from prep_kernel that matter for the memory system:
//   * a lane keeps its voxel's channel blocks PACKED (4 VGPRs per 8 channels), so up to NB blocks per wave stay resident
//     between the sum-of-squares pass and the apply pass for every channel count of the model family (<= 1280 channels):
//     each source byte is read once;
//   * all of a lane's loads are issued before the first use (NB 16-byte loads in flight per lane);
//   * WS = 1: a wave owns 64 voxels and ALL their channel blocks -- no LDS, no barrier, 256 voxels per workgroup (the fine
//     levels, where the old 64-voxel workgroups lived for a few hundred cycles each);
//     WS = 4: the four waves split the channel blocks of 64 voxels and combine their sums of squares through LDS (coarse
//     levels: few voxels, many channels).
// ------------------------------------------------------------------------------------------
typedef unsigned int pu32x4 __attribute__((ext_vector_type(4)));

template <bool F16>
__device__ __forceinline__ void unpack8(const pu32x4& v, float (&f)[8]) {
  if (F16) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const h2 h = __builtin_bit_cast(h2, (unsigned int)v[j]);
      f[2 * j] = (float)h[0]; f[2 * j + 1] = (float)h[1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned int w = v[j];
      f[2 * j] = __uint_as_float(w << 16); f[2 * j + 1] = __uint_as_float(w & 0xffff0000u);
    }
  }
}
template <bool F16>
__device__ __forceinline__ pu32x4 pack8(const float (&f)[8]) {
  pu32x4 r;
  if (F16) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 4; ++j) { h2 h; h[0] = (_Float16)f[2 * j]; h[1] = (_Float16)f[2 * j + 1]; r[j] = __builtin_bit_cast(unsigned int, h); }
  } else {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 4; ++j) { b2 h; h[0] = (__bf16)f[2 * j]; h[1] = (__bf16)f[2 * j + 1]; r[j] = __builtin_bit_cast(unsigned int, h); }
  }
  return r;
}

template <int WS, int NB, bool F16>
__global__ __launch_bounds__(256) void prep_h16_kernel(PrepArgs pa) {
  const PrepLaunch& L = pa.L;
  __shared__ float red[WS == 4 ? 4 : 1][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int S = L.S, Z = L.Z;
  const int vpn = Z * S * S;
  const long vidx = (WS == 4 ? (long)blockIdx.x * 64 : ((long)blockIdx.x * 4 + wv) * 64) + lane;
  const bool valid = vidx < (long)vpn * L.N;
  int n = 0, z = 0, y = 0, x = 0;
  if (valid) {
    n = (int)(vidx / vpn);
    int rem = (int)(vidx - (long)n * vpn);
    z = rem / (S * S); rem -= z * S * S;
    y = rem / S; x = rem - y * S;
  }
  // source plane size and the voxel's coordinates in it: as they are, nearest x2 (UP2), or every second voxel (PICK2);
  // the collage remap (half a patch down / right, into the neighbouring encoder patch) is applied in source coordinates
  const int Ss = L.resample == RS_UP2 ? S / 2 : (L.resample == RS_PICK2 ? 2 * S : S);
  const long splane = (long)Z * Ss * Ss * 8;               // elements per channel block of a source patch
  long soff[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    soff[k] = 0;
    if (k >= L.nsrc) continue;
    int ns = n, ys = y, xs = x;
    if (L.resample == RS_UP2) { ys = y >> 1; xs = x >> 1; }
    if (L.resample == RS_PICK2) { ys = 2 * y; xs = 2 * x; }
    if (L.src[k].collage) {
      const int q1 = L.p1 - 1, q2 = L.p2 - 1;
      const int bi = n / (q1 * q2);
      const int q = n - bi * q1 * q2;
      int i = q / q2, j = q - i * q2;
      ys += Ss / 2; if (ys >= Ss) { ys -= Ss; i += 1; }
      xs += Ss / 2; if (xs >= Ss) { xs -= Ss; j += 1; }
      ns = bi * L.p1 * L.p2 + i * L.p2 + j;
    }
    soff[k] = (long)ns * L.src[k].nstride + ((long)(z * Ss + ys) * Ss + xs) * 8;
  }
  const int cb0 = L.src[0].Cb, cb01 = cb0 + ((L.nsrc > 1) ? L.src[1].Cb : 0);
  const int cbtot = cb01 + ((L.nsrc > 2) ? L.src[2].Cb : 0);
  const int g0 = WS == 4 ? wv : 0;                          // this wave's virtual blocks: g0, g0 + WS, ...
  // Every one of the NB loads is issued UNCONDITIONALLY (a block past the end re-reads the last real block, an invalid lane reads
  // voxel 0's entry: a cache hit, the value is never used): with the loads under `if (gb < cbtot)` the register allocator
  // kept three copies of the block array alive across the branches (234 VGPRs for NB = 16, two waves per SIMD)
  pu32x4 c[NB];
  const int glast = g0 < cbtot ? cbtot - 1 - ((cbtot - 1 - g0) % WS) : 0;      // the wave's last real block (block 0 if it has none)
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int gb = min(g0 + WS * i, glast);
    const int k = (gb >= cb0) + (gb >= cb01);              // wave-uniform
    const int cb = gb - (k == 0 ? 0 : (k == 1 ? cb0 : cb01));
    const uint16_t* sp = (const uint16_t*)(k == 0 ? L.src[0].p : (k == 1 ? L.src[1].p : L.src[2].p));
    const long so = k == 0 ? soff[0] : (k == 1 ? soff[1] : soff[2]);
    c[i] = *(const pu32x4*)(sp + so + (long)cb * splane);
  }
  float rstd = 1.f;
  if (L.norm_w) {
    // Both forms add in ONE order -- four partial sums over the blocks gb = r, r + 4, r + 8, ... (r = 0..3), then
    // p0 + p1 + p2 + p3 -- so that the form (which depends on the size of the call) never changes a result bit: a patch
    // computed inside a large batch equals the same patch computed alone.
    float ps[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        if (g0 + WS * i < cbtot) {
          float f[8];
          unpack8<F16>(c[i], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) ps[WS == 4 ? 0 : (i & 3)] += f[j] * f[j];
        }
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // four blocks' floats live at a time, not all NB x 8 of them
      }
    }
    float ssq;
    if (WS == 4) {
      red[wv][lane] = ps[0];
      __syncthreads();
      ssq = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    } else {
      ssq = ps[0] + ps[1] + ps[2] + ps[3];
    }
    rstd = 1.0f / sqrtf(ssq * L.inv_c + TM_EPS);
  }
  if (!valid) return;
  // the apply pass unpacks the resident blocks again: without this the compiler keeps the sum-of-squares pass's unpacked
  // floats alive instead (8 VGPRs per block on top of the 4 packed ones)
#pragma unroll
  for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(c[i]));
  const long oplane = (long)vpn * 8;
  const long oin = ((long)(z * S + y) * S + x) * 8;
  const int img = n / L.per_image;
  uint16_t* const outp = L.out_h + (long)n * L.out_h_nstride + oin;
  uint16_t* const rawp = L.raw_h ? L.raw_h + (long)n * L.raw_h_nstride + oin : nullptr;
  // per-voxel modulation tensors: the output geometry, or (mod_half) half its in-plane resolution
  const long mplane = L.mod_half ? oplane >> 2 : oplane;
  const long mo = (long)n * L.mod_stride + (L.mod_half ? ((long)(z * (S >> 1) + (y >> 1)) * (S >> 1) + (x >> 1)) * 8 : oin);
  constexpr int CH = 4;                                      // blocks per chunk: their modulation loads are issued together
#pragma unroll
  for (int i0 = 0; i0 < NB; i0 += CH) {
    pu32x4 msc[CH], msh[CH];
    if (L.mod == MOD_VOXEL) {
#pragma unroll
      for (int ii = 0; ii < CH; ++ii) {
        const int gb = min(g0 + WS * (i0 + ii), glast);        // unconditional, as the source loads above
        msc[ii] = *(const pu32x4*)(L.mod_scale_h + mo + (long)gb * mplane);
        msh[ii] = *(const pu32x4*)(L.mod_shift_h + mo + (long)gb * mplane);
      }
    } else {
#pragma unroll
      for (int ii = 0; ii < CH; ++ii) { msc[ii] = pu32x4{0u, 0u, 0u, 0u}; msh[ii] = pu32x4{0u, 0u, 0u, 0u}; }
    }
#pragma unroll
    for (int ii = 0; ii < CH; ++ii) {
      const int i = i0 + ii;
      const int gb = g0 + WS * i;
      if (i < NB && gb < cbtot) {
        float v[8];
        unpack8<F16>(c[i], v);
        if (rawp) *(pu32x4*)(rawp + (long)gb * oplane) = c[i];
        if (L.norm_w) {
          const f32x4 w0 = *(const f32x4*)(L.norm_w + gb * 8), w1 = *(const f32x4*)(L.norm_w + gb * 8 + 4);
          const float wn[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = wn[j] * (v[j] * rstd);
        }
        if (L.mod == MOD_IMAGE) {
          const float* scp = L.mod_scale + (long)img * L.mod_stride + gb * 8;
          const float* shp = L.mod_shift + (long)img * L.mod_stride + gb * 8;
          const f32x4 s0 = *(const f32x4*)scp, s1 = *(const f32x4*)(scp + 4), h0 = *(const f32x4*)shp, h1 = *(const f32x4*)(shp + 4);
          const float sc[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
          const float sh[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = v[j] * (1.0f + sc[j]) + sh[j];
        } else if (L.mod == MOD_VOXEL) {
          float sc[8], sh[8];
          unpack8<F16>(msc[ii], sc);
          unpack8<F16>(msh[ii], sh);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = v[j] * (1.0f + sc[j]) + sh[j];
        }
        if (L.act) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = silu_h16(v[j]);
        }
        *(pu32x4*)(outp + (long)gb * oplane) = pack8<F16>(v);
      }
    }
    __builtin_amdgcn_sched_barrier(0);       // one chunk at a time: without it the bf16 build unpacks every block up front (234 VGPRs)
  }
  if (L.pad_blocks && (WS == 1 || wv == 0)) {
    for (int pb = 0; pb < L.pad_blocks; ++pb) {
      *(pu32x4*)(outp + (long)(cbtot + pb) * oplane) = pu32x4{0u, 0u, 0u, 0u};
      if (rawp) *(pu32x4*)(rawp + (long)(cbtot + pb) * oplane) = pu32x4{0u, 0u, 0u, 0u};
    }
  }
}

// Downsample form (ResBlock(down=True), model/MBAblocks.py:254-258, blocks.py:389-403: norm -> SiLU at full resolution, then
// the 2 x 2 average of h and of x): an output voxel gathers its four source voxels, each normalised with its OWN statistics;
// out = mean of the four activated values, raw = mean of the four inputs (the block's residual).  Four waves split the channel
// blocks of 64 output voxels (C <= 256: 8 blocks x 4 sources x 16 bytes resident per lane).
template <int NB, bool F16>
__global__ __launch_bounds__(256) void prep_down_h16_kernel(PrepArgs pa) {
  const PrepLaunch& L = pa.L;
  __shared__ float red[4][4][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int S = L.S, Z = L.Z, Ss = 2 * S;
  const int vpn = Z * S * S;
  const long vidx = (long)blockIdx.x * 64 + lane;
  const bool valid = vidx < (long)vpn * L.N;
  int n = 0, z = 0, y = 0, x = 0;
  if (valid) {
    n = (int)(vidx / vpn);
    int rem = (int)(vidx - (long)n * vpn);
    z = rem / (S * S); rem -= z * S * S;
    y = rem / S; x = rem - y * S;
  }
  const long splane = (long)Z * Ss * Ss * 8;
  const uint16_t* sp = (const uint16_t*)L.src[0].p + (long)n * L.src[0].nstride;
  long soff[4];
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) soff[sub] = ((long)(z * Ss + 2 * y + (sub >> 1)) * Ss + 2 * x + (sub & 1)) * 8;
  const int cbtot = L.src[0].Cb;
  pu32x4 c[NB][4];
  float ssq[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int gb = wv + 4 * i;
      if (gb < cbtot) {
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) c[i][sub] = *(const pu32x4*)(sp + soff[sub] + (long)gb * splane);
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if (wv + 4 * i < cbtot) {
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
          float f[8];
          unpack8<F16>(c[i][sub], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) ssq[sub] += f[j] * f[j];
        }
      }
    }
  }
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) red[wv][sub][lane] = ssq[sub];
  __syncthreads();
  if (!valid) return;
  float rstd[4];
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) {
    const float t = red[0][sub][lane] + red[1][sub][lane] + red[2][sub][lane] + red[3][sub][lane];
    rstd[sub] = L.norm_w ? 1.0f / sqrtf(t * L.inv_c + TM_EPS) : 1.0f;
  }
  const long oplane = (long)vpn * 8;
  const long oin = ((long)(z * S + y) * S + x) * 8;
  uint16_t* const outp = L.out_h + (long)n * L.out_h_nstride + oin;
  uint16_t* const rawp = L.raw_h ? L.raw_h + (long)n * L.raw_h_nstride + oin : nullptr;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int gb = wv + 4 * i;
    if (gb < cbtot) {
      float wn[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) wn[j] = 1.f;
      if (L.norm_w) {
        const f32x4 w0 = *(const f32x4*)(L.norm_w + gb * 8), w1 = *(const f32x4*)(L.norm_w + gb * 8 + 4);
        wn[0] = w0[0]; wn[1] = w0[1]; wn[2] = w0[2]; wn[3] = w0[3]; wn[4] = w1[0]; wn[5] = w1[1]; wn[6] = w1[2]; wn[7] = w1[3];
      }
      float o[8], r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { o[j] = 0.f; r[j] = 0.f; }
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        float v[8];
        unpack8<F16>(c[i][sub], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          r[j] += v[j];
          float t = L.norm_w ? wn[j] * (v[j] * rstd[sub]) : v[j];
          if (L.act) t = silu_h16(t);
          o[j] += t;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) { o[j] *= 0.25f; r[j] *= 0.25f; }
      *(pu32x4*)(outp + (long)gb * oplane) = pack8<F16>(o);
      if (rawp) *(pu32x4*)(rawp + (long)gb * oplane) = pack8<F16>(r);
    }
  }
  if (L.pad_blocks && wv == 0) {
    for (int pb = 0; pb < L.pad_blocks; ++pb) {
      *(pu32x4*)(outp + (long)(cbtot + pb) * oplane) = pu32x4{0u, 0u, 0u, 0u};
      if (rawp) *(pu32x4*)(rawp + (long)(cbtot + pb) * oplane) = pu32x4{0u, 0u, 0u, 0u};
    }
  }
}

// variant: 0 = automatic, 1 = prep_kernel (the generic form), 2 = prep_h16_kernel with one wave per 64 voxels, 3 = prep_h16_kernel
// with the four waves of a workgroup splitting the channel blocks.  fp32 calls (tm_op_prep_f32): 1 = the four-wave forms of
// prep_kernel, 2 = its wide resident form
static int g_prep_variant = 0;
void set_prep_variant(int v) { g_prep_variant = v; }

template <bool F16>
static bool launch_prep_h16(const PrepLaunch& L, hipStream_t s, int variant) {
  PrepArgs pa; pa.L = L;
  const long vox = (long)L.N * L.Z * L.S * L.S;
  int cbtot = 0;
  for (int k = 0; k < L.nsrc; ++k) cbtot += L.src[k].Cb;
  // measured on the test_brn tile shapes (tools/bench_prep.py, profiles/r02_bench_prep.txt): the one-wave form wins for up to 12
  // channel blocks on the fine levels, the split form everywhere else
  bool one = cbtot <= 12 && vox / 256 >= 2048;
  if (variant == 2) { if (cbtot > 32) return false; one = true; }
  if (variant == 3) one = false;
  if (one) {
    const unsigned grid = (unsigned)((vox + 255) / 256);
    if (cbtot <= 8) hipLaunchKernelGGL((prep_h16_kernel<1, 8, F16>), dim3(grid), dim3(256), 0, s, pa);
    else if (cbtot <= 16) hipLaunchKernelGGL((prep_h16_kernel<1, 16, F16>), dim3(grid), dim3(256), 0, s, pa);
    else hipLaunchKernelGGL((prep_h16_kernel<1, 32, F16>), dim3(grid), dim3(256), 0, s, pa);
  } else {
    if (cbtot > 160) return false;
    const unsigned grid = (unsigned)((vox + 63) / 64);
    if (cbtot <= 32) hipLaunchKernelGGL((prep_h16_kernel<4, 8, F16>), dim3(grid), dim3(256), 0, s, pa);
    else if (cbtot <= 64) hipLaunchKernelGGL((prep_h16_kernel<4, 16, F16>), dim3(grid), dim3(256), 0, s, pa);
    else hipLaunchKernelGGL((prep_h16_kernel<4, 40, F16>), dim3(grid), dim3(256), 0, s, pa);
  }
  return true;
}

hipError_t launch_prep_drop(const PrepLaunch& L, const DropRng& r, hipStream_t s) {
  if (L.nsrc != 1 || L.src_h || L.src[0].collage || L.resample != RS_SAME || !L.out || L.out_h || L.raw || L.raw_h || L.drop_mask ||
      L.mod == MOD_VOXEL || L.pad_blocks)
    return hipErrorInvalidValue;
  PrepDropArgs pa; pa.L = L; pa.r = r;
  const unsigned grid = (unsigned)(((long)L.N * L.Z * L.S * L.S + 63) / 64);
  if (L.src[0].Cb <= 32) hipLaunchKernelGGL((prep_kernel<1, true, true, PrepDropArgs>), dim3(grid), dim3(256), 0, s, pa);
  else hipLaunchKernelGGL((prep_kernel<1, false, true, PrepDropArgs>), dim3(grid), dim3(256), 0, s, pa);
  return hipGetLastError();
}

// The wide resident form of prep_kernel takes the call: decided by the properties of the call only, never by N or the launch size
bool prep_wide_applies(const PrepLaunch& L) {
  int cbtot = 0;
  for (int k = 0; k < L.nsrc; ++k) cbtot += L.src[k].Cb;
  return !L.src_h && L.out && !L.out_h && !L.raw_h && !L.drop_mask && L.resample != RS_DOWN2 && cbtot > 32 && cbtot <= PREP_WIDE_MAX_CB;
}

hipError_t launch_prep(const PrepLaunch& L, hipStream_t s) {
  static const int env_form = getenv("TM_PREP_FORM") ? atoi(getenv("TM_PREP_FORM")) : 0;       // A/B timing only
  const int form = g_prep_variant ? g_prep_variant : env_form;
  if (form != 1 && L.src_h && L.out_h && !L.out && !L.raw && !L.drop_mask && L.resample == RS_DOWN2 && L.nsrc == 1 &&
      !L.src[0].collage && L.mod == MOD_NONE && L.src[0].Cb <= 32) {
    PrepArgs pa; pa.L = L;
    const unsigned grid = (unsigned)(((long)L.N * L.Z * L.S * L.S + 63) / 64);
    if (L.h_f16) hipLaunchKernelGGL((prep_down_h16_kernel<8, true>), dim3(grid), dim3(256), 0, s, pa);
    else hipLaunchKernelGGL((prep_down_h16_kernel<8, false>), dim3(grid), dim3(256), 0, s, pa);
    return hipGetLastError();
  }
  if (form != 1 && L.src_h && L.out_h && !L.out && !L.raw && !L.drop_mask && L.resample != RS_DOWN2 &&
      (L.mod != MOD_VOXEL || L.mod_scale_h)) {
    if (L.h_f16 ? launch_prep_h16<true>(L, s, form) : launch_prep_h16<false>(L, s, form)) return hipGetLastError();
  }

  PrepArgs pa; pa.L = L;
  const long vox = (long)L.N * L.Z * L.S * L.S;
  const unsigned grid = (unsigned)((vox + 63) / 64);
  int cbtot = 0;
  for (int k = 0; k < L.nsrc; ++k) cbtot += L.src[k].Cb;
  if (form != 1 && prep_wide_applies(L)) {
    // 16 waves x <= 3 / 6 / 10 blocks.  Eight waves of twice the blocks were timed beside it (profiles/fp32_glue.txt section 4):
    // equal at 48 and 93 blocks, 31.5 against 26.3 us at 157 blocks
#define TM_PREP_WIDE(WV, NCW) hipLaunchKernelGGL((prep_kernel<1, true, false, PrepArgs, WV, NCW>), dim3(grid), dim3(WV * 64), 0, s, pa)
    if (cbtot <= 48) TM_PREP_WIDE(16, 3); else if (cbtot <= 96) TM_PREP_WIDE(16, 6); else TM_PREP_WIDE(16, 10);
#undef TM_PREP_WIDE
    return hipGetLastError();
  }
  if (L.resample == RS_DOWN2) hipLaunchKernelGGL((prep_kernel<4, false>), dim3(grid), dim3(256), 0, s, pa);
  else if (cbtot <= 32) hipLaunchKernelGGL((prep_kernel<1, true>), dim3(grid), dim3(256), 0, s, pa);
  else hipLaunchKernelGGL((prep_kernel<1, false>), dim3(grid), dim3(256), 0, s, pa);
  return hipGetLastError();
}

// ==========================================================================================
// Generic direct Conv3d on VALU (fp32 VALU rate == fp32 MFMA rate on gfx950, and these
// layers are < 1 % of the FLOPs): stem Conv3d(2->64,(1,3,3)) (model/unet_ours.py:110-114),
// head Conv3d(64->2,(1,3,3)) (:274-275), RNA pyramid SiLU->Conv3d(1,3,3)->Upsample
// (:290-295) and down_z Conv3d(G->G,(ker,3,3),pad (0,1,1)) (model/MBAblocks.py:472-474).
// lane = output voxel, blockIdx.y = block of 8 couts: weight reads are wave-uniform.
// weights are pre-transposed to [tap][Cin][Cout_pad8].
// ==========================================================================================
struct DirectArgs { DirectLaunch L; int Cop; };

__global__ __launch_bounds__(256) void conv_direct_kernel(DirectArgs da) {
  const DirectLaunch& L = da.L;
  const int S = L.S;
  const long vpn = (long)L.Zout * S * S;
  const long vidx = (long)blockIdx.x * 256 + threadIdx.x;
  if (vidx >= vpn * L.N) return;
  const int n = (int)(vidx / vpn);
  int rem = (int)(vidx - (long)n * vpn);
  const int zo = rem / (S * S); rem -= zo * S * S;
  const int y = rem / S, x = rem - y * S;
  const int cob = blockIdx.y;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const float* xb = L.x + (long)n * L.ax.sN;
  for (int kz = 0; kz < L.kz; ++kz) {
    const int zi = zo + kz - L.pz;
    if (zi < 0 || zi >= L.Zin) continue;
    for (int ky = 0; ky < L.ky; ++ky) {
      const int yi = y + ky - L.py;
      for (int kx = 0; kx < L.kx; ++kx) {
        const int xi = x + kx - L.px;
        const bool ok = yi >= 0 && yi < S && xi >= 0 && xi < S;
        const long base = zi * L.ax.sZ + (long)yi * L.ax.sY + (long)xi * L.ax.sX;
        const int tap = (kz * L.ky + ky) * L.kx + kx;
        const float* wt = L.w + ((long)tap * L.Cin) * da.Cop + cob * 8;
        for (int ci = 0; ci < L.Cin; ++ci) {
          float xv = 0.f;
          if (ok) xv = xb[base + (long)(ci >> 3) * L.ax.sCb + (long)(ci & 7) * L.ax.sC8];
          if (L.silu_in) xv = silu_f(xv);
          const float* wp = wt + (long)ci * da.Cop;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf(wp[j], xv, acc[j]);
        }
      }
    }
  }
  float* yb = L.y + (long)n * L.ay.sN + (long)cob * L.ay.sCb;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int co = cob * 8 + j;
    if (co >= L.Cout) break;
    const float v = acc[j] + L.bias[co];
    if (L.up2_out) {
      const long o = zo * L.ay.sZ + (long)(2 * y) * L.ay.sY + (long)(2 * x) * L.ay.sX + (long)j * L.ay.sC8;
      yb[o] = v; yb[o + L.ay.sX] = v; yb[o + L.ay.sY] = v; yb[o + L.ay.sY + L.ay.sX] = v;
    } else {
      yb[zo * L.ay.sZ + (long)y * L.ay.sY + (long)x * L.ay.sX + (long)j * L.ay.sC8] = v;
    }
  }
}

Acc5 acc_ncdhw(int C, int Z, int H, int W) {
  Acc5 a;
  a.sX = 1; a.sY = W; a.sZ = (long)H * W; a.sC8 = (long)Z * H * W; a.sCb = 8 * a.sC8;
  a.sN = (long)C * Z * H * W;
  return a;
}
Acc5 acc_cb8(const TV& t) {
  Acc5 a;
  a.sC8 = 1; a.sX = 8; a.sY = (long)t.W * 8; a.sZ = (long)t.H * t.W * 8; a.sCb = t.plane();
  a.sN = t.nstride;
  return a;
}

hipError_t launch_conv_direct(const DirectLaunch& L, hipStream_t s) {
  DirectArgs da; da.L = L; da.Cop = (L.Cout + 7) / 8 * 8;
  const long vox = (long)L.N * L.Zout * L.S * L.S;
  dim3 grid((unsigned)((vox + 255) / 256), (unsigned)(da.Cop / 8));
  hipLaunchKernelGGL(conv_direct_kernel, grid, dim3(256), 0, s, da);
  return hipGetLastError();
}

// ==========================================================================================
// Stem Conv3d(n_stain -> 64k, (1,3,3)) straight from the NCHW '(s z) h w' state into CB8
// (model/unet_ours.py:110-114,377) and head Conv3d(64 -> n_stain, (1,3,3)) from CB8 straight
// into the NCHW eps tensor (:274-275,424).  lane = voxel; weights are wave-uniform (scalar loads).
// ==========================================================================================
struct StemArgs {
  const float* x; float* y; const float* w; const float* bias;   // w: [tap 9][ci][Cop]
  int N, Cin, Cout, Cop, Z, S;
  long y_nstride;
  uint16_t* y_h; long yh_nstride; int h_f16;                     // 16-bit CB8 output instead of y (bf16, or fp16 with h_f16)
};
__global__ __launch_bounds__(256) void stem_kernel(StemArgs a) {
  const int S = a.S;
  const long vpn = (long)a.Z * S * S;
  const long vidx = (long)blockIdx.x * 256 + threadIdx.x;
  if (vidx >= vpn * a.N) return;
  const int n = (int)(vidx / vpn);
  int rem = (int)(vidx - (long)n * vpn);
  const int z = rem / (S * S); rem -= z * S * S;
  const int y = rem / S, x = rem - y * S;
  const int cob0 = blockIdx.y * 4;                 // 4 cout blocks (32 couts) per thread
  // accumulators as pairs: one v_pk_fma_f32 per two couts (the weights are wave-uniform SGPR pairs); each accumulator still sees
  // the same sequence of FMAs, so the result bits do not change
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  f32x2_t acc2[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc2[j] = f32x2_t{a.bias[cob0 * 8 + 2 * j], a.bias[cob0 * 8 + 2 * j + 1]};
  for (int ci = 0; ci < a.Cin; ++ci) {
    const float* xp = a.x + (((long)n * a.Cin + ci) * a.Z + z) * S * S;
    // one tap's 32 wave-uniform weights (SGPRs) at a time: with the nine taps unrolled the 288 weights of a channel did not
    // fit the scalar register file and were spilled to VGPR lanes (v_writelane / v_readlane: 3 x the FMA count)
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll 1
      for (int kx = 0; kx < 3; ++kx) {
        const int yi = y + ky - 1, xi = x + kx - 1;
        const float xv = (yi >= 0 && yi < S && xi >= 0 && xi < S) ? xp[yi * S + xi] : 0.f;
        const float* wp = a.w + ((long)(ky * 3 + kx) * a.Cin + ci) * a.Cop + cob0 * 8;
        const f32x2_t xv2 = {xv, xv};
#pragma unroll
        for (int j = 0; j < 16; ++j) acc2[j] = __builtin_elementwise_fma(f32x2_t{wp[2 * j], wp[2 * j + 1]}, xv2, acc2[j]);
      }
    }
  }
  float acc[32];
#pragma unroll
  for (int j = 0; j < 16; ++j) { acc[2 * j] = acc2[j][0]; acc[2 * j + 1] = acc2[j][1]; }
  if (a.y_h) {
    uint16_t* hp = a.y_h + (long)n * a.yh_nstride + ((long)(z * S + y) * S + x) * 8;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      uint16_t* p = hp + (long)(cob0 + b) * vpn * 8;
      if (a.h_f16) {
        typedef _Float16 f16x8_o __attribute__((ext_vector_type(8)));
        f16x8_o o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (_Float16)acc[b * 8 + j];
        *(f16x8_o*)p = o;
      } else {
        typedef __bf16 bf16x8_o __attribute__((ext_vector_type(8)));
        bf16x8_o o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)acc[b * 8 + j];
        *(bf16x8_o*)p = o;
      }
    }
    return;
  }
  float* yp = a.y + (long)n * a.y_nstride + ((long)(z * S + y) * S + x) * 8;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    float* p = yp + (long)(cob0 + b) * vpn * 8;
    *(f32x4*)p = f32x4{acc[b * 8 + 0], acc[b * 8 + 1], acc[b * 8 + 2], acc[b * 8 + 3]};
    *(f32x4*)(p + 4) = f32x4{acc[b * 8 + 4], acc[b * 8 + 5], acc[b * 8 + 6], acc[b * 8 + 7]};
  }
}
hipError_t launch_stem(const float* x, TV y, const float* w, const float* bias, int Cin, hipStream_t s, uint16_t* y_h,
                       long yh_nstride, int h_f16) {
  if (y.C % 32) return hipErrorInvalidValue;
  StemArgs a{x, y.p, w, bias, y.N, Cin, y.C, y.Cb * 8, y.Z, y.H, y.nstride, y_h, yh_nstride, h_f16};
  const long vox = (long)y.N * y.Z * y.H * y.W;
  hipLaunchKernelGGL(stem_kernel, dim3((unsigned)((vox + 255) / 256), (unsigned)(y.C / 32)), dim3(256), 0, s, a);
  return hipGetLastError();
}

struct HeadArgs {
  const float* x; long x_nstride; int Cb;
  float* y; const float* w; const float* bias;                    // w: [tap 9][ci][8]
  int N, Cout, Z, S;
};
// H16: 0 = fp32 CB8 input, 1 = bf16, 2 = fp16 (the 16-bit modes hand the normalised, activated tensor over in 16 bits like
// every other conv input: half the bytes of the 9-tap gather)
// CO = couts computed (4: the two-stain models -- half the FMAs of the padded 8; 8: anything up to 8)
template <int H16, int CO>
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a) {
  const int S = a.S;
  const long vpn = (long)a.Z * S * S;
  const long vidx = (long)blockIdx.x * 256 + threadIdx.x;
  if (vidx >= vpn * a.N) return;
  const int n = (int)(vidx / vpn);
  int rem = (int)(vidx - (long)n * vpn);
  const int z = rem / (S * S); rem -= z * S * S;
  const int y = rem / S, x = rem - y * S;
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  f32x2_t acc2[CO / 2];                                            // pairs of couts: v_pk_fma_f32, same FMA sequence per cout
#pragma unroll
  for (int j = 0; j < CO / 2; ++j) acc2[j] = f32x2_t{0.f, 0.f};
  const float* xb = a.x + (long)n * a.x_nstride;                   // H16: the same offsets count 16-bit elements
  const uint16_t* xbh = (const uint16_t*)a.x + (long)n * a.x_nstride;
  // channel block outermost: the 9 taps of one block touch 3 rows of one plane back to back (L1 hits); with the
  // taps outermost every tap strides through all Cb planes and the rows are evicted before the next tap returns
  // to them (measured: 8.7x the input bytes fetched from HBM)
  for (int cb = 0; cb < a.Cb; ++cb) {
    const long co = (long)cb * vpn * 8;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yi = y + ky - 1, xi = x + kx - 1;
        if (yi < 0 || yi >= S || xi < 0 || xi >= S) continue;
        const long eo = co + ((long)(z * S + yi) * S + xi) * 8;
        float xv[8];
        if (H16 == 0) {
          const f32x4 a0 = *(const f32x4*)(xb + eo), a1 = *(const f32x4*)(xb + eo + 4);
          xv[0] = a0[0]; xv[1] = a0[1]; xv[2] = a0[2]; xv[3] = a0[3]; xv[4] = a1[0]; xv[5] = a1[1]; xv[6] = a1[2]; xv[7] = a1[3];
        } else if (H16 == 1) {
          typedef __bf16 bf16x8_i __attribute__((ext_vector_type(8)));
          const bf16x8_i v = *(const bf16x8_i*)(xbh + eo);
#pragma unroll
          for (int c = 0; c < 8; ++c) xv[c] = (float)v[c];
        } else {
          typedef _Float16 f16x8_i __attribute__((ext_vector_type(8)));
          const f16x8_i v = *(const f16x8_i*)(xbh + eo);
#pragma unroll
          for (int c = 0; c < 8; ++c) xv[c] = (float)v[c];
        }
        const float* wp = a.w + ((long)(ky * 3 + kx) * a.Cb + cb) * 64;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const f32x2_t xv2 = {xv[c], xv[c]};
#pragma unroll
          for (int j = 0; j < CO / 2; ++j)
            acc2[j] = __builtin_elementwise_fma(f32x2_t{wp[c * 8 + 2 * j], wp[c * 8 + 2 * j + 1]}, xv2, acc2[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CO; ++j)
    if (j < a.Cout) a.y[(((long)n * a.Cout + j) * a.Z + z) * S * S + (long)y * S + x] = acc2[j / 2][j % 2] + a.bias[j];
}
hipError_t launch_head(TV x, float* y, const float* w, const float* bias, int Cout, hipStream_t s, int h16) {
  if (Cout > 8 || h16 < 0 || h16 > 2) return hipErrorInvalidValue;
  HeadArgs a{x.p, x.nstride, x.Cb, y, w, bias, x.N, Cout, x.Z, x.H};
  const long vox = (long)x.N * x.Z * x.H * x.W;
  const dim3 grid((unsigned)((vox + 255) / 256));
  if (Cout <= 4) {
    if (h16 == 0) hipLaunchKernelGGL((head_kernel<0, 4>), grid, dim3(256), 0, s, a);
    else if (h16 == 1) hipLaunchKernelGGL((head_kernel<1, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((head_kernel<2, 4>), grid, dim3(256), 0, s, a);
  } else {
    if (h16 == 0) hipLaunchKernelGGL((head_kernel<0, 8>), grid, dim3(256), 0, s, a);
    else if (h16 == 1) hipLaunchKernelGGL((head_kernel<1, 8>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((head_kernel<2, 8>), grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

// ==========================================================================================
// layout converters
// ==========================================================================================
__global__ void to_cb8_kernel(const float* x, float* y, int N, int C, int Cb, long vpn, long y_nstride) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over N*Cb*vpn*8
  const long tot = (long)N * Cb * vpn * 8;
  if (i >= tot) return;
  const int c8 = (int)(i & 7);
  long r = i >> 3;
  const long v = r % vpn; r /= vpn;
  const int cb = (int)(r % Cb);
  const int n = (int)(r / Cb);
  const int c = cb * 8 + c8;
  y[(long)n * y_nstride + ((long)cb * vpn + v) * 8 + c8] = (c < C) ? x[((long)n * C + c) * vpn + v] : 0.f;
}
__global__ void from_cb8_kernel(const float* x, float* y, int N, int C, long vpn, long x_nstride) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // over N*C*vpn
  const long tot = (long)N * C * vpn;
  if (i >= tot) return;
  const long v = i % vpn;
  long r = i / vpn;
  const int c = (int)(r % C);
  const int n = (int)(r / C);
  y[i] = x[(long)n * x_nstride + ((long)(c >> 3) * vpn + v) * 8 + (c & 7)];
}
hipError_t launch_to_cb8(const float* x, TV y, hipStream_t s) {
  const long vpn = (long)y.Z * y.H * y.W;
  const long tot = (long)y.N * y.Cb * vpn * 8;
  hipLaunchKernelGGL(to_cb8_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, x, y.p, y.N, y.C, y.Cb, vpn, y.nstride);
  return hipGetLastError();
}
hipError_t launch_from_cb8(TV x, float* y, hipStream_t s) {
  const long vpn = (long)x.Z * x.H * x.W;
  const long tot = (long)x.N * x.C * vpn;
  hipLaunchKernelGGL(from_cb8_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, x.p, y, x.N, x.C, vpn, x.nstride);
  return hipGetLastError();
}

// ==========================================================================================
// timestep embedding: sinusoid -> Linear -> SiLU -> Linear  (model/nn.py:187-206,
// model/unet_ours.py:442-476), then every ResBlock's emb_layers = SiLU -> Linear(E, 2*Cout)
// (model/MBAblocks.py:168-171) as ONE matrix [sum 2*Cout][E]: the value depends only on t,
// so it is computed once per image instead of once per patch per block.
// ==========================================================================================
__global__ __launch_bounds__(256) void time_embed_kernel(const int64_t* t, int ch, int E, const float* w1,
                                                         const float* b1, const float* w2, const float* b2,
                                                         float* te, float* te_act) {
  extern __shared__ float sm[];       // [ch] sinusoid, [E] hidden
  float* sinu = sm;
  float* hid = sm + ch;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float tv = (float)t[b];
  const int half = ch / 2;
  for (int i = tid; i < ch; i += 256) {
    const int k = (i < half) ? i : i - half;
    const float fr = expf(-logf(10000.0f) * (float)k / (float)half);
    const float arg = tv * fr;
    sinu[i] = (i < half) ? cosf(arg) : sinf(arg);
  }
  __syncthreads();
  for (int o = tid; o < E; o += 256) {
    float acc = b1[o];
    for (int k = 0; k < ch; ++k) acc = fmaf(w1[(long)o * ch + k], sinu[k], acc);
    hid[o] = silu_f(acc);
  }
  __syncthreads();
  for (int o = tid; o < E; o += 256) {
    float acc = b2[o];
    for (int k = 0; k < E; ++k) acc = fmaf(w2[(long)o * E + k], hid[k], acc);
    te[(long)b * E + o] = acc;
    te_act[(long)b * E + o] = silu_f(acc);      // what every emb_layer reads (emb_all_kernel)
  }
}
hipError_t launch_time_embed(const int64_t* t, int b, int ch, int E, const float* w1, const float* b1,
                             const float* w2, const float* b2, float* te, float* te_act, hipStream_t s) {
  hipLaunchKernelGGL(time_embed_kernel, dim3(b), dim3(256), (ch + E) * sizeof(float), s, t, ch, E, w1, b1, w2, b2, te, te_act);
  return hipGetLastError();
}

// one wave per output row e; lanes split E; weight row kept in registers across images.  te_act = SiLU(te), computed once by
// time_embed_kernel (the same silu_f: the same bits as applying it here for every row)
__global__ __launch_bounds__(256) void emb_all_kernel(const float* te_act, int b, int E, const float* wall,
                                                      const float* ball, int tot, float* ss) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= tot) return;
  float w[16];
  const int per = E / 64;            // E <= 1024
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = (j < per) ? wall[(long)e * E + j * 64 + lane] : 0.f;
  const float bias = ball[e];
  for (int i = 0; i < b; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < per) acc = fmaf(w[j], te_act[(long)i * E + j * 64 + lane], acc);
    acc = wave_sum(acc);
    if (lane == 0) ss[(long)i * tot + e] = acc + bias;
  }
}
hipError_t launch_emb_all(const float* te_act, int b, int E, const float* wall, const float* ball, int tot,
                          float* ss, hipStream_t s) {
  if (E % 64 || E > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(emb_all_kernel, dim3((tot + 3) / 4), dim3(256), 0, s, te_act, b, E, wall, ball, tot, ss);
  return hipGetLastError();
}

}  // namespace tmk
