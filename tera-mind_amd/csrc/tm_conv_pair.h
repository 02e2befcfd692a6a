// Scaffolding shared by the fp32 k x 3 x 3 MFMA conv kernels of tm_kernels.hip (conv3d_mfma, conv3d_zpair, conv3d_zpair_ups,
// conv3d_xquad): what they have in common around their K loops.  The K loops, ring schedules, barriers, waits and register pins
// stay in the kernels, and so do the halo staging, the two-plane load, the stage head and the plane-sum tail of the two z-pair
// kernels: moved into functions here they changed the compiler's wait counts and the instruction order of the K loop
// (profiles/conv_family_refactor.txt).
#pragma once
#include "tm_conv_frag.h"
#include "tm_device.h"

namespace tmk {

typedef int rsrc_words __attribute__((ext_vector_type(4)));     // a buffer descriptor as four SGPRs of an asm statement

// The tile of a workgroup: cout tile nt, patch group pg, tile row / column (tr, tc) of the S x S plane in tiles of TR x TW;
// PHASE: the output phase (py, px) of an upsampled-input form (the four phases of a tile are neighbours in the grid: they share
// the input halo); PLANE: the output plane zo of a form whose workgroups own one plane (a.Z = output planes)
struct ConvTile { int nt, pg, tr, tc, py, px, zo; };
template <int TW, int TR, bool PHASE, bool PLANE>
__device__ __forceinline__ ConvTile conv_tile_of(const ConvArgs& a) {
  const int tiles_c = a.S / TW, tiles_r = a.S / TR;
  const int tiles = tiles_c * tiles_r;
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  ConvTile t;
  t.nt = bid % a.ntile;
  int mt_ = bid / a.ntile;
  t.py = t.px = t.zo = 0;
  if (PHASE) { t.py = (mt_ >> 1) & 1; t.px = mt_ & 1; mt_ >>= 2; }
  if (PLANE) {
    t.pg = mt_ / (a.Z * tiles);
    mt_ -= t.pg * a.Z * tiles;
    t.zo = mt_ / tiles;
    mt_ -= t.zo * tiles;
  } else {
    t.pg = mt_ / tiles;
    mt_ -= t.pg * tiles;
  }
  t.tr = mt_ / tiles_c;
  t.tc = mt_ - t.tr * tiles_c;
  return t;
}

// The lane's fragment: voxel v of the workgroup's tile (rows of TWV voxels; LDS rows of ROWW positions, PS positions per patch, ROWS
// in the image) -> patch ps of the workgroup, tile row r and column c, and the LDS float offset xb of its window (starting (dy, dx)
// further) in an image of two k-half arrays (tm_conv_frag.h)
struct ConvLane { int xb, ps, r, c; };
template <int TR, int TWV, int PS, int ROWW, int ROWS>
__host__ __device__ __forceinline__ ConvLane conv_lane_of(int v, int h, int dy, int dx) {
  ConvLane l;
  l.ps = v / (TR * TWV);
  const int rem = v - l.ps * (TR * TWV);
  l.r = rem / TWV;
  l.c = rem - l.r * TWV;
  l.xb = conv_frag_off(l.ps * PS + (l.r + dy) * ROWW + l.c + dx, h, ROWS);
  return l;
}

template <int A, int B>
__device__ __forceinline__ void clear_acc(f32x16 (&acc)[A][B]) {
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int j = 0; j < B; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// Buffer descriptor over `bytes` of packed weights at `base`.  RFL: the address words pass through readfirstlane (the compiler then
// keeps them in SGPRs of their own instead of rebuilding them)
template <bool RFL>
__device__ __forceinline__ rsrc_words weight_rsrc(const float* base, int bytes) {
  const unsigned long wbase = (unsigned long)base;
  const int lo = (int)(unsigned)wbase, hi = (int)((wbase >> 32) & 0xffff);
  if (RFL) return rsrc_words{__builtin_amdgcn_readfirstlane(lo), __builtin_amdgcn_readfirstlane(hi), bytes, 0x00020000};
  return rsrc_words{lo, hi, bytes, 0x00020000};
}

// Weights global -> LDS by LDS-DMA (`buffer_load_dwordx4 ... offen lds`), no staging registers: piece k of this wave (wvu, of four)
// of a slot of NPIECES pieces of 256 floats, i.e. piece j = 4 k + wvu of the slot at float `slot` of the LDS weight area (byte
// address lw_lds), read from float `src` of the descriptor; wvo = lane * 16.  M0 = LDS address of the piece, saved, set and restored in the
// statement that uses it.  NOP: wait states between the SALU writes and the load (4 where the source offset may come straight from the SALU: five
// wait states ahead of a VMEM read of it).  hipcc does not count these loads: it neither drains them at a barrier nor waits for
// them in front of the fragment reads -- the kernels retire them with their own vmcnt waits.
template <int NOP, int NPIECES, int NWV = 4>                   // NWV: the waves that share the slot's pieces (piece j = NWV k + wvu)
__device__ __forceinline__ void lds_dma_piece(unsigned lw_lds, int slot, int src, int k, int wvu, int wvo, const rsrc_words& rs) {
  const int j = k * NWV + wvu;
  if ((k + 1) * NWV <= NPIECES || j < NPIECES) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop %5\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lw_lds + (unsigned)(slot + j * 256) * 4u), "v"(wvo), "s"(rs), "s"((src + j * 256) * 4), "i"(NOP)
                 : "memory");
  }
}

}  // namespace tmk
