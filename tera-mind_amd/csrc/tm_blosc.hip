// Blosc-1 frames (lz4 codec, byte shuffle) written on the GPU: the chunk encoding zarr 2.14.1 / numcodecs 0.15.0 give the
// state tiles of test_brn.py:222-226 (`zarr.save_array`), so that a step directory can be exported in the encoding the
// reference writes (brain.TileSweep.save_step(compressor="blosc")).  Restated from the published c-blosc 1.x frame layout
// and the LZ4 block format, as the decoder in tm_io.hip is.
//
// Frame: 16-byte header [2][1][flags][typesize][nbytes LE32][blocksize LE32][cbytes LE32], bstarts int32 [nblocks] (offsets
// from the start of the frame), then per block its streams, each an LE32 length and the bytes.  flags = 0x20 (lz4)
// | 0x01 (byte shuffle, typesize > 1) | 0x10 (blocks are not split).  A block of blocksize / typesize >= 128 elements is
// split into `typesize` streams (byte k of every element), a shorter one and the short last block are one stream: the
// whole elements shuffled, the odd bytes behind them.  A stream whose LZ4 form would take >= its plain size is stored
// (length == plain size is how both decoders tell); an LZ4 stream is therefore always shorter.
//
// Kernels
//   blosc_lz4_kernel     one wave per stream.  The (converted, shuffled) stream and a 4096-entry table of the most recent
//                        position per hash of 4 bytes live in LDS.  A round looks at 64 positions: each lane hashes its 4
//                        bytes, reads the table (positions BEFORE the round only) and verifies the candidate; the wave takes
//                        the match of the lowest lane (greedy), extends it forwards 64 bytes per iteration and backwards
//                        over the pending literals, writes the sequence (all lanes copy the literals) and then enters the
//                        positions the round consumed with an integer max.  The table never holds a position at or behind
//                        the round's, so a candidate lies before its lane and offsets are >= 1; a stream has at most 65536
//                        bytes, so offsets are <= 65535 by construction.  The LZ4 end rules (last match starts >= 12 bytes
//                        before the end and ends >= 5 before it) bound the lanes that search and the extension.
//   blosc_layout_kernel  one wave: per frame the scan of the block sizes (bstarts, cbytes), over the frames their offsets.
//   blosc_pack_kernel    one workgroup per block: header and bstarts (block 0), then the block's streams back to back.
// Nothing depends on the CU count or on the order in which waves run: the bytes are a function of the input and the arguments.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/teramind_hip.h"
#include "tm_device.h"
#include "tm_kernels.h"

namespace tmk {

bool blosc_geometry(size_t nbytes, int typesize, int blocksize, BloscGeo* g) {
  if (nbytes < 1 || nbytes > (size_t)INT32_MAX || (typesize != 1 && typesize != 2 && typesize != 4) || blocksize < BLOSC_ENC_MIN_BLOCK ||
      blocksize > BLOSC_ENC_MAX_BLOCK || (blocksize & 3))
    return false;
  long bs = (long)nbytes < blocksize ? (long)nbytes : blocksize;
  if (bs > typesize) bs -= bs % typesize;
  g->nbytes = (int)nbytes; g->typesize = typesize; g->bs = (int)bs;
  g->nfull = (int)(nbytes / bs); g->leftover = (int)(nbytes % bs);
  g->nblocks = g->nfull + (g->leftover ? 1 : 0);
  g->split = bs / typesize >= 128;
  g->nsplits = g->split ? typesize : 1;
  g->nstreams = g->nfull * g->nsplits + (g->leftover ? 1 : 0);
  g->bound = (size_t)16 + 4 * (size_t)g->nblocks + 4 * (size_t)g->nstreams + nbytes;
  return g->bound <= (size_t)INT32_MAX;                  // cbytes is an LE32 that c-blosc reads as int32
}

size_t blosc_scratch_bytes(const BloscGeo& g, int nframes) {
  const size_t slots = ((size_t)nframes * g.nbytes + 3) & ~(size_t)3;
  return slots + 4 * (size_t)nframes * ((size_t)g.nstreams + g.nblocks + 1);
}

// bytes of element `idx` of frame f, low byte first
template <int MODE>
__device__ __forceinline__ uint32_t blosc_elem(const BloscSrc& src, const BloscGeo& g, int f, int idx) {
  if (MODE == BLOSC_SRC_BYTES) {
    const uint8_t* p = src.base + (size_t)idx * g.typesize;
    uint32_t v = p[0];
    if (g.typesize >= 2) v |= (uint32_t)p[1] << 8;
    if (g.typesize == 4) v |= ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return v;
  }
  const int plane = src.TH * src.TW, c = idx / plane, r = idx - c * plane, y = r / src.TW, x = r - y * src.TW;
  const long at = src.origins[f] + (long)c * src.cstride + (long)y * src.pitch + x;
  if (MODE == BLOSC_SRC_F16) return ((const uint16_t*)src.base)[at];
  return __half_as_ushort(__float2half_rn(((const float*)src.base)[at]));     // RNE, as Tensor.half()
}

// byte `sp` of the elements idx .. idx + cnt - 1 (cnt <= 4) of frame f, the first in the low byte
template <int MODE>
__device__ __forceinline__ uint32_t blosc_bytes4(const BloscSrc& src, const BloscGeo& g, int f, int idx, int cnt, int sp) {
  uint32_t w = 0;
  if (MODE != BLOSC_SRC_BYTES && cnt == 4 && !(src.TW & 3) && !(idx & 3)) {     // four neighbours of one row: one address
    const int plane = src.TH * src.TW, c = idx / plane, r = idx - c * plane, y = r / src.TW, x = r - y * src.TW;
    const long at = src.origins[f] + (long)c * src.cstride + (long)y * src.pitch + x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t v = MODE == BLOSC_SRC_F16 ? ((const uint16_t*)src.base)[at + k]
                                               : __half_as_ushort(__float2half_rn(((const float*)src.base)[at + k]));
      w |= ((v >> (8 * sp)) & 255u) << (8 * k);
    }
    return w;
  }
  for (int k = 0; k < cnt; ++k) w |= ((blosc_elem<MODE>(src, g, f, idx + k) >> (8 * sp)) & 255u) << (8 * k);
  return w;
}

__device__ __forceinline__ uint32_t rd32(const uint8_t* s, int p) {
  return (uint32_t)s[p] | ((uint32_t)s[p + 1] << 8) | ((uint32_t)s[p + 2] << 16) | ((uint32_t)s[p + 3] << 24);
}
__device__ __forceinline__ int len_ext_bytes(int v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }   // v: the length the token's nibble stands for
// the extension bytes of v >= 15: (v - 15) / 255 times 255, then the rest; by all lanes.  Returns their number.
__device__ __forceinline__ int put_len_ext(uint8_t* o, int v, int lane) {
  const int cnt = (v - 15) / 255 + 1;
  for (int i = lane; i < cnt; i += 64) o[i] = i < cnt - 1 ? 255 : (uint8_t)((v - 15) % 255);
  return cnt;
}

constexpr int BLOSC_HASH_BITS = 12, BLOSC_TABLE = 1 << BLOSC_HASH_BITS;

template <int MODE>
__global__ __launch_bounds__(64) void blosc_lz4_kernel(BloscSrc src, BloscGeo g, uint8_t* __restrict__ slots, int32_t* __restrict__ lens) {
  extern __shared__ uint32_t blosc_lds[];
  uint32_t* table = blosc_lds;                                     // most recent position + 1 per hash, 0 = none
  uint8_t* s = (uint8_t*)(blosc_lds + BLOSC_TABLE);                // the stream
  const int lane = threadIdx.x, st = blockIdx.x, f = blockIdx.y;
  const bool full = st < g.nfull * g.nsplits;
  const int j = full ? st / g.nsplits : g.nfull, sp = full ? st - j * g.nsplits : 0;
  const int bsize = full ? g.bs : g.leftover, ns = full ? g.nsplits : 1, n = bsize / ns;
  const int ts = g.typesize, e0 = (int)(((long)j * g.bs) / ts);    // first element of the block (bs is a multiple of ts, or the only block)
  uint8_t* out = slots + (size_t)f * g.nbytes + (size_t)j * g.bs + (size_t)sp * n;

  for (int i = lane; i < BLOSC_TABLE; i += 64) table[i] = 0;
  if (ns == ts) {                                                  // byte `sp` of every element (typesize 1: the block itself)
#pragma unroll 2
    for (int e = 4 * lane; e < n; e += 256) {                      // four elements per lane: independent loads, one LDS word
      const int cnt = n - e < 4 ? n - e : 4;
      const uint32_t w = blosc_bytes4<MODE>(src, g, f, e0 + e, cnt, sp);
      if (cnt == 4) *(uint32_t*)(s + e) = w;
      else for (int k = 0; k < cnt; ++k) s[e + k] = (uint8_t)(w >> (8 * k));
    }
  } else {                                                         // one stream: the whole elements shuffled, the odd bytes after them
    const int nel = bsize / ts, rem = bsize - nel * ts;
    for (int e = lane; e < nel; e += 64) {
      const uint32_t v = blosc_elem<MODE>(src, g, f, e0 + e);
      for (int k = 0; k < ts; ++k) s[k * nel + e] = (uint8_t)(v >> (8 * k));
    }
    // odd bytes exist only where the frame is a byte buffer (a tile is whole 16-bit elements)
    for (int r = lane; r < rem; r += 64) s[nel * ts + r] = src.base[(size_t)j * g.bs + (size_t)nel * ts + r];
  }
  __syncthreads();

  const int mfl = n - 12;                                          // the last position a match may start at
  const int mend = n - 5;                                          // a match ends at or before it
  int ip = 0, anchor = 0, op = 0;
  bool stored = false;
  while (ip <= mfl) {
    const int p = ip + lane;
    const bool valid = p <= mfl;
    uint32_t v = 0;
    int h = 0, cand = -1;
    bool ok = false;
    if (valid) {
      v = rd32(s, p);
      h = (int)((v * 2654435761u) >> (32 - BLOSC_HASH_BITS));
      cand = (int)table[h] - 1;                                    // < ip: entered by an earlier round
      ok = cand >= 0 && rd32(s, cand) == v;
    }
    const unsigned long long hit = __ballot(ok);
    int next = ip + 64;
    if (hit) {
      const int m = __ffsll((long long)hit) - 1;
      int mp = ip + m, mc = __shfl(cand, m, 64), ml = 4;
      for (;;) {                                                   // forwards, 64 bytes per iteration
        const int q = mp + ml + lane;
        const bool eq = q < mend && s[q] == s[mc + ml + lane];
        const unsigned long long b = __ballot(eq);
        if (b == ~0ull) { ml += 64; continue; }
        ml += __ffsll((long long)~b) - 1;
        break;
      }
      {                                                            // backwards over the pending literals, at most 64 bytes
        const int k = lane + 1;
        const bool eq = mp - k >= anchor && mc - k >= 0 && s[mp - k] == s[mc - k];
        const unsigned long long b = __ballot(eq);
        const int back = b == ~0ull ? 64 : __ffsll((long long)~b) - 1;
        mp -= back; mc -= back; ml += back;
      }
      const int ll = mp - anchor, off = mp - mc, mcode = ml - 4;
      const int size = 1 + len_ext_bytes(ll) + ll + 2 + len_ext_bytes(mcode);
      if (op + size >= n) { stored = true; break; }                // 5 literals and their token still follow: not shorter than plain
      uint8_t* o = out + op;
      if (lane == 0) o[0] = (uint8_t)(((ll < 15 ? ll : 15) << 4) | (mcode < 15 ? mcode : 15));
      o += 1;
      if (ll >= 15) o += put_len_ext(o, ll, lane);
      for (int i = lane; i < ll; i += 64) o[i] = s[anchor + i];
      o += ll;
      if (lane == 0) { o[0] = (uint8_t)(off & 255); o[1] = (uint8_t)(off >> 8); }
      o += 2;
      if (mcode >= 15) o += put_len_ext(o, mcode, lane);
      op += size;
      next = mp + ml;
      anchor = next;
    }
    if (valid && p < next) atomicMax(&table[h], (uint32_t)(p + 1));  // the positions this round consumed; max: no order dependence
    ip = next;
    __syncthreads();
  }
  if (!stored) {                                                   // the last sequence: literals only
    const int ll = n - anchor, size = 1 + len_ext_bytes(ll) + ll;
    if (op + size >= n) {
      stored = true;
    } else {
      uint8_t* o = out + op;
      if (lane == 0) o[0] = (uint8_t)((ll < 15 ? ll : 15) << 4);
      o += 1;
      if (ll >= 15) o += put_len_ext(o, ll, lane);
      for (int i = lane; i < ll; i += 64) o[i] = s[anchor + i];
      op += size;
    }
  }
  if (stored) {
    const int n4 = ((uintptr_t)out & 3) ? 0 : n & ~3;              // words where the slot allows it
    for (int i = 4 * lane; i < n4; i += 256) *(uint32_t*)(out + i) = *(const uint32_t*)(s + i);
    for (int i = n4 + lane; i < n; i += 64) out[i] = s[i];
  }
  if (lane == 0) lens[(size_t)f * g.nstreams + st] = stored ? n : op;
}

// bst[f][j] = offset of block j in frame f, cb[f] = the frame's bytes; offsets[f] = bytes of the frames before f (if given),
// *total = bytes of all frames (if given).  One wave.
__global__ __launch_bounds__(64) void blosc_layout_kernel(BloscGeo g, int nframes, const int32_t* __restrict__ lens, int32_t* __restrict__ bst,
                                                          int32_t* __restrict__ cb, int64_t* __restrict__ offsets, int64_t* __restrict__ total) {
  const int lane = threadIdx.x;
  int64_t base = 0;
  for (int f = 0; f < nframes; ++f) {
    const int32_t* ln = lens + (size_t)f * g.nstreams;
    int run = 16 + 4 * g.nblocks;
    for (int j0 = 0; j0 < g.nblocks; j0 += 64) {
      const int j = j0 + lane;
      int v = 0;
      if (j < g.nfull)
        for (int k = 0; k < g.nsplits; ++k) v += 4 + ln[j * g.nsplits + k];
      else if (j < g.nblocks)
        v = 4 + ln[g.nfull * g.nsplits];
      int inc = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
      }
      if (j < g.nblocks) bst[(size_t)f * g.nblocks + j] = run + inc - v;
      run += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      cb[f] = run;                                                 // <= g.bound <= INT32_MAX
      if (offsets) offsets[f] = base;
    }
    base += run;
  }
  if (lane == 0) {
    if (offsets) offsets[nframes] = base;
    if (total) *total = base;
  }
}

__device__ __forceinline__ void put_le32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

__global__ __launch_bounds__(256) void blosc_pack_kernel(BloscGeo g, const uint8_t* __restrict__ slots, const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ bst, const int32_t* __restrict__ cb,
                                                         const int64_t* __restrict__ offsets, uint8_t* __restrict__ packed) {
  const int j = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  uint8_t* frame = packed + (offsets ? offsets[f] : 0);
  const int32_t* fb = bst + (size_t)f * g.nblocks;
  if (j == 0) {
    if (tid == 0) {
      frame[0] = 2;                                                // Blosc format version
      frame[1] = 1;                                                // LZ4 format version
      frame[2] = (uint8_t)(0x20 | (g.typesize > 1 ? 0x01 : 0) | (g.split ? 0 : 0x10));
      frame[3] = (uint8_t)g.typesize;
      put_le32(frame + 4, (uint32_t)g.nbytes);
      put_le32(frame + 8, (uint32_t)g.bs);
      put_le32(frame + 12, (uint32_t)cb[f]);
    }
    for (int i = tid; i < g.nblocks; i += 256) put_le32(frame + 16 + 4 * (size_t)i, (uint32_t)fb[i]);
  }
  const bool full = j < g.nfull;
  const int ns = full ? g.nsplits : 1, n = (full ? g.bs : g.leftover) / ns;
  const int32_t* ln = lens + (size_t)f * g.nstreams + (size_t)(full ? j * g.nsplits : g.nfull * g.nsplits);
  const uint8_t* slot = slots + (size_t)f * g.nbytes + (size_t)j * g.bs;
  uint8_t* o = frame + fb[j];
  for (int k = 0; k < ns; ++k) {
    const int len = ln[k];
    if (tid == 0) put_le32(o, (uint32_t)len);
    o += 4;
    for (int i = tid; i < len; i += 256) o[i] = slot[(size_t)k * n + i];
    o += len;
  }
}

hipError_t launch_blosc_frames(const BloscSrc& src, const BloscGeo& g, int nframes, void* scratch, uint8_t* packed, int64_t* offsets,
                               int64_t* total, hipStream_t s) {
  uint8_t* slots = (uint8_t*)scratch;
  int32_t* lens = (int32_t*)(slots + (((size_t)nframes * g.nbytes + 3) & ~(size_t)3));
  int32_t* bst = lens + (size_t)nframes * g.nstreams;
  int32_t* cb = bst + (size_t)nframes * g.nblocks;
  static DevOnce once;
  if (once.need()) {                                               // a 65536-byte stream and the table: 80 KB of the CU's 160 KB
    const int most = BLOSC_TABLE * 4 + BLOSC_ENC_MAX_BLOCK;
    hipError_t e = hipFuncSetAttribute((const void*)blosc_lz4_kernel<BLOSC_SRC_BYTES>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)blosc_lz4_kernel<BLOSC_SRC_F16>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)blosc_lz4_kernel<BLOSC_SRC_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    if (e != hipSuccess) return e;
    once.mark();
  }
  const int nmax = g.bs / g.nsplits > g.leftover ? g.bs / g.nsplits : g.leftover;       // the longest stream
  const size_t lds = BLOSC_TABLE * 4 + (((size_t)nmax + 3) & ~(size_t)3);
  const dim3 grid((unsigned)g.nstreams, (unsigned)nframes);
  if (src.mode == BLOSC_SRC_BYTES) blosc_lz4_kernel<BLOSC_SRC_BYTES><<<grid, dim3(64), lds, s>>>(src, g, slots, lens);
  else if (src.mode == BLOSC_SRC_F16) blosc_lz4_kernel<BLOSC_SRC_F16><<<grid, dim3(64), lds, s>>>(src, g, slots, lens);
  else blosc_lz4_kernel<BLOSC_SRC_F32><<<grid, dim3(64), lds, s>>>(src, g, slots, lens);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  blosc_layout_kernel<<<dim3(1), dim3(64), 0, s>>>(g, nframes, lens, bst, cb, offsets, total);
  blosc_pack_kernel<<<dim3((unsigned)g.nblocks, (unsigned)nframes), dim3(256), 0, s>>>(g, slots, lens, bst, cb, offsets, packed);
  return hipGetLastError();
}

}  // namespace tmk
