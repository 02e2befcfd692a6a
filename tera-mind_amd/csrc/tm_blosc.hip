// Blosc-1 frames (lz4 codec, byte shuffle) written on the GPU: the chunk encoding zarr 2.14.1 / numcodecs 0.15.0 give the
// state tiles of test_brn.py:222-226 (`zarr.save_array`), so that a step directory can be exported in the encoding the
// reference writes (brain.TileSweep.save_step(compressor="blosc")).  Restated from the published c-blosc 1.x frame layout
// and the LZ4 block format, as the decoder in tm_io.hip is.  The second half of the file is the way back: the same frames,
// and c-blosc's own, decoded on the GPU into plain bytes or a resident canvas (blosc_lz4_decode_kernel, blosc_unshuffle_kernel).
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
#include "tm_blosc_lz4.h"
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

// ==============================================================================================================
// The way back: the frames of a step directory decoded on the GPU (tm_blosc_decompress_dev / _tiles).
//
// The host walks each frame's header, bstarts and stream lengths (blosc_dec_walk, the rules of blosc_decompress in
// tm_io.hip) into a table of streams; a range outside its frame is refused there, so the kernels take offsets on trust.
//   blosc_lz4_decode_kernel<WIN>  one wave per stream.  A stored stream (length == plain size) is a copy.  Otherwise the
//       wave walks the LZ4 sequences (blosc_lz4_walk of tm_blosc_lz4.h, every check in it): the compressed bytes are read
//       through a 256-byte register window (a dword per lane, v_readlane), so token, extensions and offset are wave-uniform;
//       literals and matches are copied 64 bytes at a time by all lanes.  Decoded bytes live in LDS -- a match never reads
//       global memory the wave wrote: position p at ring[(p + shift) & (WIN - 1)], shift = the low 4 bits of the output
//       address, so that whole 16-byte vectors leave LDS for global memory.  WIN = 32768: the stream (<= 32768 bytes) lives
//       whole in LDS, sized to the longest stream of the launch.  WIN = 65536: a ring; offsets are <= 65535, and a slot is
//       flushed before position p + 65536 takes it.  A match chunk [c, c + 64) reads dst[p - m off] with m the smallest
//       multiple that lands before c: bytes written before this chunk, also when the match overlaps itself (the periodic
//       pattern), and never further back than 65535.  All lanes read before any lane writes (one ds_read, one ds_write).
//   blosc_unshuffle_kernel<SINK>  gathers a block's streams back into elements (unsplit blocks and the bytes behind the last
//       whole element as the host decoder does, frames without shuffle as a copy) into plain bytes or into a box of a
//       canvas (float16 copied, or widened to float32; the chunk clipped to the array).  16 elements per thread: 16-byte
//       loads per stream and 16-byte stores where the addresses allow, else byte by byte.  Frames whose status is not 0 are
//       left out.

static inline uint32_t dec_le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

int blosc_dec_walk(const char* fn, int k, const uint8_t* f, size_t len, BloscDecInfo* info, std::vector<BloscStream>* tab, long long src_base,
                   long long dst_base, int* longest_lz4) {
  BloscDecInfo in = {};
  if (!f || len < 16) return fail(TM_ERR_ARG, "%s: frame %d is shorter than its header (%zu bytes)", fn, k, len);
  const unsigned flags = f[2];
  const long long typesize = f[3] ? f[3] : 1;
  const long long nbytes = dec_le32(f + 4), blocksize = dec_le32(f + 8), cbytes = dec_le32(f + 12);
  in.nbytes = nbytes; in.typesize = (int)typesize; in.blocksize = (int)(blocksize > INT32_MAX ? INT32_MAX : blocksize); in.flags = (int)flags;
  if (info) *info = in;
  if ((unsigned long long)cbytes > len) return fail(TM_ERR_ARG, "%s: frame %d truncated: cbytes %lld of %zu bytes", fn, k, cbytes, len);
  const bool memcpyed = flags & 2;
  // what the GPU decoder takes; the rest is the host decoder's (or nobody's)
  if ((!memcpyed && ((flags & 4) || ((flags >> 5) & 7) != 1)) || (typesize != 1 && typesize != 2 && typesize != 4) || nbytes > (1ll << 30))
    return TM_OK;
  in.gpu = 1;
  if (nbytes == 0) { if (info) *info = in; return TM_OK; }
  const size_t first = tab ? tab->size() : 0;
  auto add = [&](long long src, long long clen, long long plen, long long dst) {
    ++in.nstreams;
    if (plen > in.longest) in.longest = (int)plen;
    if (longest_lz4 && clen != plen && plen > *longest_lz4) *longest_lz4 = (int)plen;
    if (tab) tab->push_back(BloscStream{src_base + src, dst_base + dst, (int)clen, (int)plen, k, 0});
  };
  auto bad = [&](const char* what, long long j) {
    if (tab) tab->resize(first);
    return fail(TM_ERR_ARG, "%s: frame %d, block %lld: %s", fn, k, j, what);
  };
  if (memcpyed) {
    if (cbytes < 16 + nbytes) return bad("memcpyed frame truncated", 0);
    add(16, nbytes, nbytes, 0);
    if (info) *info = in;
    return TM_OK;
  }
  if (blocksize <= 0) return bad("bad block size", 0);
  const long long nblocks = (nbytes + blocksize - 1) / blocksize, leftover = nbytes % blocksize;
  if (16 + 4 * nblocks > cbytes) return bad("block table truncated", 0);
  for (long long j = 0; j < nblocks; ++j) {
    const bool last_short = j == nblocks - 1 && leftover > 0;
    const long long bsize = last_short ? leftover : blocksize;
    const long long nsplits = (!(flags & 16) && bsize / typesize >= 128 && !last_short) ? typesize : 1;
    if (bsize % nsplits) return bad("block size is no multiple of the typesize", j);
    const long long ne = bsize / nsplits;
    long long ip = dec_le32(f + 16 + 4 * j);
    for (long long sp = 0; sp < nsplits; ++sp) {
      if (ip + 4 > cbytes) return bad("bstarts entry / stream header outside the frame", j);
      const long long cb = dec_le32(f + ip);
      ip += 4;
      if (ip + cb > cbytes) return bad("stream length outside the frame", j);
      add(ip, cb, ne, j * blocksize + sp * ne);
      ip += cb;
    }
  }
  if (info) *info = in;
  return TM_OK;
}

template <int WIN>
struct BloscWaveIO {
  static constexpr int MASK = WIN - 1;
  const uint8_t* src;                // the compressed stream [n]
  uint8_t* out;                      // its plain bytes in the scratch
  uint8_t* ring;
  int n, lane, shift;
  int base, flushed;                 // window: bytes [base, base + 256) of src; out[0, flushed) is written
  uint32_t w;

  __device__ __forceinline__ void refill(int p) {
    base = p - (int)((uintptr_t)(src + p) & 3);                    // an aligned dword per lane; >= -3
    const int a = base + 4 * lane;
    w = 0;
    if (a >= 0 && a + 4 <= n) {
      w = *(const uint32_t*)(src + a);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (a + k >= 0 && a + k < n) w |= (uint32_t)src[a + k] << (8 * k);
    }
  }
  __device__ __forceinline__ unsigned byte(int p) {                // 0 <= p < n, p never decreases below base
    if (p - base >= 256) refill(p);
    const int idx = __builtin_amdgcn_readfirstlane(p - base);
    return (__builtin_amdgcn_readlane(w, idx >> 2) >> (8 * (idx & 3))) & 255u;
  }
  // out[flushed, to) <- ring; (flushed + shift) % 16 == 0 or flushed == 0; whole vectors where (position + shift) % 16 == 0
  __device__ __forceinline__ void flush(int to) {
    const int from = flushed;
    int head = from + ((16 - ((from + shift) & 15)) & 15);
    if (head > to) head = to;
    if (from + lane < head) out[from + lane] = ring[(from + lane + shift) & MASK];
    const int nv = (to - head) >> 4;
    for (int v = lane; v < nv; v += 64) {
      const int p = head + 16 * v;
      *(uint4*)(out + p) = *(const uint4*)(ring + ((p + shift) & MASK));
    }
    const int tail = head + 16 * nv;
    if (tail + lane < to) out[tail + lane] = ring[(tail + lane + shift) & MASK];
    flushed = to;
  }
  // before positions [c, c + 64) are written: the slots they take (those of c - WIN ...) have left LDS
  __device__ __forceinline__ void make_room(int c) {
    if (c + 64 - flushed > WIN) flush(c - ((c + shift) & 15));
  }
  __device__ __forceinline__ void literals(int ip, int op, int len) {
    for (int c = 0; c < len; c += 64) {
      make_room(op + c);
      const int k = c + lane;
      if (k < len) ring[(op + k + shift) & MASK] = src[ip + k];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
  }
  __device__ __forceinline__ void match(int op, int off, int len) {
    const int back = off >= 64 ? off : (lane / off + 1) * off;     // the smallest multiple of off that lands before the chunk
    for (int c = 0; c < len; c += 64) {
      make_room(op + c);
      const int k = c + lane;
      if (k < len) {
        const uint8_t v = ring[(op + k - back + shift) & MASK];
        ring[(op + k + shift) & MASK] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
  }
};

// src[0, n) -> out[0, n) by one wave; every read inside [0, n): whole dwords of src are realigned to the output's 16-byte
// vectors where all five lie inside the range, bytes elsewhere
__device__ __forceinline__ void blosc_wave_copy(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, int n, int lane) {
  int head = (int)((16 - ((uintptr_t)out & 15)) & 15);
  if (head > n) head = n;
  const int s = (int)((uintptr_t)(src + head) & 3);                // the same for every vector: they are 16 bytes apart
  int v0 = 0, v1 = (n - head) >> 4;                                // vectors [v0, v1) read src[p - s, p - s + 20)
  if (s) {
    if (head - s < 0) v0 = 1;
    while (v1 > v0 && head + 16 * (v1 - 1) - s + 20 > n) --v1;
  }
  if (v1 <= v0) v0 = v1 = 0;
  const int lo = head + 16 * v0, hi = head + 16 * v1;
  for (int i = lane; i < lo; i += 64) out[i] = src[i];
  for (int v = v0 + lane; v < v1; v += 64) {
    const int p = head + 16 * v;
    const uint32_t* q = (const uint32_t*)(src + p - s);
    uint4 r;
    if (s == 0) {
      r = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
      const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];
      r = make_uint4(__builtin_amdgcn_alignbyte(a1, a0, s), __builtin_amdgcn_alignbyte(a2, a1, s), __builtin_amdgcn_alignbyte(a3, a2, s),
                     __builtin_amdgcn_alignbyte(a4, a3, s));
    }
    *(uint4*)(out + p) = r;
  }
  for (int i = hi + lane; i < n; i += 64) out[i] = src[i];
}

template <int WIN>
__global__ __launch_bounds__(64) void blosc_lz4_decode_kernel(const uint8_t* __restrict__ frames, const BloscStream* __restrict__ tab,
                                                              uint8_t* __restrict__ scratch, int32_t* __restrict__ status) {
  extern __shared__ uint4 blosc_dec_lds[];
  const BloscStream t = tab[blockIdx.x];
  const int lane = threadIdx.x;
  const uint8_t* src = frames + t.src;
  uint8_t* out = scratch + t.dst;
  if (t.clen == t.plen) {                                          // stored
    blosc_wave_copy(src, out, t.plen, lane);
    return;
  }
  BloscWaveIO<WIN> io;
  io.src = src; io.out = out; io.ring = (uint8_t*)blosc_dec_lds; io.n = t.clen; io.lane = lane;
  io.shift = (int)((uintptr_t)out & 15); io.base = 0; io.flushed = 0; io.w = 0;
  if (t.clen > 0) io.refill(0);
  const int code = blosc_lz4_walk(io, t.clen, t.plen);
  if (code != BLOSC_DEC_OK) {
    if (lane == 0) atomicMax(&status[t.frame], code);
    return;
  }
  io.flush(t.plen);
}

// byte q of frame fr, read from the frame's shuffled image in the scratch
__device__ __forceinline__ uint32_t blosc_plain_byte(const BloscDecFrame& fr, const uint8_t* __restrict__ img, int q) {
  if (!fr.shuffled) return img[q];
  const int j = q / fr.blocksize, r = q - j * fr.blocksize;
  const int left = fr.nbytes - j * fr.blocksize, bsize = left < fr.blocksize ? left : fr.blocksize;
  const int nel = bsize / fr.typesize;
  if (r >= nel * fr.typesize) return img[q];                       // the bytes behind the last whole element
  const int i = r / fr.typesize, k = r - i * fr.typesize;
  return img[(size_t)j * fr.blocksize + (size_t)k * nel + i];
}

__device__ __forceinline__ uint32_t blosc_weave(uint32_t lo, uint32_t hi, int half) {  // bytes lo[2 half], hi[2 half], lo[2 half + 1], hi[2 half + 1]
  return half ? __builtin_amdgcn_perm(hi, lo, 0x07030602u) : __builtin_amdgcn_perm(hi, lo, 0x05010400u);
}

template <int SINK>
__global__ __launch_bounds__(256) void blosc_unshuffle_kernel(const BloscDecFrame* __restrict__ frs, const uint8_t* __restrict__ scratch,
                                                              BloscSink sink, const int32_t* __restrict__ status) {
  const BloscDecFrame fr = frs[blockIdx.y];
  if (status[blockIdx.y] != 0) return;
  const uint8_t* img = scratch + fr.scratch;
  const int ts = SINK == BLOSC_SINK_BYTES ? (fr.shuffled ? fr.typesize : 1) : 2;      // a copy goes byte-wise
  const int nel = (fr.nbytes + ts - 1) / ts;                       // the last one may be cut (plain sink only)
  const int e0 = 16 * (int)(blockIdx.x * 256 + threadIdx.x);
  if (e0 >= nel) return;
  const int cnt = nel - e0 < 16 ? nel - e0 : 16;
  if (SINK == BLOSC_SINK_BYTES) {
    uint8_t* d = (uint8_t*)sink.base + fr.dst;
    const int q0 = e0 * ts;
    if (cnt == 16 && q0 + 16 * ts <= fr.nbytes) {
      if (ts == 1 && !(((uintptr_t)(img + q0) | (uintptr_t)(d + q0)) & 15)) {
        *(uint4*)(d + q0) = *(const uint4*)(img + q0);
        return;
      }
      if (ts == 2) {
        const int j = q0 / fr.blocksize, r = q0 - j * fr.blocksize;
        const int left = fr.nbytes - j * fr.blocksize, bsize = left < fr.blocksize ? left : fr.blocksize, ne = bsize / 2;
        const uint8_t* lo = img + (size_t)j * fr.blocksize + (r >> 1);
        if (!(r & 1) && r + 32 <= 2 * ne && !(((uintptr_t)lo | (uintptr_t)(lo + ne) | (uintptr_t)(d + q0)) & 15)) {
          const uint4 a = *(const uint4*)lo, b = *(const uint4*)(lo + ne);
          *(uint4*)(d + q0) = make_uint4(blosc_weave(a.x, b.x, 0), blosc_weave(a.x, b.x, 1), blosc_weave(a.y, b.y, 0), blosc_weave(a.y, b.y, 1));
          *(uint4*)(d + q0 + 16) = make_uint4(blosc_weave(a.z, b.z, 0), blosc_weave(a.z, b.z, 1), blosc_weave(a.w, b.w, 0), blosc_weave(a.w, b.w, 1));
          return;
        }
      }
    }
    const int q1 = q0 + cnt * ts < fr.nbytes ? q0 + cnt * ts : fr.nbytes;
    for (int q = q0; q < q1; ++q) d[q] = (uint8_t)blosc_plain_byte(fr, img, q);
    return;
  }
  // canvas sink: element e = (c * H + y) * W + x of the chunk, kept where it lies inside the clipped box
  const int H = fr.chunk[1], W = fr.chunk[2];
  const int row = e0 / W, x0 = e0 - row * W, c0 = row / H, y0 = row - c0 * H;
  const bool one_row = cnt == 16 && x0 + 16 <= W;
  if (one_row && (c0 >= fr.clip[0] || y0 >= fr.clip[1] || x0 >= fr.clip[2])) return;
  if (one_row && x0 + 16 <= fr.clip[2]) {
    const int q0 = 2 * e0, j = q0 / fr.blocksize, r = q0 - j * fr.blocksize;
    const int left = fr.nbytes - j * fr.blocksize, bsize = left < fr.blocksize ? left : fr.blocksize, ne = bsize / 2;
    const uint8_t* lo = img + (size_t)j * fr.blocksize + (r >> 1);
    const long at = fr.dst + (long)c0 * sink.cstride + (long)y0 * sink.pitch + x0;
    const bool src_ok = fr.shuffled ? (!(r & 1) && r + 32 <= 2 * ne && !(((uintptr_t)lo | (uintptr_t)(lo + ne)) & 15)) : !((uintptr_t)(img + q0) & 15);
    const bool dst_ok = SINK == BLOSC_SINK_F16 ? !((uintptr_t)((__half*)sink.base + at) & 15) : !((uintptr_t)((float*)sink.base + at) & 15);
    if (src_ok && dst_ok) {
      uint32_t h[8];
      if (fr.shuffled) {
        const uint4 a = *(const uint4*)lo, b = *(const uint4*)(lo + ne);
        h[0] = blosc_weave(a.x, b.x, 0); h[1] = blosc_weave(a.x, b.x, 1); h[2] = blosc_weave(a.y, b.y, 0); h[3] = blosc_weave(a.y, b.y, 1);
        h[4] = blosc_weave(a.z, b.z, 0); h[5] = blosc_weave(a.z, b.z, 1); h[6] = blosc_weave(a.w, b.w, 0); h[7] = blosc_weave(a.w, b.w, 1);
      } else {
        const uint4 a = *(const uint4*)(img + q0), b = *(const uint4*)(img + q0 + 16);
        h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w; h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
      }
      if (SINK == BLOSC_SINK_F16) {
        uint4* o = (uint4*)((__half*)sink.base + at);
        o[0] = make_uint4(h[0], h[1], h[2], h[3]);
        o[1] = make_uint4(h[4], h[5], h[6], h[7]);
      } else {
        float4* o = (float4*)((float*)sink.base + at);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[i] = make_float4(__half2float(__ushort_as_half((unsigned short)(h[2 * i] & 0xffffu))), __half2float(__ushort_as_half((unsigned short)(h[2 * i] >> 16))),
                             __half2float(__ushort_as_half((unsigned short)(h[2 * i + 1] & 0xffffu))), __half2float(__ushort_as_half((unsigned short)(h[2 * i + 1] >> 16))));
      }
      return;
    }
  }
  for (int e = e0; e < e0 + cnt; ++e) {
    const int rw = e / W, x = e - rw * W, c = rw / H, y = rw - c * H;
    if (c >= fr.clip[0] || y >= fr.clip[1] || x >= fr.clip[2]) continue;
    const unsigned short v = (unsigned short)(blosc_plain_byte(fr, img, 2 * e) | (blosc_plain_byte(fr, img, 2 * e + 1) << 8));
    const long at = fr.dst + (long)c * sink.cstride + (long)y * sink.pitch + x;
    if (SINK == BLOSC_SINK_F16) ((unsigned short*)sink.base)[at] = v;
    else ((float*)sink.base)[at] = __half2float(__ushort_as_half(v));
  }
}

hipError_t launch_blosc_decode(const uint8_t* frames, const BloscStream* tab, int nstreams, int longest_lz4, const BloscDecFrame* fr,
                               int nframes, int max_nbytes, uint8_t* scratch, const BloscSink& sink, int32_t* status, hipStream_t s) {
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)nframes, s);
  if (e != hipSuccess) return e;
  if (nstreams > 0) {
    static DevOnce once;
    if (once.need()) {
      e = hipFuncSetAttribute((const void*)blosc_lz4_decode_kernel<65536>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
      if (e != hipSuccess) return e;
      once.mark();
    }
    // the whole stream in LDS up to 32768 bytes (five waves a CU at that size, more below it), else the 64 KiB ring (two)
    const int win = longest_lz4 <= 32768 ? 32768 : 65536;
    int lds = (longest_lz4 + 16 + 15) & ~15;                       // + 16: the shift
    if (lds > win) lds = win;                                      // wraps: the whole ring
    if (lds < 256) lds = 256;
    if (win == 32768) blosc_lz4_decode_kernel<32768><<<dim3((unsigned)nstreams), dim3(64), (size_t)lds, s>>>(frames, tab, scratch, status);
    else blosc_lz4_decode_kernel<65536><<<dim3((unsigned)nstreams), dim3(64), (size_t)lds, s>>>(frames, tab, scratch, status);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (max_nbytes < 1) return hipSuccess;
  const dim3 grid((unsigned)(((size_t)max_nbytes + 16 * 256 - 1) / (16 * 256)), (unsigned)nframes);
  if (sink.mode == BLOSC_SINK_BYTES) blosc_unshuffle_kernel<BLOSC_SINK_BYTES><<<grid, dim3(256), 0, s>>>(fr, scratch, sink, status);
  else if (sink.mode == BLOSC_SINK_F16) blosc_unshuffle_kernel<BLOSC_SINK_F16><<<grid, dim3(256), 0, s>>>(fr, scratch, sink, status);
  else blosc_unshuffle_kernel<BLOSC_SINK_F32><<<grid, dim3(256), 0, s>>>(fr, scratch, sink, status);
  return hipGetLastError();
}

}  // namespace tmk
