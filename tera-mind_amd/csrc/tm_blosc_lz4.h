// The LZ4 sequence walk of the Blosc decoder, with every check, shared by the GPU kernel (tm_blosc.hip: one wave per
// stream, the copies by all 64 lanes) and the host check (tools/blosc_decode_check.cpp: scalar copies into buffers of
// exactly the stream's sizes).  It accepts and refuses what lz4_block_decode of tm_io.hip accepts and refuses, followed by
// that decoder's "decodes to the split size" test: the lenient reader, no end-of-block rules.
//
// The walk only reads source bytes through io.byte(p) with 0 <= p < n and hands the copies to
//   io.literals(ip, op, len)   src[ip, ip + len) -> dst[op, op + len), 1 <= len, ip + len <= n, op + len <= cap
//   io.match(op, off, len)     dst[op + k] = dst[op - off + k % off] for k < len, 1 <= off <= op, 4 <= len, op + len <= cap
// so an `io` that does exactly that never leaves [0, n) of the source or [0, cap) of the destination.  Every loop takes at
// least one source byte per turn and stops at n: a corrupt stream ends.  Lengths stay below 2^31: a length that passes `cap`
// is refused where it does (the reader refuses it at the latest when the run is copied).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TM_LZ4_HD __host__ __device__ inline
#else
#define TM_LZ4_HD inline
#endif

namespace tmk {

// status[frame] of tm_blosc_decompress_dev / _tiles: 0, or the largest code of the frame's streams
enum {
  BLOSC_DEC_OK = 0,
  BLOSC_DEC_SHORT = 1,          // the stream ends short of its plain size
  BLOSC_DEC_LEN_EXT = 2,        // a length extension runs off the end of the stream
  BLOSC_DEC_LIT_SRC = 3,        // a literal run passes the end of the stream
  BLOSC_DEC_LIT_DST = 4,        // a literal run passes the plain size
  BLOSC_DEC_OFF_CUT = 5,        // fewer than two bytes where an offset is due
  BLOSC_DEC_OFF_ZERO = 6,       // offset 0
  BLOSC_DEC_OFF_FAR = 7,        // offset beyond the bytes produced
  BLOSC_DEC_MATCH_DST = 8,      // a match passes the plain size
};

template <class IO>
TM_LZ4_HD int blosc_lz4_walk(IO& io, int n, int cap) {
  int ip = 0, op = 0;
  while (ip < n) {
    const unsigned tok = io.byte(ip++);
    int lit = (int)(tok >> 4);
    if (lit == 15) {
      unsigned b;
      do {
        if (ip >= n) return BLOSC_DEC_LEN_EXT;
        b = io.byte(ip++);
        lit += (int)b;
        if (lit > cap) return BLOSC_DEC_LIT_DST;
      } while (b == 255);
    }
    if (lit > n - ip) return BLOSC_DEC_LIT_SRC;
    if (lit > cap - op) return BLOSC_DEC_LIT_DST;
    if (lit) io.literals(ip, op, lit);
    ip += lit;
    op += lit;
    if (ip >= n) break;                                   // the last sequence carries literals only
    if (n - ip < 2) return BLOSC_DEC_OFF_CUT;
    const unsigned off_lo = io.byte(ip);                  // in this order: the source is read forwards only
    const unsigned off_hi = io.byte(ip + 1);
    const int off = (int)(off_lo | (off_hi << 8));
    ip += 2;
    if (off == 0) return BLOSC_DEC_OFF_ZERO;
    if (off > op) return BLOSC_DEC_OFF_FAR;
    int ml = (int)(tok & 15);
    if (ml == 15) {
      unsigned b;
      do {
        if (ip >= n) return BLOSC_DEC_LEN_EXT;
        b = io.byte(ip++);
        ml += (int)b;
        if (ml > cap) return BLOSC_DEC_MATCH_DST;
      } while (b == 255);
    }
    ml += 4;
    if (ml > cap - op) return BLOSC_DEC_MATCH_DST;
    io.match(op, off, ml);
    op += ml;
  }
  return op == cap ? BLOSC_DEC_OK : BLOSC_DEC_SHORT;
}

}  // namespace tmk
