// Stand-alone host check of the LZ4 sequence walk of the GPU Blosc decoder (no GPU): blosc_lz4_walk of
// tera-mind_amd/csrc/tm_blosc_lz4.h -- the routine the kernel runs, with every check in it -- is driven with a scalar stand-in
// for the wave's copies over a corpus of streams (`python tests/blosc_decode_cases.py corpus.bin`: every stream of every good
// frame with its plain bytes, and the frames with one corrupt stream).  Each stream is copied into a heap buffer of exactly
// its compressed length and decoded into one of exactly its plain length, so that built with -fsanitize=address,undefined a
// read or write outside either aborts.  The stand-in also asserts the contract the walk promises its copies (ranges, 1 <=
// offset <= bytes produced) and that the source is read forwards only, which the kernel's register window relies on.  Match
// copies use the kernel's chunk rule: 64 positions at a time, each from the smallest multiple of the offset that lands before
// the chunk.  A good stream must decode to its plain bytes, a stream marked corrupt must be refused with a non-zero code, and
// bytes the walk did not produce must be untouched.
//   hipcc -O1 -g -std=c++17 -x hip --cuda-host-only -fsanitize=address,undefined -Itera-mind_amd/csrc \
//         tools/blosc_decode_check.cpp -o blosc_decode_check && ./blosc_decode_check corpus.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "tm_blosc_lz4.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct ScalarIO {
  const uint8_t* src; int n;
  uint8_t* dst; int cap;
  int last_read = -1, produced = 0;
  std::string name;
  unsigned byte(int p) {
    CHECK(p >= 0 && p < n, "%s: byte(%d) outside [0, %d)", name.c_str(), p, n);
    CHECK(p > last_read, "%s: byte(%d) after byte(%d): the source is read forwards only", name.c_str(), p, last_read);
    last_read = p;
    return src[p];
  }
  void literals(int ip, int op, int len) {
    CHECK(len >= 1 && ip > last_read && ip + len <= n && op == produced && op + len <= cap, "%s: literals(%d, %d, %d)", name.c_str(), ip, op, len);
    for (int k = 0; k < len; ++k) dst[op + k] = src[ip + k];
    last_read = ip + len - 1;
    produced = op + len;
  }
  void match(int op, int off, int len) {
    CHECK(len >= 4 && off >= 1 && off <= op && op == produced && op + len <= cap, "%s: match(%d, %d, %d)", name.c_str(), op, off, len);
    for (int c = 0; c < len; c += 64) {                             // the kernel's chunk: all 64 lanes read, then all write
      uint8_t v[64];
      const int cnt = len - c < 64 ? len - c : 64;
      for (int lane = 0; lane < cnt; ++lane) {
        const int back = off >= 64 ? off : (lane / off + 1) * off;
        CHECK(back <= 65535 + 63 && op + c + lane - back < op + c, "%s: lane %d reads inside its own chunk", name.c_str(), lane);
        v[lane] = dst[op + c + lane - back];
      }
      for (int lane = 0; lane < cnt; ++lane) dst[op + c + lane] = v[lane];
    }
    produced = op + len;
  }
};

// The kernel's history ring, lane by lane: position p lives at ring[(p + shift) & (WIN - 1)], a chunk of 64 positions is read
// by all lanes before any lane writes, and before a chunk is written the slots it takes are flushed to `out` (make_room) in
// 16-byte vectors of (position + shift).  `out` has exactly the plain size; nothing is ever read back from it.
struct RingIO {
  const uint8_t* src; int n;
  uint8_t* out; int cap;
  int WIN, shift, flushed = 0;
  std::vector<uint8_t> ring;
  std::string name;
  unsigned byte(int p) { return src[p]; }
  uint8_t& slot(int p) { return ring[(size_t)((p + shift) & (WIN - 1))]; }
  void flush(int to) {
    CHECK(to >= flushed && to <= cap, "%s: flush(%d) from %d of %d", name.c_str(), to, flushed, cap);
    const int from = flushed;
    int head = from + ((16 - ((from + shift) & 15)) & 15);
    if (head > to) head = to;
    for (int lane = 0; lane < 64; ++lane) if (from + lane < head) out[from + lane] = slot(from + lane);
    const int nv = (to - head) >> 4;
    for (int v = 0; v < nv; ++v) {
      const int p = head + 16 * v, at = (p + shift) & (WIN - 1);
      CHECK(at % 16 == 0 && at + 16 <= WIN, "%s: vector at ring offset %d", name.c_str(), at);
      memcpy(out + p, &ring[(size_t)at], 16);
    }
    const int tail = head + 16 * nv;
    CHECK(to - tail < 64 && head - from < 64, "%s: flush edges longer than a wave", name.c_str());
    for (int lane = 0; lane < 64; ++lane) if (tail + lane < to) out[tail + lane] = slot(tail + lane);
    flushed = to;
  }
  void make_room(int c) { if (c + 64 - flushed > WIN) flush(c - ((c + shift) & 15)); }
  void literals(int ip, int op, int len) {
    for (int c = 0; c < len; c += 64) {
      make_room(op + c);
      for (int lane = 0; lane < 64 && c + lane < len; ++lane) slot(op + c + lane) = src[ip + c + lane];
    }
  }
  void match(int op, int off, int len) {
    for (int c = 0; c < len; c += 64) {
      make_room(op + c);
      uint8_t v[64];
      const int cnt = len - c < 64 ? len - c : 64;
      for (int lane = 0; lane < cnt; ++lane) v[lane] = slot(op + c + lane - (off >= 64 ? off : (lane / off + 1) * off));
      for (int lane = 0; lane < cnt; ++lane) slot(op + c + lane) = v[lane];
    }
  }
};

static void ring_check(const std::string& name, const uint8_t* comp, int clen, const uint8_t* want, int plen, int WIN, int shift) {
  RingIO io;
  io.src = comp; io.n = clen; io.cap = plen; io.WIN = WIN; io.shift = shift; io.name = name;
  io.ring.assign((size_t)WIN, 0xEE);
  uint8_t* out = (uint8_t*)malloc(plen ? plen : 1);
  io.out = out;
  const int code = tmk::blosc_lz4_walk(io, clen, plen);
  CHECK(code == 0, "%s: ring %d shift %d: code %d", name.c_str(), WIN, shift, code);
  if (code == 0) {
    io.flush(plen);
    CHECK(memcmp(out, want, plen) == 0, "%s: ring %d shift %d: bytes differ", name.c_str(), WIN, shift);
  }
  free(out);
}

static uint32_t rd32(FILE* f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) { printf("corpus truncated\n"); exit(2); }
  return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  char magic[8];
  if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "TMBLZ4C1", 8)) { printf("%s: not a corpus\n", argv[1]); return 2; }
  const uint32_t count = rd32(f);
  int good = 0, stored = 0, refused = 0, rings = 0, codes[16] = {};
  size_t bytes = 0, longest = 0;
  for (uint32_t r = 0; r < count; ++r) {
    const uint32_t nl = rd32(f);
    std::string name(nl, ' ');
    if (fread(&name[0], 1, nl, f) != nl) return 2;
    const uint32_t expect = rd32(f), clen = rd32(f), plen = rd32(f);
    uint8_t* comp = (uint8_t*)malloc(clen ? clen : 1);             // exactly the stream: a byte past it is the sanitizer's
    uint8_t* plain = (uint8_t*)malloc(plen ? plen : 1);
    uint8_t* want = (uint8_t*)malloc(plen ? plen : 1);
    if (fread(comp, 1, clen, f) != clen) return 2;
    if (!expect && fread(want, 1, plen, f) != plen) return 2;
    memset(plain, 0xA5, plen);
    if (clen == plen) {                                            // stored: a copy, no walk
      CHECK(!expect, "%s: a corrupt stream of the plain size would be taken as stored", name.c_str());
      CHECK(memcmp(comp, want, plen) == 0, "%s: stored stream differs", name.c_str());
      ++stored;
    } else {
      ScalarIO io;
      io.src = comp; io.n = (int)clen; io.dst = plain; io.cap = (int)plen; io.name = name;
      const int code = tmk::blosc_lz4_walk(io, (int)clen, (int)plen);
      CHECK(code >= 0 && code < 16, "%s: code %d", name.c_str(), code);
      if (expect) {
        CHECK(code != 0, "%s: a corrupt stream was accepted", name.c_str());
        if (code) { ++refused; ++codes[code & 15]; printf("refused  %-48s code %d after %d of %u bytes\n", name.c_str(), code, io.produced, plen); }
      } else {
        CHECK(code == 0, "%s: refused with code %d", name.c_str(), code);
        CHECK(io.produced == (int)plen && memcmp(plain, want, plen) == 0, "%s: decoded bytes differ", name.c_str());
        ++good;
        for (int shift : {0, 5, 15}) {                               // the two windows the kernel is built with
          ring_check(name, comp, (int)clen, want, (int)plen, 65536, shift);
          if (plen <= 32768) ring_check(name, comp, (int)clen, want, (int)plen, 32768, shift);
          rings += 1 + (plen <= 32768);
        }
      }
      for (uint32_t k = (uint32_t)io.produced; k < plen; ++k)
        if (plain[k] != 0xA5) { CHECK(false, "%s: byte %u beyond the %d produced was written", name.c_str(), k, io.produced); break; }
      bytes += plen;
      if (plen > longest) longest = plen;
    }
    free(comp); free(plain); free(want);
  }
  fclose(f);
  printf("%u streams: %d LZ4 streams decoded to their plain bytes (%zu bytes, longest %zu), %d stored, %d corrupt refused (codes", count, good,
         bytes, longest, stored, refused);
  for (int c = 1; c < 16; ++c)
    if (codes[c]) printf(" %d:%d", c, codes[c]);
  printf(")\n%d ring decodes (windows 65536 and 32768, shifts 0, 5, 15) gave the same bytes\n", rings);
  printf(fails ? "FAILED: %d checks\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
