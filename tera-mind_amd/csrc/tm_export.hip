// Slice export: what the reference leaves to libvips (infer_brn.py:11-54, `tiffsave(tile=True,
// compression='jpeg', pyramid=True, bigtiff=True)`), done next to the resident canvas.
//
//  * u8_shrink2_kernel: one pyramid level from the one above, dst = (a + b + c + d + 2) >> 2 over 2 x 2 blocks of uint8; an odd
//    last row / column is repeated.
//  * jpeg_tile_kernel: baseline JPEG (ITU-T T.81) of one 8-bit grey component, one 256 x 256 tile per scan.  Every step is
//    exact integer work restated from the published algorithm: the 8 x 8 "islow" forward DCT (CONST_BITS 13, PASS1_BITS 2), the
//    quantiser (|c| + qv / 2) / qv with qv = q << 3, zigzag order, DC prediction inside the tile, the typical Huffman tables of
//    Annex K.3, MSB-first bit packing, a zero byte after every 0xFF, one-bit padding of the last byte.  The kernel emits the
//    entropy-coded segment only; markers are the host's.
//  * jpeg_offsets_kernel / jpeg_compact_kernel: the filled slots of a batch packed back to back.
//  * jpeg_tables: the tables-only datastream SOI DQT DHT DHT EOI, from the same table statements the kernel encodes with.
//  * rgb_compose_kernel / jpeg_tile_rgb_kernel / jpeg_tables_rgb: the two-stain colour composite of utils/vis_mba.py:193-195
//    (three planes as R, G, B, brightness, ontology overlay as onto_overlay :118-179) and its 4:4:4 YCbCr JPEG tiles, the
//    composite formed in the encoder's block load; Annex K.2 / K.4 / K.6 for the chrominance components.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/teramind_hip.h"
#include "tm_kernels.h"

namespace tmk {

// ---- the one statement of the tables (T.81 Annex K) --------------------------------------------------------------------
// K.1 luminance quantisation table, natural (row-major) order
static constexpr uint8_t K1_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                        14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                        18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
// zigzag position -> natural index
static constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// K.3 typical luminance Huffman tables: number of codes of each length 1 .. 16, then the symbols in code order
static constexpr uint8_t DC_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static constexpr uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static constexpr uint8_t AC_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
static constexpr uint8_t AC_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// K.2 chrominance quantisation table, natural order
static constexpr uint8_t K2_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                          99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// K.4 / K.6 typical chrominance Huffman tables (the DC symbols are DC_VALS again)
static constexpr uint8_t DC_BITS_C[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static constexpr uint8_t AC_BITS_C[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
static constexpr uint8_t AC_VALS_C[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// encoder form of the Huffman tables: entry = (code << 8) | length, indexed by symbol (Annex C code assignment)
struct HuffEnc {
  uint32_t dc[16];
  uint32_t ac[256];
};
static constexpr HuffEnc make_huff(const uint8_t* dc_bits, const uint8_t* dc_vals, const uint8_t* ac_bits, const uint8_t* ac_vals) {
  HuffEnc h{};
  unsigned code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < dc_bits[l - 1]; ++i) h.dc[dc_vals[k++]] = (code++ << 8) | (unsigned)l;
    code <<= 1;
  }
  code = 0;
  k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < ac_bits[l - 1]; ++i) h.ac[ac_vals[k++]] = (code++ << 8) | (unsigned)l;
    code <<= 1;
  }
  return h;
}
__device__ __constant__ HuffEnc d_huff = make_huff(DC_BITS, DC_VALS, AC_BITS, AC_VALS);
__device__ __constant__ HuffEnc d_huff_c = make_huff(DC_BITS_C, DC_VALS, AC_BITS_C, AC_VALS_C);

// the K.1 table (or `base`) at `quality` (1 .. 100), natural order: s = 5000 / Q below 50, else 200 - 2 Q;
// q = clamp((base s + 50) / 100, 1, 255)
static void scaled_qtable(int quality, uint8_t q[64], const uint8_t* base = K1_LUMA) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    int v = (base[i] * s + 50) / 100;
    q[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
  }
}

// Quantiser operands of the kernel, natural order.  n / qv for n < 2^17 and qv <= 2040 is umulhi(n, ceil(2^32 / qv)) exactly:
// with m = ceil(2^32 / qv) the excess e = m qv - 2^32 is below qv < 2^11, so n e < 2^28 < 2^32 (Granlund-Montgomery).
struct JpegQ {
  uint32_t recip[64];
  uint16_t qv[64];
};
static JpegQ make_jpegq(int quality, const uint8_t* base = K1_LUMA) {
  uint8_t q[64];
  scaled_qtable(quality, q, base);
  JpegQ t;
  for (int i = 0; i < 64; ++i) {
    const uint32_t qv = (uint32_t)q[i] << 3;
    t.qv[i] = (uint16_t)qv;
    t.recip[i] = (uint32_t)(((1ull << 32) + qv - 1) / qv);
  }
  return t;
}

int jpeg_tables(int quality, void* buf, size_t cap, size_t* out_bytes) {
  uint8_t t[2 + (2 + 67) + (2 + 31) + (2 + 181) + 2], q[64];
  size_t n = 0;
  scaled_qtable(quality, q);
  t[n++] = 0xFF; t[n++] = 0xD8;                                          // SOI
  t[n++] = 0xFF; t[n++] = 0xDB; t[n++] = 0; t[n++] = 67; t[n++] = 0;     // DQT: 8-bit precision, table 0, zigzag order
  for (int k = 0; k < 64; ++k) t[n++] = q[ZIGZAG[k]];
  t[n++] = 0xFF; t[n++] = 0xC4; t[n++] = 0; t[n++] = 31; t[n++] = 0x00;  // DHT: DC table 0
  memcpy(t + n, DC_BITS, 16); n += 16;
  memcpy(t + n, DC_VALS, 12); n += 12;
  t[n++] = 0xFF; t[n++] = 0xC4; t[n++] = 0; t[n++] = 181; t[n++] = 0x10; // DHT: AC table 0
  memcpy(t + n, AC_BITS, 16); n += 16;
  memcpy(t + n, AC_VALS, 162); n += 162;
  t[n++] = 0xFF; t[n++] = 0xD9;                                          // EOI
  if (out_bytes) *out_bytes = n;
  if (!buf) return TM_OK;                                                // size query
  if (cap < n) return fail(TM_ERR_ARG, "tm_jpeg_tables: buffer of %zu bytes, the tables take %zu", cap, n);
  memcpy(buf, t, n);
  return TM_OK;
}

// the colour datastream: SOI DQT(0) DQT(1) DHT(DC 0) DHT(AC 0) DHT(DC 1) DHT(AC 1) EOI, the segments and the order libjpeg writes
int jpeg_tables_rgb(int quality, void* buf, size_t cap, size_t* out_bytes) {
  uint8_t t[2 + 2 * (2 + 67) + 2 * (2 + 31) + 2 * (2 + 181) + 2], q[64];
  size_t n = 0;
  t[n++] = 0xFF; t[n++] = 0xD8;
  for (int id = 0; id < 2; ++id) {                                       // DQT: K.1 as table 0, K.2 as table 1
    scaled_qtable(quality, q, id ? K2_CHROMA : K1_LUMA);
    t[n++] = 0xFF; t[n++] = 0xDB; t[n++] = 0; t[n++] = 67; t[n++] = (uint8_t)id;
    for (int k = 0; k < 64; ++k) t[n++] = q[ZIGZAG[k]];
  }
  for (int id = 0; id < 2; ++id) {                                       // DHT: K.3 / K.5 as tables 0, K.4 / K.6 as tables 1
    t[n++] = 0xFF; t[n++] = 0xC4; t[n++] = 0; t[n++] = 31; t[n++] = (uint8_t)id;
    memcpy(t + n, id ? DC_BITS_C : DC_BITS, 16); n += 16;
    memcpy(t + n, DC_VALS, 12); n += 12;
    t[n++] = 0xFF; t[n++] = 0xC4; t[n++] = 0; t[n++] = 181; t[n++] = (uint8_t)(0x10 | id);
    memcpy(t + n, id ? AC_BITS_C : AC_BITS, 16); n += 16;
    memcpy(t + n, id ? AC_VALS_C : AC_VALS, 162); n += 162;
  }
  t[n++] = 0xFF; t[n++] = 0xD9;
  if (out_bytes) *out_bytes = n;
  if (!buf) return TM_OK;                                                // size query
  if (cap < n) return fail(TM_ERR_ARG, "tm_jpeg_tables_rgb: buffer of %zu bytes, the tables take %zu", cap, n);
  memcpy(buf, t, n);
  return TM_OK;
}

// ---- 2 x 2 reduction -----------------------------------------------------------------------------------------------------
// one thread per 8 destination pixels of a row: two 16-byte loads and one 8-byte store where the pointers, the pitches and
// the row end allow (`vec`: bit 0 = source, bit 1 = destination), single bytes with the clamped edge otherwise
__device__ __forceinline__ uint32_t pair_sums(uint32_t w) { return (w & 0x00FF00FFu) + ((w >> 8) & 0x00FF00FFu); }
__global__ __launch_bounds__(256) void u8_shrink2_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, long spitch,
                                                         uint8_t* __restrict__ dst, int Hd, int Wd, long dpitch, int gx, int vec) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int y = (int)(idx / gx), xg = (int)(idx - (long)y * gx);
  if (y >= Hd) return;
  const int y0 = 2 * y, y1 = 2 * y + 1 < Hs ? 2 * y + 1 : Hs - 1, x = xg * 8;
  const uint8_t* r0 = src + (long)y0 * spitch;
  const uint8_t* r1 = src + (long)y1 * spitch;
  uint8_t* o = dst + (long)y * dpitch + x;
  uint32_t out[2];
  if ((vec & 1) && 2 * x + 16 <= Ws) {
    const uint4 a = *(const uint4*)(r0 + 2 * x), b = *(const uint4*)(r1 + 2 * x);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    uint32_t px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i] = ((pair_sums(aw[i]) + pair_sums(bw[i]) + 0x00020002u) >> 2) & 0x00FF00FFu;   // two pixels, 16 bits apart
    out[0] = (px[0] & 0xFF) | ((px[0] >> 8) & 0xFF00) | ((px[1] & 0xFF) << 16) | ((px[1] >> 16) << 24);
    out[1] = (px[2] & 0xFF) | ((px[2] >> 8) & 0xFF00) | ((px[3] & 0xFF) << 16) | ((px[3] >> 16) << 24);
  } else {
    out[0] = out[1] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int xa = 2 * (x + i) < Ws ? 2 * (x + i) : Ws - 1, xb = 2 * (x + i) + 1 < Ws ? 2 * (x + i) + 1 : Ws - 1;
      const uint32_t v = ((uint32_t)r0[xa] + r0[xb] + r1[xa] + r1[xb] + 2) >> 2;
      out[i >> 2] |= v << (8 * (i & 3));
    }
  }
  if ((vec & 2) && x + 8 <= Wd) {
    *(uint2*)o = make_uint2(out[0], out[1]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (x + i < Wd) o[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
  }
}

hipError_t launch_u8_shrink2(const uint8_t* src, int Hs, int Ws, long spitch, uint8_t* dst, long dpitch, hipStream_t s) {
  const int Hd = (Hs + 1) / 2, Wd = (Ws + 1) / 2, gx = (Wd + 7) / 8;
  const int vec = ((((uintptr_t)src | (uintptr_t)spitch) & 15) == 0 ? 1 : 0) | ((((uintptr_t)dst | (uintptr_t)dpitch) & 7) == 0 ? 2 : 0);
  const long blocks = ((long)Hd * gx + 255) / 256;
  u8_shrink2_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(src, Hs, Ws, spitch, dst, Hd, Wd, dpitch, gx, vec);
  return hipGetLastError();
}

// ---- JPEG tile encoder ---------------------------------------------------------------------------------------------------
// One workgroup of 256 lanes per tile; lane l owns the four 8 x 8 blocks 4 l .. 4 l + 3 of the tile's raster order (the
// same block row), so its share of the scan is one contiguous bit run.
//   count   DCT + quantiser per block into the lane's LDS row (zigzag order), AC bit count, DC to LDS
//   scan    DC differences, bits per lane, exclusive scan -> bit offset of every lane, bits of the tile
//   emit    the same DCT again (cheaper than keeping 128 KB of coefficients), codes into the zeroed bit buffer: whole words
//           by plain stores, the two words a lane shares with its neighbours by OR (disjoint bits: order independent)
//   stuff   0xFF count -> need[tile]; if the slot holds it, scan the counts in 4 KB windows and write the stuffed bytes
constexpr int JPEG_ROW = 33;                                   // dwords per lane row: 64 int16 + one pad dword (bank spread)
constexpr int JPEG_BLOCK_BITS = 1660;                          // 20 (DC) + 63 * 26 (AC) = 1658 at most
constexpr int JPEG_WG_WORDS = (1024 * JPEG_BLOCK_BITS / 32 + 15) / 16 * 16;   // bit buffer of one workgroup, 32-bit words

template <int PASS>
__device__ __forceinline__ void fdct_1d(int* d, const int s) {
  constexpr int CB = 13, P1 = 2;
  const int t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
  const int t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int SH = PASS == 1 ? CB - P1 : CB + P1, RND = 1 << (SH - 1);
  if (PASS == 1) {
    d[0] = (t10 + t11) << P1;
    d[4 * s] = (t10 - t11) << P1;
  } else {
    d[0] = (t10 + t11 + (1 << (P1 - 1))) >> P1;
    d[4 * s] = (t10 - t11 + (1 << (P1 - 1))) >> P1;
  }
  int z1 = (t12 + t13) * 4433;
  d[2 * s] = (z1 + t13 * 6270 + RND) >> SH;
  d[6 * s] = (z1 - t12 * 15137 + RND) >> SH;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * s] = (m4 + z1 + z3 + RND) >> SH;
  d[5 * s] = (m5 + z2 + z4 + RND) >> SH;
  d[3 * s] = (m6 + z2 + z3 + RND) >> SH;
  d[s] = (m7 + z1 + z4 + RND) >> SH;
}

// the quantised block at (y0, x0) into `row` (LDS, 32 dwords = 64 int16 in zigzag order); returns the quantised DC.
// A block that crosses the image edge (or an unaligned plane) goes
// through the row first, byte by byte with the clamped coordinates, in a rolled loop: the edge is rare and the code stays small.
__device__ __forceinline__ int block_coefs(const uint8_t* __restrict__ plane, long pitch, int H, int W, int y0, int x0, bool vec8,
                                           const JpegQ& q, uint32_t* row) {
  uint32_t px[16];
  if (vec8 && y0 + 8 <= H && x0 + 8 <= W) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint2 v = *(const uint2*)(plane + (long)(y0 + r) * pitch + x0);
      px[2 * r] = v.x;
      px[2 * r + 1] = v.y;
    }
  } else {
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const uint8_t* p = plane + (long)(y0 + r < H ? y0 + r : H - 1) * pitch;
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        lo |= (uint32_t)p[x0 + c < W ? x0 + c : W - 1] << (8 * c);
        hi |= (uint32_t)p[x0 + 4 + c < W ? x0 + 4 + c : W - 1] << (8 * c);
      }
      row[2 * r] = lo;
      row[2 * r + 1] = hi;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) px[k] = row[k];
  }
  int d[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d[r * 8 + c] = (int)((px[2 * r] >> (8 * c)) & 255) - 128;
      d[r * 8 + 4 + c] = (int)((px[2 * r + 1] >> (8 * c)) & 255) - 128;
    }
    fdct_1d<1>(d + r * 8, 1);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct_1d<2>(d + c, 8);
#pragma unroll
  for (int n = 0; n < 64; ++n) {
    const int v = d[n];
    const int t = (int)__umulhi((uint32_t)(v < 0 ? -v : v) + (q.qv[n] >> 1), q.recip[n]);
    d[n] = v < 0 ? -t : t;
  }
#pragma unroll
  for (int k = 0; k < 32; ++k)
    row[k] = ((uint32_t)d[ZIGZAG[2 * k]] & 0xFFFFu) | ((uint32_t)d[ZIGZAG[2 * k + 1]] << 16);
  return d[0];
}

// MSB-first bit run of one lane, starting `bit` bits into the workgroup's buffer
struct BitRun {
  uint64_t acc;
  int n;
  uint32_t* p;
  bool first;
  __device__ __forceinline__ void start(uint32_t* buf, int bit) {
    p = buf + (bit >> 5);
    n = bit & 31;
    acc = 0;
    first = true;
  }
  __device__ __forceinline__ void put(uint32_t v, int len) {      // len <= 27, v < 2^len
    acc = (acc << len) | v;
    n += len;
    if (n >= 32) {
      const uint32_t w = (uint32_t)(acc >> (n - 32));
      if (first) atomicOr(p, w); else *p = w;
      first = false;
      ++p;
      n -= 32;
      acc &= (1ull << n) - 1;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(p, (uint32_t)(acc << (32 - n)));
  }
};

__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(v < 0 ? -v : v); }       // 0 for 0
__device__ __forceinline__ uint32_t value_bits(int v, int s) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1); }

// the AC coefficients of the lane's row: returns their bit count, emits them if `emit`
__device__ __forceinline__ int encode_ac(const uint32_t* row, const uint32_t* s_ac, bool emit, BitRun& br) {
  int bits = 0, run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = (int)(int16_t)(row[k >> 1] >> (16 * (k & 1)));
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {                                             // ZRL
      const uint32_t e = s_ac[0xF0];
      bits += e & 255;
      if (emit) br.put(e >> 8, e & 255);
      run -= 16;
    }
    const int s = bit_size(v);
    const uint32_t e = s_ac[(run << 4) | s];
    bits += (e & 255) + s;
    if (emit) br.put(((e >> 8) << s) | value_bits(v, s), (e & 255) + s);
    run = 0;
  }
  if (run) {                                                       // EOB
    const uint32_t e = s_ac[0];
    bits += e & 255;
    if (emit) br.put(e >> 8, e & 255);
  }
  return bits;
}

// exclusive scan of one int per lane over the 256 lanes; every lane gets the total.  Called by all lanes.
__device__ __forceinline__ int block_scan_excl(int v, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const int t = __shfl_up(inc, dlt, 64);
    if (lane >= dlt) inc += t;
  }
  __syncthreads();                                                 // s_wave may still be read from the call before
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = s_wave[i];
    if (i < wv) base += t;
    total += t;
  }
  return base + inc - v;
}

__device__ __forceinline__ int count_ff(uint32_t w) {
  return ((w & 0xFFu) == 0xFFu) + ((w & 0xFF00u) == 0xFF00u) + ((w & 0xFF0000u) == 0xFF0000u) + ((w >> 24) == 0xFFu);
}

__global__ __launch_bounds__(256) void jpeg_tile_kernel(const uint8_t* __restrict__ plane, int H, int W, long pitch, int tiles_x,
                                                        int tile0, int ntiles, const JpegQ q, uint32_t* __restrict__ bitbuf,
                                                        uint8_t* __restrict__ slots, long slot_bytes, int32_t* __restrict__ need) {
  __shared__ uint32_t s_rows[256 * JPEG_ROW];
  __shared__ int s_dc[1024];
  __shared__ uint32_t s_ac[256];
  __shared__ uint32_t s_dcc[16];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x;
  s_ac[tid] = d_huff.ac[tid];
  if (tid < 16) s_dcc[tid] = d_huff.dc[tid];
  uint32_t* row = s_rows + tid * JPEG_ROW;
  uint32_t* buf = bitbuf + (size_t)blockIdx.x * JPEG_WG_WORDS;
  const bool vec8 = (((uintptr_t)plane | (uintptr_t)pitch) & 7) == 0;
  const int b0 = tid * 4, by = b0 >> 5, bx = b0 & 31;              // the lane's first block: row by, columns bx .. bx + 3
  BitRun br;
  __syncthreads();

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tile = tile0 + t, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * 256 + by * 8, x0 = tx * 256 + bx * 8;

    // pass 0 counts, pass 1 emits: one loop body, so that the DCT is instantiated once
    int bits = 0, total_bits = 0, nbytes = 0, nwords = 0;
    for (int pass = 0; pass < 2; ++pass) {
      int prev = (pass && b0) ? s_dc[b0 - 1] : 0;
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        const int dc = block_coefs(plane, pitch, H, W, y0, x0 + 8 * i, vec8, q, row);
        if (pass) {
          const int df = dc - prev, s = bit_size(df);
          const uint32_t e = s_dcc[s];
          br.put(((e >> 8) << s) | value_bits(df, s), (e & 255) + s);
          prev = dc;
        } else {
          s_dc[b0 + i] = dc;
        }
        bits += encode_ac(row, s_ac, pass != 0, br);
      }
      if (pass) break;
      __syncthreads();
      prev = b0 ? s_dc[b0 - 1] : 0;
      for (int i = 0; i < 4; ++i) {
        const int dc = s_dc[b0 + i], s = bit_size(dc - prev);
        bits += (s_dcc[s] & 255) + s;
        prev = dc;
      }
      const int bit0 = block_scan_excl(bits, s_wave, total_bits);
      nbytes = (total_bits + 7) >> 3;
      nwords = (((total_bits + 31) >> 5) + 3) & ~3;               // words in fours: uint4 reads below
      for (int w = tid; w < nwords; w += 256) buf[w] = 0;
      __threadfence();
      __syncthreads();
      br.start(buf, bit0);
    }
    br.finish();
    if (tid == 0 && (total_bits & 7)) {                            // one-bits up to the end of the last byte
      const int np = 8 - (total_bits & 7);
      atomicOr(buf + (total_bits >> 5), ((1u << np) - 1) << (32 - (total_bits & 31) - np));
    }
    __threadfence();                                               // the stuffing pass reads other lanes' words
    __syncthreads();

    // stuffing: bytes past nbytes are zero, so whole words can be counted
    int ff = 0;
    for (int w = tid; w < nwords; w += 256) ff += count_ff(buf[w]);
    int nff;
    block_scan_excl(ff, s_wave, nff);
    const int out_bytes = nbytes + nff;
    if (tid == 0) need[t] = out_bytes;
    if (out_bytes <= slot_bytes) {
      uint8_t* o = slots + (size_t)t * slot_bytes;
      int before = 0;                                              // 0xFF bytes of the windows done
      for (int w0 = 0; w0 < nwords; w0 += 1024) {
        const int w = w0 + 4 * tid;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (w < nwords) v = *(const uint4*)(buf + w);
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
        int win;
        const int mine = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
        int pos = 4 * w + before + block_scan_excl(mine, s_wave, win);
        before += win;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if (4 * w + j < nbytes) {
            const uint32_t b = (vw[j >> 2] >> (24 - 8 * (j & 3))) & 255;
            o[pos++] = (uint8_t)b;
            if (b == 255) o[pos++] = 0;
          }
        }
      }
    }
    __syncthreads();                                               // s_dc and the rows are rewritten by the next tile
  }
}

// offsets[k] = bytes of the filled slots before slot k (a slot that was too small counts 0), offsets[ntiles] = their sum
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int32_t* __restrict__ need, int ntiles, long slot_bytes,
                                                           int64_t* __restrict__ offsets) {
  __shared__ int s_wave[4];
  int64_t base = 0;
  for (int k0 = 0; k0 < ntiles; k0 += 256) {
    const int k = k0 + threadIdx.x;
    const int v = k < ntiles && need[k] <= slot_bytes ? need[k] : 0;
    int win;
    const int ex = block_scan_excl(v, s_wave, win);                // a window holds at most 256 slots of < 2^22 bytes
    if (k < ntiles) offsets[k] = base + ex;
    base += win;
  }
  if (threadIdx.x == 0) offsets[ntiles] = base;
}

__global__ __launch_bounds__(256) void jpeg_compact_kernel(const uint8_t* __restrict__ slots, long slot_bytes, const int32_t* __restrict__ need,
                                                           const int64_t* __restrict__ offsets, uint8_t* __restrict__ packed) {
  const int k = blockIdx.x, n = need[k];
  if (n > slot_bytes) return;
  const uint8_t* s = slots + (size_t)k * slot_bytes;
  uint8_t* o = packed + offsets[k];
  for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) o[i] = s[i];
}

size_t jpeg_scratch_bytes(int ntiles) { return (size_t)(ntiles < JPEG_MAX_WGS ? ntiles : JPEG_MAX_WGS) * JPEG_WG_WORDS * sizeof(uint32_t); }

hipError_t launch_jpeg_tiles(const uint8_t* plane, int H, int W, long pitch, int quality, int tile0, int ntiles, uint32_t* scratch,
                             uint8_t* slots, long slot_bytes, int32_t* need, uint8_t* packed, int64_t* offsets, hipStream_t s) {
  const JpegQ q = make_jpegq(quality);
  const int wgs = ntiles < JPEG_MAX_WGS ? ntiles : JPEG_MAX_WGS;
  jpeg_tile_kernel<<<dim3((unsigned)wgs), dim3(256), 0, s>>>(plane, H, W, pitch, (W + 255) / 256, tile0, ntiles, q, scratch, slots,
                                                            slot_bytes, need);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !packed) return e;
  jpeg_offsets_kernel<<<dim3(1), dim3(256), 0, s>>>(need, ntiles, slot_bytes, offsets);
  jpeg_compact_kernel<<<dim3((unsigned)ntiles, 4), dim3(256), 0, s>>>(slots, slot_bytes, need, offsets, packed);
  return hipGetLastError();
}

// ---- colour composite: three stain planes as R, G, B ------------------------------------------------------------------
// The composite of pixel (y, x) of a level (the one definition; tests/jpeg_rgb_cases.py restates it): the planes' bytes (0 for
// a null plane), brightness v <- min(255, trunc(bright * v)) in float32 unless bright == 1, then the overlay pixel
// ov = overlay[(y oh) / H][(x ow) / W] blended in where it is not black: v <- (ov alpha + v (255 - alpha) + 127) / 255.
// `ovrow` is the overlay row of y (null without an overlay), `ox` the overlay column of x.  -> R | G << 8 | B << 16
__device__ __forceinline__ uint32_t bright_u8(uint32_t v, float b) { return (uint32_t)fminf(b * (float)v, 255.f); }
__device__ __forceinline__ uint32_t compose_px(const RgbSrc& s, int y, int x, const uint8_t* __restrict__ ovrow, int ox) {
  uint32_t v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = s.p[c] ? s.p[c][(long)y * s.pitch[c] + x] : 0u;
  if (s.bright != 1.f) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = bright_u8(v[c], s.bright);
  }
  if (ovrow) {
    const uint8_t* o = ovrow + 3 * ox;
    const uint32_t o0 = o[0], o1 = o[1], o2 = o[2], a = (uint32_t)s.alpha;
    if (o0 | o1 | o2) {
      v[0] = (o0 * a + v[0] * (255u - a) + 127u) / 255u;
      v[1] = (o1 * a + v[1] * (255u - a) + 127u) / 255u;
      v[2] = (o2 * a + v[2] * (255u - a) + 127u) / 255u;
    }
  }
  return v[0] | (v[1] << 8) | (v[2] << 16);
}

// the composite of a whole level, interleaved [H][W][3]: one thread per pixel (the quicklook image; not a hot path)
__global__ __launch_bounds__(256) void rgb_compose_kernel(const RgbSrc s, uint8_t* __restrict__ dst, long dpitch) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)s.H * s.W) return;
  const int y = (int)(idx / s.W), x = (int)(idx - (long)y * s.W);
  const uint8_t* ovrow = s.ov ? s.ov + (long)(((uint32_t)y * (uint32_t)s.oh) / (uint32_t)s.H) * s.ow * 3 : nullptr;
  const uint32_t v = compose_px(s, y, x, ovrow, s.ov ? (int)(((uint32_t)x * (uint32_t)s.ow) / (uint32_t)s.W) : 0);
  uint8_t* o = dst + (long)y * dpitch + 3L * x;
  o[0] = (uint8_t)v;
  o[1] = (uint8_t)(v >> 8);
  o[2] = (uint8_t)(v >> 16);
}

hipError_t launch_rgb_compose(const RgbSrc& src, uint8_t* dst, long dpitch, hipStream_t s) {
  const long blocks = ((long)src.H * src.W + 255) / 256;
  rgb_compose_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(src, dst, dpitch);
  return hipGetLastError();
}

// ---- colour JPEG tile encoder ------------------------------------------------------------------------------------------
// Baseline JPEG of the composite, three components all 1 x 1, one interleaved scan: an MCU is 8 x 8 pixels = one Y, one Cb,
// one Cr block.  The plan is jpeg_tile_kernel's (count, scan, emit, stuff; the DCT run twice) with a lane owning the four
// consecutive MCUs 4 l .. 4 l + 3, twelve blocks in scan order, one contiguous bit run.  The composite is formed in the block
// load and converted one component at a time (libjpeg's fixed-point YCbCr, 16 fraction bits), so that no RGB image of the level
// exists and a lane never holds more than one block's 64 values.  Y goes through quantiser 0 and the K.3 / K.5 codes, Cb and
// Cr through quantiser 1 (K.2) and the K.4 / K.6 codes; the DC chain is per component.  The scan and stuffing parts repeat
// jpeg_tile_kernel's text instead of sharing it: the grey kernel is left exactly as it was measured and pinned.
constexpr int JPEG_WG_WORDS_RGB = 3 * JPEG_WG_WORDS;           // 12 blocks per lane: 22 (DC) + 63 * 26 = 1660 bits each at most
struct JpegQ2 {
  JpegQ t[2];
};

// columns pass, quantiser and zigzag of a block whose rows pass is done, into `row`; returns the quantised DC
__device__ __forceinline__ int fdct_cols_quant(int* d, const JpegQ& q, uint32_t* row) {
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct_1d<2>(d + c, 8);
#pragma unroll
  for (int n = 0; n < 64; ++n) {
    const int v = d[n];
    const int t = (int)__umulhi((uint32_t)(v < 0 ? -v : v) + (q.qv[n] >> 1), q.recip[n]);
    d[n] = v < 0 ? -t : t;
  }
#pragma unroll
  for (int k = 0; k < 32; ++k)
    row[k] = ((uint32_t)d[ZIGZAG[2 * k]] & 0xFFFFu) | ((uint32_t)d[ZIGZAG[2 * k + 1]] << 16);
  return d[0];
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of the composite block at (y0, x0), quantised into `row`; returns the quantised DC.
// vec8: every given plane is 8-byte aligned and there is no overlay, so an interior block is read as one uint2 per plane row.
// Every other block goes through the row byte by byte with the clamped coordinates, in a rolled loop, as in block_coefs.
__device__ __forceinline__ int block_coefs_rgb(const RgbSrc& s, int comp, int y0, int x0, bool vec8, const JpegQ& q, uint32_t* row) {
  const int kr = comp == 0 ? 19595 : comp == 1 ? -11059 : 32768;
  const int kg = comp == 0 ? 38470 : comp == 1 ? -21709 : -27439;
  const int kb = comp == 0 ? 7471 : comp == 1 ? 32768 : -5329;
  const int k0 = comp == 0 ? 32768 : (128 << 16) + 32767;
  // y0 is the same for the lane's twelve blocks.  Left visible, the compiler computes the 24 row addresses of the three planes
  // once per tile and keeps them in 48 registers, which costs the kernel its second wave per SIMD; hidden, they are computed
  // per block, a few dozen instructions next to the transform.
  asm volatile("" : "+v"(y0));
  uint32_t px[16];                                                 // the component's 64 bytes, as in block_coefs
  if (vec8 && y0 + 8 <= s.H && x0 + 8 <= s.W) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint2 p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        p[c] = s.p[c] ? *(const uint2*)(s.p[c] + (long)(y0 + r) * s.pitch[c] + x0) : make_uint2(0u, 0u);
      px[2 * r] = px[2 * r + 1] = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        uint32_t v[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = ((c < 4 ? p[j].x : p[j].y) >> (8 * (c & 3))) & 255u;
        if (s.bright != 1.f) {
#pragma unroll
          for (int j = 0; j < 3; ++j) v[j] = bright_u8(v[j], s.bright);
        }
        px[2 * r + (c >> 2)] |= (uint32_t)((kr * (int)v[0] + kg * (int)v[1] + kb * (int)v[2] + k0) >> 16) << (8 * (c & 3));
      }
    }
  } else {
    uint32_t dH = (uint32_t)s.H, dW = (uint32_t)s.W;               // the divisors, hidden likewise (their reciprocals)
    asm volatile("" : "+s"(dH), "+s"(dW));
    int oxs[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int x = x0 + c < s.W ? x0 + c : s.W - 1;
      oxs[c] = s.ov ? (int)(((uint32_t)x * (uint32_t)s.ow) / dW) : 0;
    }
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      const int y = y0 + r < s.H ? y0 + r : s.H - 1;
      const uint8_t* ovrow = s.ov ? s.ov + (long)(((uint32_t)y * (uint32_t)s.oh) / dH) * s.ow * 3 : nullptr;
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t v = compose_px(s, y, x0 + c < s.W ? x0 + c : s.W - 1, ovrow, oxs[c]);
        const uint32_t e = (uint32_t)((kr * (int)(v & 255u) + kg * (int)((v >> 8) & 255u) + kb * (int)(v >> 16) + k0) >> 16);
        if (c < 4) lo |= e << (8 * c); else hi |= e << (8 * (c - 4));
      }
      row[2 * r] = lo;
      row[2 * r + 1] = hi;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) px[k] = row[k];
  }
  int d[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d[r * 8 + c] = (int)((px[2 * r] >> (8 * c)) & 255) - 128;
      d[r * 8 + 4 + c] = (int)((px[2 * r + 1] >> (8 * c)) & 255) - 128;
    }
    fdct_1d<1>(d + r * 8, 1);
  }
  return fdct_cols_quant(d, q, row);
}

// The table of a block is chosen at run time.  Indexing a kernel argument so makes the compiler read both tables and keep the
// selected values in 96 registers, so the two tables are put in device memory first and read from there by scalar loads.
__global__ void jpeg_q2_kernel(const JpegQ2 q, JpegQ2* __restrict__ dst) {
  if (threadIdx.x == 0) *dst = q;
}

__global__ __launch_bounds__(256, 2) void jpeg_tile_rgb_kernel(const RgbSrc src, int tiles_x, int tile0, int ntiles,
                                                            const JpegQ2* __restrict__ q, uint32_t* __restrict__ bitbuf, uint8_t* __restrict__ slots, long slot_bytes,
                                                            int32_t* __restrict__ need) {
  __shared__ uint32_t s_rows[256 * JPEG_ROW];
  __shared__ int s_dc[3][1024];
  __shared__ uint32_t s_ac[2][256];
  __shared__ uint32_t s_dcc[2][16];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x;
  s_ac[0][tid] = d_huff.ac[tid];
  s_ac[1][tid] = d_huff_c.ac[tid];
  if (tid < 16) {
    s_dcc[0][tid] = d_huff.dc[tid];
    s_dcc[1][tid] = d_huff_c.dc[tid];
  }
  uint32_t* row = s_rows + tid * JPEG_ROW;
  uint32_t* buf = bitbuf + (size_t)blockIdx.x * JPEG_WG_WORDS_RGB;
  bool vec8 = !src.ov;
#pragma unroll
  for (int c = 0; c < 3; ++c) vec8 = vec8 && (!src.p[c] || (((uintptr_t)src.p[c] | (uintptr_t)src.pitch[c]) & 7) == 0);
  const int b0 = tid * 4;                                          // the lane's first MCU: row b0 >> 5, columns (b0 & 31) .. + 3
  BitRun br;
  __syncthreads();

  // This kernel fits two waves per SIMD only just.  Where a part takes the lane index afresh through an empty asm, it is to
  // keep the compiler from carrying that part's multiples of it through the twelve blocks, where they would be spilled.
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tile = tile0 + t, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    int tq = threadIdx.x;
    asm volatile("" : "+v"(tq));
    const int y0 = ty * 256 + (tq >> 3) * 8, x0 = tx * 256 + (tq & 7) * 32;

    int bits = 0, total_bits = 0, nbytes = 0, nwords = 0;
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
          const int tb = __builtin_amdgcn_readfirstlane(c != 0);       // scalar: the quantiser is read by scalar loads
          const int dc = block_coefs_rgb(src, c, y0, x0 + 8 * i, vec8, q->t[tb], row);
          if (pass) {
            const int df = dc - (b0 + i ? s_dc[c][b0 + i - 1] : 0), s = bit_size(df);
            const uint32_t e = s_dcc[tb][s];
            br.put(((e >> 8) << s) | value_bits(df, s), (e & 255) + s);
          } else {
            s_dc[c][b0 + i] = dc;
          }
          bits += encode_ac(row, s_ac[tb], pass != 0, br);
        }
      }
      if (pass) break;
      __syncthreads();
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {
        int prev = b0 ? s_dc[c][b0 - 1] : 0;
        for (int i = 0; i < 4; ++i) {
          const int dc = s_dc[c][b0 + i], s = bit_size(dc - prev);
          bits += (s_dcc[c != 0][s] & 255) + s;
          prev = dc;
        }
      }
      const int bit0 = block_scan_excl(bits, s_wave, total_bits);
      nbytes = (total_bits + 7) >> 3;
      nwords = (((total_bits + 31) >> 5) + 3) & ~3;               // words in fours: uint4 reads below
      int tl = threadIdx.x;                                        // taken afresh, as for the stuffing below
      asm volatile("" : "+v"(tl));
      for (int w = tl; w < nwords; w += 256) buf[w] = 0;
      __threadfence();
      __syncthreads();
      br.start(buf, bit0);
    }
    br.finish();
    if (threadIdx.x == 0 && (total_bits & 7)) {                    // one-bits up to the end of the last byte
      const int np = 8 - (total_bits & 7);
      atomicOr(buf + (total_bits >> 5), ((1u << np) - 1) << (32 - (total_bits & 31) - np));
    }
    __threadfence();                                               // the stuffing pass reads other lanes' words
    __syncthreads();

    // stuffing, as in jpeg_tile_kernel: bytes past nbytes are zero, so whole words can be counted.  The lane index is taken
    // afresh (the compiler would carry its multiples for this part through the twelve blocks above, and spill them)
    int tl = threadIdx.x;
    asm volatile("" : "+v"(tl));
    int ff = 0;
    for (int w = tl; w < nwords; w += 256) ff += count_ff(buf[w]);
    int nff;
    block_scan_excl(ff, s_wave, nff);
    const int out_bytes = nbytes + nff;
    if (tl == 0) need[t] = out_bytes;
    if (out_bytes <= slot_bytes) {
      uint8_t* o = slots + (size_t)t * slot_bytes;
      int before = 0;                                              // 0xFF bytes of the windows done
      for (int w0 = 0; w0 < nwords; w0 += 1024) {
        const int w = w0 + 4 * tl;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (w < nwords) v = *(const uint4*)(buf + w);
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
        int win;
        const int mine = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
        int pos = 4 * w + before + block_scan_excl(mine, s_wave, win);
        before += win;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if (4 * w + j < nbytes) {
            const uint32_t b = (vw[j >> 2] >> (24 - 8 * (j & 3))) & 255;
            o[pos++] = (uint8_t)b;
            if (b == 255) o[pos++] = 0;
          }
        }
      }
    }
    __syncthreads();                                               // s_dc and the rows are rewritten by the next tile
  }
}

constexpr size_t JPEG_Q2_BYTES = 1024;                         // the two quantisers at the start of the scratch, then the bit buffers
static_assert(sizeof(JpegQ2) <= JPEG_Q2_BYTES, "the quantisers outgrow their place in the scratch");
size_t jpeg_rgb_scratch_bytes(int ntiles) {
  return JPEG_Q2_BYTES + (size_t)(ntiles < JPEG_MAX_WGS ? ntiles : JPEG_MAX_WGS) * JPEG_WG_WORDS_RGB * sizeof(uint32_t);
}

hipError_t launch_jpeg_tiles_rgb(const RgbSrc& src, int quality, int tile0, int ntiles, uint32_t* scratch, uint8_t* slots,
                                 long slot_bytes, int32_t* need, uint8_t* packed, int64_t* offsets, hipStream_t s) {
  JpegQ2 q;
  q.t[0] = make_jpegq(quality, K1_LUMA);
  q.t[1] = make_jpegq(quality, K2_CHROMA);
  const int wgs = ntiles < JPEG_MAX_WGS ? ntiles : JPEG_MAX_WGS;
  JpegQ2* qdev = (JpegQ2*)scratch;
  jpeg_q2_kernel<<<dim3(1), dim3(64), 0, s>>>(q, qdev);
  jpeg_tile_rgb_kernel<<<dim3((unsigned)wgs), dim3(256), 0, s>>>(src, (src.W + 255) / 256, tile0, ntiles, qdev,
                                                                scratch + JPEG_Q2_BYTES / sizeof(uint32_t), slots, slot_bytes, need);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !packed) return e;
  jpeg_offsets_kernel<<<dim3(1), dim3(256), 0, s>>>(need, ntiles, slot_bytes, offsets);
  jpeg_compact_kernel<<<dim3((unsigned)ntiles, 4), dim3(256), 0, s>>>(slots, slot_bytes, need, offsets, packed);
  return hipGetLastError();
}

}  // namespace tmk

extern "C" int tm_jpeg_tables(int quality, void* buf, size_t cap, size_t* out_bytes) {
  if (quality < 1 || quality > 100) return tmk::fail(TM_ERR_ARG, "tm_jpeg_tables: quality %d outside 1 .. 100", quality);
  if (!buf && !out_bytes) return tmk::fail(TM_ERR_ARG, "tm_jpeg_tables: null buffer and null size");
  return tmk::jpeg_tables(quality, buf, cap, out_bytes);
}

extern "C" int tm_jpeg_tables_rgb(int quality, void* buf, size_t cap, size_t* out_bytes) {
  if (quality < 1 || quality > 100) return tmk::fail(TM_ERR_ARG, "tm_jpeg_tables_rgb: quality %d outside 1 .. 100", quality);
  if (!buf && !out_bytes) return tmk::fail(TM_ERR_ARG, "tm_jpeg_tables_rgb: null buffer and null size");
  return tmk::jpeg_tables_rgb(quality, buf, cap, out_bytes);
}

extern "C" int tm_u8_shrink2(const void* src, int H, int W, int64_t src_pitch, void* dst, int64_t dst_pitch, void* stream) {
  using namespace tmk;
  if (!src || !dst) return fail(TM_ERR_ARG, "tm_u8_shrink2: null source / destination");
  if (H < 1 || W < 1) return fail(TM_ERR_ARG, "tm_u8_shrink2: H and W must be positive, got %d x %d", H, W);
  if (src_pitch < W) return fail(TM_ERR_ARG, "tm_u8_shrink2: source pitch %lld below W %d", (long long)src_pitch, W);
  if (dst_pitch < (W + 1) / 2) return fail(TM_ERR_ARG, "tm_u8_shrink2: destination pitch %lld below ceil(W / 2) = %d", (long long)dst_pitch, (W + 1) / 2);
  HIP_TRY(launch_u8_shrink2((const uint8_t*)src, H, W, (long)src_pitch, (uint8_t*)dst, (long)dst_pitch, (hipStream_t)stream));
  return TM_OK;
}
