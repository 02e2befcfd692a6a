// Tile I/O either side of the denoising path.
//
//  * gene_tile_scatter: the COO transcript tile of utils/MBADataset_tst.py:65-91 (`_getgene`: gblk x gblk
//    block sum + z padding; `_pad_gn`: shift by the halo offset and crop to the gsz x gsz grid) and the
//    densification of model/unet_ours.py:301-306, as one scatter-add pass.  Counts are integers held in
//    fp32, so the atomic adds are exact and order independent (bit-exact against the oracle).
//  * blosc_decompress: decoder of the Blosc-1 frames that zarr 2.14.1 / numcodecs 0.15.0 (the reference's
//    pins, environment.yml:172,220) write by default for the per-step state tiles (test_brn.py:225
//    `zarr.save_array`): lz4 codec, byte shuffle.  Host code; restated from the published c-blosc 1.x
//    frame layout (16-byte header, bstarts, per-split streams) and the LZ4 block format.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/teramind_hip.h"
#include "tm_kernels.h"

namespace tmk {

// one thread per COO entry; grid-stride so that nnz up to 2^31 is covered with a bounded grid
__global__ __launch_bounds__(256) void gene_tile_scatter_kernel(const int32_t* __restrict__ crd, const float* __restrict__ dat,
                                                                long nnz, int gblk, int shift_h, int shift_w, int gsz,
                                                                int chan_in, int zpad_ch, float* __restrict__ out) {
  const long ch_out = (long)chan_in + 2L * zpad_ch;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (long)gridDim.x * blockDim.x) {
    const int h = crd[i], w = crd[nnz + i], c = crd[2 * nnz + i];
    if (h < 0 || w < 0 || c < 0 || c >= chan_in) continue;      // outside the declared shape: ignored, never written
    const int gh = h / gblk + shift_h, gw = w / gblk + shift_w;
    if (gh < 0 || gh >= gsz || gw < 0 || gw >= gsz) continue;   // _pad_gn crop
    atomicAdd(out + ((long)gh * gsz + gw) * ch_out + zpad_ch + c, dat[i]);
  }
}

hipError_t launch_gene_tile_scatter(const int32_t* crd, const float* dat, long nnz, int gblk, int shift_h, int shift_w,
                                    int gsz, int chan_in, int zpad_ch, float* out, hipStream_t s) {
  const size_t bytes = (size_t)gsz * gsz * ((size_t)chan_in + 2 * (size_t)zpad_ch) * sizeof(float);
  hipError_t e = hipMemsetAsync(out, 0, bytes, s);
  if (e != hipSuccess || nnz == 0) return e;
  long blocks = (nnz + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  gene_tile_scatter_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(crd, dat, nnz, gblk, shift_h, shift_w, gsz, chan_in,
                                                                       zpad_ch, out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Training batches from resident tiles (utils/MBADataset.py:69-170 + experiment.py:129).
//
// z geometry shared by both kernels (MBADataset.py:36,111): spad padded slices each side, the image keeps the window's
// middle snum - 2 * shf slices
struct TrainZ { int spad, shf, nz; };
static inline bool train_z(int snum, TrainZ* z) {
  switch (snum) {
    case 1: *z = {0, 0, 1}; return true;
    case 4: *z = {1, 1, 2}; return true;
    case 8: *z = {1, 2, 4}; return true;
    case 16: *z = {3, 4, 8}; return true;
  }
  return false;
}

// images: one thread per output pixel, x fastest, so that a wave stores 64 consecutive floats whatever rot / flip; the loads
// walk a source row (even rot) or a source column (odd rot)
template <typename T>
__device__ inline float px_to_float(T v);
template <>
__device__ inline float px_to_float<uint8_t>(uint8_t v) { return (float)v; }
template <>
__device__ inline float px_to_float<__half>(__half v) { return __half2float(v); }

template <typename T>
__global__ __launch_bounds__(256) void train_images_kernel(const T* __restrict__ img, int n_tiles, int zt, int H, int W,
                                                           const tm_train_sample* __restrict__ desc, int sdim, int nz, int spad,
                                                           int shf, int stain, float* __restrict__ out) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= sdim * sdim) return;
  const int y = pix / sdim, x = pix - y * sdim, c = blockIdx.y, b = blockIdx.z;
  const tm_train_sample d = desc[b];
  // the host mirror was validated before the launch; a device copy that disagrees with it must still not read out of bounds
  if (d.tile < 0 || d.tile >= n_tiles || d.top < 0 || d.top > H - sdim || d.left < 0 || d.left > W - sdim) return;
  // out = hflip(rot90(crop, rot)):  undo the flip, then the quarter turns
  const int j = d.flip ? sdim - 1 - x : x, e = sdim - 1;
  int sy, sx;
  switch (d.rot & 3) {
    case 0: sy = y; sx = j; break;
    case 1: sy = j; sx = e - y; break;
    case 2: sy = e - y; sx = e - j; break;
    default: sy = e - j; sx = y; break;
  }
  const int s = stain == 0 ? c / nz : stain - 1;
  const int z = d.snm + shf + (c % nz) - spad;                      // slice of the unpadded stack
  float v = 0.0f;                                                   // the zero-padded slices
  if (z >= 0 && z < zt) v = px_to_float<T>(img[(((size_t)d.tile * 2 + s) * zt + z) * H * W + (size_t)(d.top + sy) * W + d.left + sx]);
  out[(((size_t)b * gridDim.y + c) * sdim + y) * sdim + x] = __fsub_rn(__fdiv_rn(v, 127.5f), 1.0f);   // true division: torch's bits
}

// genes: a sample reads only its tile's entries of rows [top, top + sdim) (the entries are ordered by row, row_start holds the
// first entry of each row); blockIdx.y = sample, grid-stride over that range
__global__ __launch_bounds__(256) void train_genes_kernel(const int32_t* __restrict__ crd, const float* __restrict__ dat, long nnz,
                                                          const int64_t* __restrict__ tile_base, const int32_t* __restrict__ row_start,
                                                          int n_tiles, int H, int chan_in, const tm_train_sample* __restrict__ desc, int sdim,
                                                          int gblk, int pdim, int snum, int spad, float* __restrict__ out) {
  const int b = blockIdx.y;
  const tm_train_sample d = desc[b];
  if (d.tile < 0 || d.tile >= n_tiles || d.top < 0 || d.top > H - sdim) return;          // see train_images_kernel
  const int gs = sdim / gblk, gp = gs + 2 * pdim, ch = snum * 500;
  const long base = tile_base[d.tile] < 0 ? 0 : tile_base[d.tile];
  const long end_t = tile_base[d.tile + 1] < nnz ? tile_base[d.tile + 1] : nnz;
  const int32_t* rs = row_start + (size_t)d.tile * (H + 1);
  const long r0 = rs[d.top] < 0 ? 0 : rs[d.top], r1 = rs[d.top + sdim];
  const long i0 = base + r0, i1 = base + r1 < end_t ? base + r1 : end_t;
  float* o = out + (size_t)b * gp * gp * ch;
  for (long i = i0 + (long)blockIdx.x * 256 + threadIdx.x; i < i1; i += (long)gridDim.x * 256) {
    const int h = crd[i] - d.top, w = crd[nnz + i] - d.left, c0 = crd[2 * nnz + i];
    if (h < 0 || h >= sdim || w < 0 || w >= sdim || c0 < 0 || c0 >= chan_in) continue;   // outside the crop / declared shape
    const int c = c0 + (spad - d.snm) * 500;                                              // z pad, then the slice window
    if (c < 0 || c >= ch) continue;
    int gh = h / gblk, gw = w / gblk;
    for (int r = 0; r < (d.rot & 3); ++r) {                          // transpose, then reverse h (MBADataset.py:158-161)
      const int t = gh;
      gh = gs - 1 - gw;
      gw = t;
    }
    if (d.flip) gw = gs - 1 - gw;
    atomicAdd(o + ((size_t)(gh + pdim) * gp + gw + pdim) * ch + c, dat[i]);
  }
}

static int check_train_desc(const char* fn, const tm_train_sample* desc, const tm_train_sample* desc_host, int B, int n_tiles, int zt,
                            int H, int W, int sdim, int snum, TrainZ* z) {
  if (!desc || !desc_host) return fail(TM_ERR_ARG, "%s: null sample descriptors (device array and its host mirror)", fn);
  if (B < 1 || B > 65535) return fail(TM_ERR_ARG, "%s: batch %d outside [1, 65535]", fn, B);
  if (n_tiles < 1 || zt < 1 || H < 1 || W < 1) return fail(TM_ERR_ARG, "%s: bad tile geometry", fn);
  if (!train_z(snum, z)) return fail(TM_ERR_ARG, "%s: snum must be 1, 4, 8 or 16 (MBADataset.py:30), got %d", fn, snum);
  if (sdim < 1 || sdim > H || sdim > W) return fail(TM_ERR_ARG, "%s: sdim %d does not fit the %d x %d tile", fn, sdim, H, W);
  const int snm_max = zt + 2 * z->spad - snum;
  if (snm_max < 0) return fail(TM_ERR_ARG, "%s: %d slices (+ %d padded each side) are fewer than snum %d", fn, zt, z->spad, snum);
  for (int b = 0; b < B; ++b) {
    const tm_train_sample& d = desc_host[b];
    if (d.tile < 0 || d.tile >= n_tiles) return fail(TM_ERR_ARG, "%s: sample %d: tile %d outside [0, %d)", fn, b, d.tile, n_tiles);
    if (d.top < 0 || d.top > H - sdim || d.left < 0 || d.left > W - sdim)
      return fail(TM_ERR_ARG, "%s: sample %d: crop (%d, %d) + %d outside the %d x %d tile", fn, b, d.top, d.left, sdim, H, W);
    if (d.snm < 0 || d.snm > snm_max) return fail(TM_ERR_ARG, "%s: sample %d: snm %d outside [0, %d]", fn, b, d.snm, snm_max);
    if (d.rot < 0 || d.rot > 3) return fail(TM_ERR_ARG, "%s: sample %d: rot %d outside [0, 3]", fn, b, d.rot);
    if (d.flip < 0 || d.flip > 1) return fail(TM_ERR_ARG, "%s: sample %d: flip %d is not 0 or 1", fn, b, d.flip);
  }
  return TM_OK;
}

}  // namespace tmk

extern "C" int tm_train_batch_images(const void* img, int img_dtype, int n_tiles, int zt, int H, int W, const tm_train_sample* desc,
                                     const tm_train_sample* desc_host, int B, int sdim, int snum, int stain, void* out, void* stream) {
  using namespace tmk;
  const char* fn = "tm_train_batch_images";
  if (!img || !out) return fail(TM_ERR_ARG, "%s: null image / output pointer", fn);
  if (img_dtype != 0 && img_dtype != 1) return fail(TM_ERR_ARG, "%s: img_dtype must be 0 (uint8) or 1 (float16)", fn);
  if (stain < 0 || stain > 2) return fail(TM_ERR_ARG, "%s: stain must be 0 (all), 1 (DAPI) or 2 (PolyT)", fn);
  TrainZ z;
  const int rc = check_train_desc(fn, desc, desc_host, B, n_tiles, zt, H, W, sdim, snum, &z);
  if (rc != TM_OK) return rc;
  const int C = (stain == 0 ? 2 : 1) * z.nz;
  const dim3 grid((unsigned)(((long)sdim * sdim + 255) / 256), (unsigned)C, (unsigned)B);
  if (img_dtype == 0)
    train_images_kernel<uint8_t><<<grid, dim3(256), 0, (hipStream_t)stream>>>((const uint8_t*)img, n_tiles, zt, H, W, desc, sdim, z.nz, z.spad,
                                                                               z.shf, stain, (float*)out);
  else
    train_images_kernel<__half><<<grid, dim3(256), 0, (hipStream_t)stream>>>((const __half*)img, n_tiles, zt, H, W, desc, sdim, z.nz, z.spad,
                                                                              z.shf, stain, (float*)out);
  HIP_TRY(hipGetLastError());
  return TM_OK;
}

extern "C" int tm_train_batch_genes(const int32_t* crd, const void* dat, int64_t nnz, const int64_t* tile_base, const int32_t* row_start,
                                    int n_tiles, int zt, int H, int W, const tm_train_sample* desc, const tm_train_sample* desc_host,
                                    int B, int sdim, int gblk, int pdim, int snum, void* out, void* stream) {
  using namespace tmk;
  const char* fn = "tm_train_batch_genes";
  if (!out || !tile_base || !row_start || nnz < 0 || (nnz > 0 && (!crd || !dat)))
    return fail(TM_ERR_ARG, "%s: null pointer / negative entry count", fn);
  if (gblk != 8 && gblk != 16 && gblk != 32) return fail(TM_ERR_ARG, "%s: gblk must be 8, 16 or 32 (config_parm.py:47), got %d", fn, gblk);
  if (pdim < 0) return fail(TM_ERR_ARG, "%s: negative pdim", fn);
  if (sdim % gblk) return fail(TM_ERR_ARG, "%s: sdim %d is not a multiple of gblk %d", fn, sdim, gblk);
  TrainZ z;
  const int rc = check_train_desc(fn, desc, desc_host, B, n_tiles, zt, H, W, sdim, snum, &z);
  if (rc != TM_OK) return rc;
  const size_t gp = (size_t)(sdim / gblk + 2 * pdim);
  HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * gp * gp * snum * 500 * sizeof(float), (hipStream_t)stream));
  if (nnz == 0) return TM_OK;
  // 64 workgroups per sample cover the ~1e5 entries of a 256-row band of a brain tile in a few strides
  train_genes_kernel<<<dim3(64, (unsigned)B), dim3(256), 0, (hipStream_t)stream>>>(crd, (const float*)dat, (long)nnz, tile_base, row_start,
                                                                                  n_tiles, H, zt * 500, desc, sdim, gblk, pdim, snum, z.spad,
                                                                                  (float*)out);
  HIP_TRY(hipGetLastError());
  return TM_OK;
}

namespace tmk {

// ------------------------------------------------------------------------------------------
// LZ4 block format: sequences of [token][literal length ext][literals][offset LE16][match length ext].
// Returns the number of bytes written, or -1 on malformed input / overflow of `cap`.
static long lz4_block_decode(const uint8_t* src, long n, uint8_t* dst, long cap) {
  long ip = 0, op = 0;
  while (ip < n) {
    const unsigned tok = src[ip++];
    long lit = tok >> 4;
    if (lit == 15) {
      unsigned b;
      do {
        if (ip >= n) return -1;
        b = src[ip++];
        lit += b;
      } while (b == 255);
    }
    if (ip + lit > n || op + lit > cap) return -1;
    memcpy(dst + op, src + ip, (size_t)lit);
    ip += lit;
    op += lit;
    if (ip >= n) break;                       // the last sequence carries literals only
    if (ip + 2 > n) return -1;
    const long off = src[ip] | (src[ip + 1] << 8);
    ip += 2;
    if (off == 0 || off > op) return -1;
    long ml = (tok & 15);
    if (ml == 15) {
      unsigned b;
      do {
        if (ip >= n) return -1;
        b = src[ip++];
        ml += b;
      } while (b == 255);
    }
    ml += 4;
    if (op + ml > cap) return -1;
    for (long k = 0; k < ml; ++k) dst[op + k] = dst[op + k - off];      // overlapping copies are the RLE case
    op += ml;
  }
  return op;
}

static inline uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

enum { BLOSC_SHUFFLE = 1, BLOSC_MEMCPYED = 2, BLOSC_BITSHUFFLE = 4, BLOSC_DONT_SPLIT = 16 };
static const int BLOSC_MAX_SPLITS = 16, BLOSC_MIN_BUFFERSIZE = 128, BLOSC_HEADER = 16;

int blosc_decompress(const void* src_, size_t src_bytes, void* dst_, size_t dst_cap, size_t* out_bytes) {
  const uint8_t* src = (const uint8_t*)src_;
  uint8_t* dst = (uint8_t*)dst_;
  if (!src || src_bytes < (size_t)BLOSC_HEADER) return fail(TM_ERR_ARG, "blosc: frame shorter than its header");
  const unsigned flags = src[2];
  const long typesize = src[3] ? src[3] : 1;
  const long nbytes = le32(src + 4), blocksize = le32(src + 8), cbytes = le32(src + 12);
  if (out_bytes) *out_bytes = (size_t)nbytes;
  if (!dst) return TM_OK;                                        // size query
  if ((size_t)cbytes > src_bytes) return fail(TM_ERR_ARG, "blosc: frame truncated");
  if ((size_t)nbytes > dst_cap) return fail(TM_ERR_ARG, "blosc: destination too small");
  if (nbytes == 0) return TM_OK;
  if (flags & BLOSC_MEMCPYED) {
    if (cbytes < BLOSC_HEADER + nbytes) return fail(TM_ERR_ARG, "blosc: memcpyed frame truncated");
    memcpy(dst, src + BLOSC_HEADER, (size_t)nbytes);
    return TM_OK;
  }
  if (flags & BLOSC_BITSHUFFLE) return fail(TM_ERR_ARG, "blosc: bit-shuffled frames are not supported (zarr default is byte shuffle)");
  const int codec = (flags >> 5) & 7;
  if (codec != 1) return fail(TM_ERR_ARG, "blosc: only the lz4 codec is supported (zarr/numcodecs default)");
  if (blocksize <= 0) return fail(TM_ERR_ARG, "blosc: bad block size");
  const long nblocks = (nbytes + blocksize - 1) / blocksize, leftover = nbytes % blocksize;
  if (BLOSC_HEADER + 4 * nblocks > cbytes) return fail(TM_ERR_ARG, "blosc: block table truncated");
  std::vector<uint8_t> tmp((size_t)blocksize);
  const bool shuffled = (flags & BLOSC_SHUFFLE) && typesize > 1;
  for (long j = 0; j < nblocks; ++j) {
    const bool last_short = (j == nblocks - 1) && leftover > 0;
    const long bsize = last_short ? leftover : blocksize;
    long nsplits = 1;
    if (!(flags & BLOSC_DONT_SPLIT) && typesize <= BLOSC_MAX_SPLITS && bsize / typesize >= BLOSC_MIN_BUFFERSIZE && !last_short)
      nsplits = typesize;
    const long neblock = bsize / nsplits;
    long ip = le32(src + BLOSC_HEADER + 4 * j);
    uint8_t* o = shuffled ? tmp.data() : dst + j * blocksize;
    long done = 0;
    for (long sp = 0; sp < nsplits; ++sp) {
      if (ip + 4 > cbytes) return fail(TM_ERR_ARG, "blosc: split header out of range");
      const long cb = le32(src + ip);
      ip += 4;
      if (cb < 0 || ip + cb > cbytes) return fail(TM_ERR_ARG, "blosc: split out of range");
      if (cb == neblock) {
        memcpy(o + done, src + ip, (size_t)neblock);
      } else if (lz4_block_decode(src + ip, cb, o + done, neblock) != neblock) {
        return fail(TM_ERR_ARG, "blosc: lz4 stream does not decode to the split size");
      }
      ip += cb;
      done += neblock;
    }
    if (done != bsize) return fail(TM_ERR_ARG, "blosc: block size mismatch");
    if (shuffled) {
      uint8_t* d = dst + j * blocksize;
      const long nel = bsize / typesize, rem = bsize - nel * typesize;
      for (long k = 0; k < typesize; ++k) {
        const uint8_t* s = tmp.data() + k * nel;
        for (long i = 0; i < nel; ++i) d[i * typesize + k] = s[i];
      }
      memcpy(d + nel * typesize, tmp.data() + nel * typesize, (size_t)rem);
    }
  }
  return TM_OK;
}

}  // namespace tmk
