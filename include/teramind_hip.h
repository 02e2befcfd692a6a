/* teramind_hip.h -- C ABI of libteramind_hip.so (MI355X / gfx950 only).
 *
 * The reference (CTPLab/Tera-MIND) has no FFI / plugin interface for this path: its hot
 * path is stock PyTorch modules.  This ABI is what a binding for the path would attach to;
 * each entry point cites the reference interface it replaces (paths relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers owned by the caller (PyTorch-ROCm
 *     allocations); the library borrows them for the duration of the enqueue and never
 *     frees or allocates caller-visible memory.  The only library-owned device memory is
 *     the packed weight arena (freed by tm_model_destroy); the single-operator entry points
 *     below keep call-local scratch of their own.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no hidden
 *     device synchronisation, no internal threads.  One host thread per model.  (The
 *     single-operator entry points below are the exception: see their section.)
 *   - return value: 0 = OK, negative = TM_ERR_*; text via tm_last_error() (thread local).
 *     No C++ exception crosses the ABI.
 *   - image-like tensors are fp32, contiguous, NCHW as in the reference ("b (s z) h w").
 */
#ifndef TERAMIND_HIP_H
#define TERAMIND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TM_ABI_VERSION 1

enum {
  TM_OK = 0,
  TM_ERR_ARG = -1,        /* bad argument / unsupported configuration */
  TM_ERR_STATE = -2,      /* call order violated (e.g. forward before finalize) */
  TM_ERR_KEY = -3,        /* unknown / duplicate / missing state_dict key, or shape mismatch */
  TM_ERR_HIP = -4,        /* a HIP runtime call failed */
  TM_ERR_WORKSPACE = -5   /* workspace too small */
};

/* TM_DTYPE_F32: every kernel computes in fp32 (exact-fp32 MFMA).  TM_DTYPE_BF16: the 3x3x3 convs
 * (95 % of the FLOPs) take bf16 weights and bf16 normalised/activated inputs on the bf16 MFMA with
 * fp32 accumulation; the residual stream, norms, attention and everything else stay fp32.
 * TM_DTYPE_F16: the same kernels with IEEE-half operands -- the arithmetic the reference runs on GPUs
 * (autocast('cuda', fp16), diffusion/base.py:377): same speed as bf16, 3 more mantissa bits, fp16 range.
 * Parameters are always loaded as fp32 and rounded (RNE) when packed. */
enum { TM_DTYPE_F32 = 0, TM_DTYPE_BF16 = 1, TM_DTYPE_F16 = 2 };
enum { TM_SAMPLE_DDPM = 0, TM_SAMPLE_DDIM = 1 };

/* Model configuration.  Replaces BeatGANsUNetConfig as filled by
 * TrainConfig.make_model_conf (config.py:280-326) from prep_config_parm (config_parm.py:5-59). */
typedef struct tm_config {
  int32_t patch_size;     /* image_size / patch_size: 32 | 64 | 128 (config_parm.py:47-55; 64 = the published checkpoint) */
  int32_t rna_slc;        /* len(rna_tpl): 1 | 4 | 8 | 16 (train.py:24-26) -> z_size = ceil(rna_slc/2); gn^2 * rna_slc <= 512 */
  int32_t n_stain;        /* 2 for stain='all', else 1 */
  int32_t rna_num;        /* 229 */
  int32_t net_ch;         /* model_channels: 64 */
  int32_t ch_mult[4];     /* (1,2,4,8) */
  int32_t embed_ch;       /* embed_channels: 512 */
  int32_t attn_res;       /* attention_resolutions[0]: 16 */
  int32_t num_res_blocks; /* 2 */
  int32_t vis_only;       /* 1: attention-map model (model/unet_attn.py), time_embed + rna_blocks[0] */
  int32_t dtype;          /* TM_DTYPE_F32 | TM_DTYPE_BF16 | TM_DTYPE_F16 (operand type of the convs / Linears / attention) */
} tm_config;

typedef struct tm_model tm_model;

int tm_version(void);
const char* tm_last_error(void);

/* Replaces BeatGANsUNetConfig.make_model() (model/unet_ours.py:78-79,82-275). */
int tm_model_create(const tm_config* cfg, tm_model** out);

/* Replaces model.load_state_dict(state_dct, strict=True) (test_brn.py:140-147), one tensor
 * at a time: `ref_key` is the reference state_dict key (after stripping 'model.'),
 * `host_ptr` a contiguous fp32 HOST tensor of `shape[ndim]`. */
int tm_model_load_param(tm_model* m, const char* ref_key, const void* host_ptr,
                        const int64_t* shape, int ndim, int dtype);

/* strict=True check (every key present), packs / pads / reorders into the device arena
 * (replaces `.to(gpu_id)`, test_brn.py:148).  After this the weights are immutable. */
int tm_model_finalize(tm_model* m);

/* Number of keys the model expects / i-th key (for diagnostics and tests). */
int tm_model_num_params(const tm_model* m);
const char* tm_model_param_key(const tm_model* m, int i);

/* Size of the arena in bytes (after finalize) and raw device pointer: lets the host
 * broadcast rank 0's packed weights over RCCL instead of re-reading the checkpoint on
 * every rank (replaces DDP's construction-time parameter broadcast, test_brn.py:149). */
size_t tm_model_arena_bytes(const tm_model* m);
void* tm_model_arena_ptr(tm_model* m);

/* Workspace (activations, RNA pyramid, skips) needed by tm_unet_forward for
 * `b` images of (p1-1)x(p2-1) interior patches, i.e. b*p1*p2 encoder patches. */
size_t tm_workspace_bytes(const tm_model* m, int b, int p1, int p2, int want_pred2);

/* Replaces BeatGANsUNetModel.forward (model/unet_ours.py:343-426) as called through
 * _WrappedModel.forward (diffusion/diffusion.py:134-154):
 *   x         [b*p1*p2, C, ps, ps] fp32        (C = n_stain*z_size)
 *   t         [b] int64, ORIGINAL-scale timesteps (already mapped by timestep_map)
 *   rna_dense [b*p1*p2, gn, gn, rna_slc*500] fp32 (dense, as test_brn.py:180-181 builds it)
 *   p1, p2    patches per image side including the half-patch padding (= H/ps + 1)
 *   pred      [b*(p1-1)*(p2-1), C, ps, ps]     collage ("o==0") decoder output
 *   pred2     NULL, or [b*p1*p2, C, ps, ps]    original-patch ("o==1") decoder output
 */
int tm_unet_forward(tm_model* m, const void* x, const int64_t* t, const void* rna_dense,
                    int b, int p1, int p2, void* pred, void* pred2_or_null,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The RNA conditioning of a forward (BeatGANsUNetModel.get_rna, model/unet_ours.py:298-323: gene-gene attention block,
 * down_z, the three pyramid convs) depends on the genes only -- not on x or t.  A caller that runs many diffusion steps on
 * the same genes (mode A: LitModel.gen_sample's reverse loop, experiment.py:325-330; the reference recomputes it in every
 * step) computes it ONCE into a buffer of its own and hands it to every step:
 *   tm_rna_pyramid_bytes   size of that buffer for (b, p1, p2)
 *   tm_rna_pyramid         rna_dense [b*p1*p2, gn, gn, rna_slc*500] fp32 -> pyramid (opaque; valid for this model, b, p1, p2)
 *   tm_unet_forward_rna    tm_unet_forward with the precomputed pyramid in place of rna_dense; bit-identical results.
 * The buffer also holds what every AttnBlock derives from its pyramid level and its weights alone (MBAblocks.py:484-489:
 * the 7C adaLN tensor Linear(SiLU(cond)) and k / v = Linear(cross-cond chunk), 9C values per conditioning voxel) for the
 * blocks of the encoder, the middle and the `pred` decoder, so that a step runs neither those Linears nor SiLU(cond); the
 * `pred2` decoder pass computes its own.  With the checkpoint configuration that is 2.8 MiB per encoder patch and 3.4 MiB
 * per interior patch in fp32 (half of it in the 16-bit modes), about as much again as the levels: sized for a sampler's
 * batch, not for a sweep (tm_unet_forward and tm_unet_forward_level0 compute this part inside each step).
 * The pyramid buffer is only read by tm_unet_forward_rna and may be shared by any number of steps. */
size_t tm_rna_pyramid_bytes(const tm_model* m, int b, int p1, int p2);
int tm_rna_pyramid(tm_model* m, const void* rna_dense, int b, int p1, int p2, void* pyramid, size_t pyramid_bytes,
                   void* stream);
int tm_unet_forward_rna(tm_model* m, const void* x, const int64_t* t, const void* pyramid, size_t pyramid_bytes,
                        int b, int p1, int p2, void* pred, void* pred2_or_null, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The tile sweep (mode B, test_brn.py:232-255) also recomputes the conditioning of the SAME genes at each of its T diffusion
 * steps, but the whole pyramid of a tile (~1 MB per patch) is too large to keep for every tile.  Level 0 -- gene-gene
 * attention -> down_z -> Upsample (model/unet_ours.py:298-310, MBAblocks.py:472-479), the part that reads the gene counts and
 * costs most -- is 59 KB per patch: a caller may keep it per tile / window and skip that part (and the dense gene tensor)
 * from the second step on:
 *   tm_rna_level0_bytes     size of the level-0 tensor for (b, p1, p2) (the activation-stream type of the model: fp32 or 16-bit)
 *   tm_rna_level0           rna_dense -> level0 (16-byte aligned device buffer); workspace >= tm_workspace_bytes(.., 0)
 *   tm_unet_forward_level0  tm_unet_forward with level0 in place of rna_dense; bit-identical results. */
size_t tm_rna_level0_bytes(const tm_model* m, int b, int p1, int p2);
int tm_rna_level0(tm_model* m, const void* rna_dense, int b, int p1, int p2, void* level0, size_t level0_bytes,
                  void* workspace, size_t workspace_bytes, void* stream);
int tm_unet_forward_level0(tm_model* m, const void* x, const int64_t* t, const void* level0, size_t level0_bytes,
                           int b, int p1, int p2, void* pred, void* pred2_or_null, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Per-step scalar coefficients: the float64 tables of GaussianDiffusionBeatGans.__init__
 * (diffusion/base.py:64-109) gathered at index i and cast `.float()` (base.py:643) by
 * the host. */
typedef struct tm_step_coefs {
  float sqrt_recip_alphas_cumprod;     /* base.py:89  */
  float sqrt_recipm1_alphas_cumprod;   /* base.py:90  */
  float posterior_mean_coef1;          /* base.py:100 */
  float posterior_mean_coef2;          /* base.py:103 */
  float sigma;                         /* DDPM: exp(0.5*log_variance) (base.py:479-480), 0 when t==0 */
  float sqrt_alpha_bar_prev;           /* DDIM: sqrt(alpha_bar_prev)      (base.py:492) */
  float sqrt_one_minus_alpha_bar_prev; /* DDIM: sqrt(1 - alpha_bar_prev)  (base.py:493, eta=0) */
} tm_step_coefs;

/* Replaces p_mean_variance's eps re-tiling + x0 / clamp / posterior mean
 * (diffusion/base.py:386-393,423-427), ddm_sample's DDPM / DDIM(eta=0) update (:476-498) and
 * the un-patchify + crop of ddm_sample_loop_progressive (:627-628):
 *   x_patches [b*(P1+1)*(P2+1), C, ps, ps]; eps [b*P1*P2, C, ps, ps] (model pred);
 *   noise     NULL or like x_patches (DDPM);  x_prev_img [b, C, P1*ps, P2*ps]. */
int tm_sampler_step(const tm_step_coefs* coefs, const void* x_patches, const void* eps,
                    const void* noise_or_null, void* x_prev_img, int b, int P1, int P2, int C,
                    int ps, int mode, void* stream);

/* Replaces F.pad(img, halfp) + rearrange(im2tl) (diffusion/base.py:606-607):
 *   img [b, C, P1*ps, P2*ps] -> patches [b*(P1+1)*(P2+1), C, ps, ps], zero border. */
int tm_pad_patchify(const void* img, void* patches, int b, int C, int P1, int P2, int ps,
                    float pad_value, void* stream);

/* Replaces unet_attn.BeatGANsUNetModel.get_rna (model/unet_attn.py:143-173):
 *   rna_dense [B, gn, gn, rna_slc*500] -> attn_out [4, B, G, G] fp32 softmax maps
 *   (3 slice-pair-masked + 1 unmasked), rna_mid [B, G, rna_slc-2, gn, gn]. */
size_t tm_gene_attn_workspace_bytes(const tm_model* m, int B);
int tm_gene_attn(tm_model* m, const void* rna_dense, int B, void* attn_out, void* rna_mid,
                 void* workspace, size_t workspace_bytes, void* stream);

/* The pathway read-out of the attention driver (test_attn.py:404-423) without the maps:
 *   rna_dense [B, gn, gn, 4*500], glst = K host gene indices (1 <= K <= 8, distinct, each in [0, rna_num)) ->
 *   out [B, 4K, 2*gn*gn] fp32: rows (map 0 | map 1) x middle slice 0 and (map 1 | map 2) x middle slice 1 side by side,
 *       then map 3 x both middle slices, then the raw counts of the K genes;
 *   sub [4, B, K, K] fp32 (optional, may be NULL): the K x K blocks attn[:, :, glst][..., glst] of tm_gene_attn's maps.
 * For the checkpoint geometry (gn^2 * 4 = 64 features, rna_num <= 232) one fused kernel computes only the K query rows of the
 * logits and no G x G map is written: the workspace is 256 bytes whatever B.  Every other rna_slc = 4 configuration runs the
 * map kernels over chunks of 8 patches into the workspace (bounded independently of B) and gathers from there. */
size_t tm_gene_attn_readout_workspace_bytes(const tm_model* m, int B, int K);
int tm_gene_attn_readout(tm_model* m, const void* rna_dense, int B, const int* glst, int K, void* out, void* sub,
                         void* workspace, size_t workspace_bytes, void* stream);

int tm_model_destroy(tm_model* m);

/* ---- tile I/O either side of the path ----------------------------
 * tm_gene_tile_dense replaces MBADataset_tst._getgene + _pad_gn (utils/MBADataset_tst.py:65-91) and the
 * sparse->dense step of BeatGANsUNetModel.get_rna (model/unet_ours.py:301-306) for one gene tile:
 *   crd  int32 [3][nnz] device: (h, w, channel) of the tile's COO transcript counts, h/w in pixels of the
 *        +-128-px padded ROI, channel = slice*500 + gene;   dat fp32 [nnz] device: counts
 *   out  fp32 [gsz][gsz][chan_in + 2*zpad_ch] device: out[h/gblk + shift_h][w/gblk + shift_w][zpad_ch + c] += dat
 *        for every entry whose cell lands inside the gsz x gsz grid; everything else is zero.
 * The reference values are gblk=16, shift = pad/gblk - (roi - roio)/gblk = -6, gsz=20, chan_in=25000,
 * zpad_ch = Z_PAD[rna_slc]*500.  Counts are integers, so the result is independent of the order of the adds. */
int tm_gene_tile_dense(const int32_t* crd, const void* dat, int64_t nnz, int gblk, int shift_h, int shift_w,
                       int gsz, int chan_in, int zpad_ch, void* out, void* stream);

/* ---- training batches from resident tiles (utils/MBADataset.py:69-170, experiment.py:129) ----
 * One descriptor per sample: the tile it is cut from, the crop corner in pixels, the first slice of its z window (in slices
 * of the stack padded by spad = {1:0, 4:1, 8:1, 16:3}[snum] each side), `rot` quarter turns (0..3) and `flip` (0 / 1).
 * Both calls take the descriptors twice: `desc` is the device array the kernels read, `desc_host` the same values in host
 * memory, checked (tile index, crop inside the tile, snm, rot, flip ranges) before anything is launched.  Both are
 * asynchronous on `stream` and return TM_ERR_ARG with a tm_last_error() text on a bad argument.  n_tiles tiles of
 * [H, W] pixels and zt slices (50 in the data). */
typedef struct tm_train_sample {
  int32_t tile, top, left, snm, rot, flip;
} tm_train_sample;

/* MBADataset._getimg + the image half of _trans + `im / 127.5 - 1`:
 *   img  uint8 (img_dtype 0) or float16 (1), device, [n_tiles][2 * zt][H][W], channel order (stain, z)
 *   out  fp32 [B][C][sdim][sdim], C = (stain == 0 ? 2 : 1) * nz, nz = snum - 2 * (snum / 4) for snum > 1, 1 for snum = 1
 *   stain 0 = all, 1 = DAPI, 2 = PolyT.   out = hflip^flip(rot90^rot(window of the crop)) / 127.5 - 1, the division a
 *   correctly rounded fp32 division (bit-equal to torch); slices that fall in the z padding are 0 before scaling. */
int tm_train_batch_images(const void* img, int img_dtype, int n_tiles, int zt, int H, int W, const tm_train_sample* desc,
                          const tm_train_sample* desc_host, int B, int sdim, int snum, int stain, void* out, void* stream);

/* MBADataset._getgene + the gene half of _trans + _to_sparse(pad = pdim) + sparse_coo_tensor(...).to_dense():
 *   crd  int32 [3][nnz] device: (h, w, slice * 500 + gene) of ALL tiles' COO entries, tile after tile, each tile's entries
 *        ordered by h;   dat fp32 [nnz] device: counts
 *   tile_base  int64 [n_tiles + 1] device: first entry of each tile;   row_start int32 [n_tiles][H + 1] device: first
 *        entry of each pixel row, relative to the tile's base (so a sample reads rows [top, top + sdim) only)
 *   out  fp32 [B][gs + 2 pdim][gs + 2 pdim][snum * 500], gs = sdim / gblk: zero-filled by the call, then one atomic add per
 *        entry inside the crop and the slice window.  Counts are integers: the result does not depend on the add order. */
int tm_train_batch_genes(const int32_t* crd, const void* dat, int64_t nnz, const int64_t* tile_base, const int32_t* row_start,
                         int n_tiles, int zt, int H, int W, const tm_train_sample* desc, const tm_train_sample* desc_host,
                         int B, int sdim, int gblk, int pdim, int snum, void* out, void* stream);

/* Host-side decoder of one Blosc-1 frame (lz4 codec, optional byte shuffle): the chunk encoding zarr 2.14.1 /
 * numcodecs 0.15.0 use by default for the state tiles the reference writes with zarr.save_array
 * (test_brn.py:225) and reads back with zarr.load (utils/MBADataset_tst.py:60, infer_brn.py:76).
 * dst == NULL: only *out_bytes (the decoded size) is set.  No GPU involved. */
int tm_blosc_decompress(const void* src, size_t src_bytes, void* dst, size_t dst_cap, size_t* out_bytes);

/* ---- Blosc-lz4 encoder: the frames tm_blosc_decompress reads, written on the GPU ----------------------------------
 * What zarr.save_array (test_brn.py:225) gives a state tile by default: Blosc-1, lz4 codec, byte shuffle.
 *   header   [2][1][flags][typesize][nbytes LE32][blocksize LE32][cbytes LE32]; flags = 0x20 (lz4) | 0x01 (byte shuffle,
 *            typesize > 1) | 0x10 (blocks not split); never 0x02 (memcpyed) or 0x04 (bit shuffle)
 *   blocks   of min(blocksize, nbytes) bytes (rounded down to whole elements above one element); bstarts int32 [nblocks]
 *            after the header; a block of >= 128 elements is split into `typesize` streams, a shorter one and the short last
 *            block are one stream (whole elements shuffled, the odd bytes after them); a stream is an LE32 length and its bytes
 *   streams  strict LZ4 blocks (what LZ4_decompress_safe accepts: minimum match 4, the last 5 bytes literals, the last match
 *            starts >= 12 bytes before the end), always SHORTER than the plain stream: one that would not be is stored, and
 *            length == plain size is how a decoder tells.  Offsets are <= 65535 because a stream is <= 65536 bytes.
 * Two calls on the same input give the same bytes: nothing depends on the CU count or on the order waves run in.  Pinned:
 * the frames decode (tm_blosc_decompress, and a strict decoder in the tests), the header fields equal c-blosc's for the same
 * arguments, and frames are within 15 % of c-blosc 1.21 (clevel 5) on recorded buffers.  Not pinned: byte equality with c-blosc.
 * Accepted: nbytes >= 1 (and a bound below 2^31), typesize 1, 2 or 4, blocksize a multiple of 4 in [256, 65536]; anything else
 * is TM_ERR_ARG with a text, before any device call.
 *
 * tm_blosc_bound: the largest frame the arguments can give, 16 + 4 nblocks + 4 (number of streams) + nbytes (every stream
 *   stored).  0 for arguments that are not accepted (text in tm_last_error()).  Host only. */
size_t tm_blosc_bound(size_t nbytes, int typesize, int blocksize);

/* tm_blosc_compress: one frame of the `nbytes` contiguous bytes at src (device, no alignment needed) into frame (device,
 *   frame_cap >= tm_blosc_bound(...) bytes); *out_bytes (int64, device) = the frame's length.  Bytes of `frame` past that
 *   length are not written.  Asynchronous on `stream`; the stream slots are stream-ordered scratch (nbytes + tables). */
int tm_blosc_compress(const void* src, size_t nbytes, int typesize, int blocksize, void* frame, size_t frame_cap,
                      int64_t* out_bytes, void* stream);

/* tm_blosc_compress_tiles: one frame per state tile [C][TH][TW], cut in place out of a resident canvas and written as
 *   float16 (typesize 2, blocksize 65536: the reference's tile [100][256][256] is 200 whole blocks).
 *   canvas       device, TM_DTYPE_F16 or TM_DTYPE_F32, `canvas_elems` elements; element (c, y, x) of tile k sits at
 *                origins[k] + c * chan_stride + y * pitch + x.  float32 is rounded as Tensor.half() rounds: to nearest even,
 *                overflow to +-inf, subnormals and -0.0 kept, NaN as the hardware conversion gives it
 *   origins      int64 [ntiles] device, origins_host its host mirror (checked against canvas_elems before any device call)
 *   packed       uint8 [packed_cap] device, packed_cap >= ntiles * tm_blosc_bound(2 C TH TW, 2, 65536): the frames back to back
 *   offsets      int64 [ntiles + 1] device: frame k at packed + offsets[k], offsets[ntiles] = their total
 *   Asynchronous on `stream`; stream-ordered scratch of ntiles x (tile bytes + tables). */
int tm_blosc_compress_tiles(const void* canvas, int dtype, int64_t canvas_elems, int C, int TH, int TW, int64_t chan_stride,
                            int64_t pitch, const int64_t* origins, const int64_t* origins_host, int ntiles, void* packed,
                            int64_t packed_cap, int64_t* offsets, void* stream);

/* ---- Blosc-lz4 decoder on the GPU: the way back from a step directory into a resident canvas ----------------------
 * Reads what tm_blosc_decompress reads -- the frames of tm_blosc_compress_tiles and those c-blosc writes for zarr (any block
 * size, so streams of any length; blocks split or not; byte shuffle or none; memcpyed frames as a plain copy; typesize 1, 2
 * or 4) -- with the same leniency: the LZ4 end-of-block rules are not enforced, a file the host route reads reads the same
 * here.  The host walks header, bstarts and stream lengths of every frame (its host mirror) before any device call; the
 * kernels decode one stream per wave with the decoded history in LDS and never read back global memory they wrote.
 *
 * tm_blosc_frame_info: one frame (host memory, no device call).  TM_OK and *out filled: gpu = 1, the GPU decoder takes the
 *   frame (nstreams and the longest stream's plain size set); gpu = 0, "host only": bit shuffle, a codec other than lz4, a
 *   typesize other than 1 / 2 / 4 or more than 2^30 plain bytes (nstreams = longest = 0).  TM_ERR_ARG with a text: a frame
 *   shorter than its header, cbytes beyond the buffer, a block table, bstarts entry or stream length outside the frame. */
typedef struct tm_blosc_frame {
  int64_t nbytes;        /* plain bytes */
  int32_t typesize, blocksize, nstreams, longest, flags, gpu;
} tm_blosc_frame;
int tm_blosc_frame_info(const void* frame, size_t frame_bytes, tm_blosc_frame* out);

/* tm_blosc_decompress_dev: nframes (1 .. 65535) frames; frame k is the bytes [frame_offsets[k], frame_offsets[k + 1]) of
 *   `frames` (device, no alignment needed) and of `frames_host`, its host mirror (what the zip reader holds); frame_offsets
 *   int64 [nframes + 1] host, non-decreasing from >= 0.  The plain bytes of frame k go to dst + dst_offsets[k] (device;
 *   dst_offsets int64 [nframes] host, every range inside dst_cap; bytes outside the ranges are not written).
 *   status int32 [nframes] device: 0, or which rule a stream of the frame broke (1 ends short of its plain size, 2 length
 *   extension off the end, 3 literals past the stream, 4 literals past the plain size, 5 offset cut, 6 offset 0, 7 offset
 *   beyond the bytes produced, 8 match past the plain size; the largest of the frame's streams).  A frame with a non-zero
 *   status has no bytes delivered; the other frames of the call are unaffected.
 *   TM_ERR_ARG with a text and nothing launched: anything tm_blosc_frame_info refuses or answers "host only", a null
 *   pointer, a range outside dst_cap.  Asynchronous on `stream`; stream-ordered scratch of the plain size plus tables. */
int tm_blosc_decompress_dev(const void* frames, const void* frames_host, const int64_t* frame_offsets, int nframes, void* dst,
                            int64_t dst_cap, const int64_t* dst_offsets, int32_t* status, void* stream);

/* tm_blosc_decompress_tiles: the same into a canvas (the mirror of tm_blosc_compress_tiles).  Frame k is a float16 chunk
 *   [chunk[0]][chunk[1]][chunk[2]] (typesize 2, nbytes = 2 x its elements: zarr stores edge chunks full size); its element
 *   (c, y, x) with c < clip[0], y < clip[1], x < clip[2] lands at origin + c * chan_stride + y * pitch + x of the canvas
 *   (TM_DTYPE_F16: copied; TM_DTYPE_F32: widened, as .float() does); 1 <= clip[i] <= chunk[i].  boxes [nframes] host; every
 *   box is checked against canvas_elems before any device call.  Elements outside the boxes are not written. */
typedef struct tm_blosc_box {
  int64_t origin;
  int32_t chunk[3], clip[3];
} tm_blosc_box;
int tm_blosc_decompress_tiles(const void* frames, const void* frames_host, const int64_t* frame_offsets, int nframes, void* canvas,
                              int dtype, int64_t canvas_elems, int64_t chan_stride, int64_t pitch, const tm_blosc_box* boxes,
                              int32_t* status, void* stream);

/* ---- slice export: the pyramid levels and JPEG tiles of infer_brn.get_ome --------
 * (infer_brn.py:11-54: `tiffsave(tile=True, compression='jpeg', pyramid=True, bigtiff=True, tile 256 x 256)`), computed
 * from a resident uint8 plane.  The container is written by teramind_amd.ometiff.
 *
 * tm_u8_shrink2: dst [ceil(H / 2)][ceil(W / 2)] uint8 device = (a + b + c + d + 2) >> 2 over the 2 x 2 blocks of
 *   src [H][W]; an odd last row / column is repeated.  Pitches in bytes, src_pitch >= W, dst_pitch >= ceil(W / 2); bytes of
 *   dst outside the level are not written.  Asynchronous on `stream`. */
int tm_u8_shrink2(const void* src, int H, int W, int64_t src_pitch, void* dst, int64_t dst_pitch, void* stream);

/* tm_jpeg_encode_tiles: baseline-JPEG entropy-coded segments (ITU-T T.81; no markers) of tiles [tile0, tile0 + ntiles) of
 *   the ceil(H / 256) x ceil(W / 256) grid (row-major) of plane [H][W] uint8 device, one 8-bit grey component, one
 *   256 x 256 tile per scan; pixels beyond the image repeat the last row / column.  Exact integer arithmetic: level shift
 *   128, the 8 x 8 "islow" integer forward DCT, quantiser (|c| + qv / 2) / qv with qv = q << 3 and q the Annex K.1
 *   luminance table scaled for `quality` (1 .. 100; s = 5000 / Q below 50, else 200 - 2 Q; q = clamp((base s + 50) / 100,
 *   1, 255)), zigzag, DC predicted from the previous block of the tile (0 at its start), the typical Huffman tables of
 *   Annex K.3, byte stuffing, one-bit padding, no restart markers.  The bytes are those libjpeg writes for the tile.
 *   slots  uint8 [ntiles][slot_bytes] device: slot k belongs to tile tile0 + k
 *   need   int32 [ntiles] device: always written, the bytes tile tile0 + k takes.  The bytes themselves are written only if
 *          need[k] <= slot_bytes; a slot that is too small is left untouched (the caller encodes that tile again with a
 *          slot sized from need: a size query, not a fallback)
 *   packed / offsets (both or neither): uint8 [ntiles * slot_bytes] and int64 [ntiles + 1] device: the filled slots back
 *          to back, slot k at offsets[k], offsets[ntiles] = their total (a slot that was too small takes 0 bytes)
 *   Asynchronous on `stream`; the bit buffers are stream-ordered scratch of the call (at most 512 x 208 KB). */
int tm_jpeg_encode_tiles(const void* plane, int H, int W, int64_t pitch, int quality, int tile0, int ntiles, void* slots,
                         int64_t slot_bytes, int32_t* need, void* packed, int64_t* offsets, void* stream);

/* The tables-only datastream SOI DQT DHT(DC) DHT(AC) EOI for `quality`: the TIFF JPEGTables tag of tiles encoded by
 * tm_jpeg_encode_tiles (which reads the same table statements).  buf == NULL: only *out_bytes is set.  Host only. */
int tm_jpeg_tables(int quality, void* buf, size_t cap, size_t* out_bytes);

/* ---- colour composite export: two stains in one image, as utils/vis_mba.py:193-195 stacks [0, PolyT, DAPI] and
 * onto_overlay (:118-179) brightens it and blends an ontology image over it.
 *
 * The composite of pixel (y, x) of a level [H][W], from three planar uint8 device planes planes[0 .. 2] = R, G, B with their
 * own pitches[] in bytes (a null plane is all zeros; not all three may be null):
 *   brightness  v <- min(255, trunc(float32(bright) * float32(v))) per channel, skipped when bright == 1 (bright >= 0, finite)
 *   overlay     optional uint8 [oh][ow][3] device image, alpha 0 .. 255: ov = overlay[(y oh) / H][(x ow) / W] (integer
 *               division: nearest sampling by the level's own size); where any channel of ov is non-zero
 *               v_c <- (ov_c alpha + v_c (255 - alpha) + 127) / 255, elsewhere v is unchanged.  H oh and W ow below 2^31.
 * in that order.  The blend rounding is this library's own (equality with libvips' composite is not pinned).
 *
 * tm_rgb_compose: the composite of the whole level as interleaved uint8 dst [H][W][3] device, dst_pitch >= 3 W bytes.
 *   Asynchronous on `stream`. */
int tm_rgb_compose(const void* const* planes, const int64_t* pitches, int H, int W, float bright, const void* overlay, int oh, int ow,
                   int alpha, void* dst, int64_t dst_pitch, void* stream);

/* tm_jpeg_encode_tiles_rgb: tm_jpeg_encode_tiles for the composite, which is formed in the block load (no RGB image of the
 *   level is stored).  Baseline JPEG, three components Y Cb Cr all sampled 1 x 1 (4:4:4), one interleaved scan per 256 x 256
 *   tile, MCU = 8 x 8 pixels = one Y, one Cb, one Cr block; colour conversion in libjpeg's fixed point:
 *     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   Y on quantiser 0 (K.1) and Huffman tables 0 / 0 (K.3, K.5); Cb and Cr on quantiser 1 (K.2, scaled and clipped like K.1)
 *   and tables 1 / 1 (K.4, K.6); DC predicted per component.  The bytes are those libjpeg writes for the tile with
 *   4:4:4 sampling.  slots / slot_bytes / need / packed / offsets / stream exactly as in tm_jpeg_encode_tiles; the bit
 *   buffers are three times as large (at most 512 x 623 KB of stream-ordered scratch). */
int tm_jpeg_encode_tiles_rgb(const void* const* planes, const int64_t* pitches, int H, int W, float bright, const void* overlay,
                             int oh, int ow, int alpha, int quality, int tile0, int ntiles, void* slots, int64_t slot_bytes,
                             int32_t* need, void* packed, int64_t* offsets, void* stream);

/* The tables-only datastream SOI DQT(0) DQT(1) DHT(DC 0) DHT(AC 0) DHT(DC 1) DHT(AC 1) EOI for `quality` (the segments and
 * the order libjpeg writes): the JPEGTables tag of tiles encoded by tm_jpeg_encode_tiles_rgb.  buf == NULL: only
 * *out_bytes is set.  Host only. */
int tm_jpeg_tables_rgb(int quality, void* buf, size_t cap, size_t* out_bytes);

/* ---- attention heat maps: the figures test_attn.py:145-250 (`gen_img`) draws from a slice of the read-out mosaic --------
 * tm_heat_field: the smoothed scalar field of one slice.  src float16 device [C][H][W], row y of channel c at
 *   src + c * src_chan + y * src_pitch (both in ELEMENTS, so a slice of the [50, 4K, H, W] mosaic or a window of it is read in
 *   place); dst float32 device [H][W], dst_pitch in elements; cells of dst outside [H][W] are not written.  Per cell
 *     v = sum over c in [sum0, sum0 + nsum) of max(float(src[c]), 0), added in index order in float32 (1 <= nsum <= 8)
 *     f = log2(v * wei + 1)
 *     p = f where every src[mask0 + k] != 0, k < nmask (0 <= nmask <= 8; nmask = 0: everywhere), else 0
 *     dst[y][x] = sum_i sum_j t[i] t[j] p[R(y + i - r, H)][R(x + j - r, W)], along axis 0 first, then along axis 1, each
 *       a float32 sum of 2 r + 1 multiply-adds in tap order from zero; t = taps_host, 2 r + 1 float32 on the HOST, 0 <= r <= 16
 *       (r = 0 with t = {1}: the identity); R the half-sample reflection of scipy's mode='reflect', R(-j) = j - 1,
 *       R(n - 1 + j) = n - j
 *   = scipy.ndimage.gaussian_filter(np.log2(s * wei + 1) * msk, sigma) (test_attn.py:204-206) when the taps are scipy's.
 *   Held to a derived float32 bound against a float64 model (tests/heatmap_cases.py), not to bits; no atomics, two calls give
 *   the same bits.  Non-finite inputs give non-finite outputs inside their window.  One kernel, no global scratch.
 *   Asynchronous on `stream`.  TM_ERR_ARG with a text before any device call: a null pointer, r outside 0 .. 16, H or W below
 *   max(r, 1) (one reflection must suffice), nsum outside 1 .. 8, nmask outside 0 .. 8, a channel range outside [0, C), a
 *   pitch below the row, a channel stride below the extent of one channel, a misaligned pointer. */
int tm_heat_field(const void* src, int C, int H, int W, int64_t src_pitch, int64_t src_chan, int sum0, int nsum, float wei,
                  int mask0, int nmask, const float* taps_host, int r, void* dst, int64_t dst_pitch, void* stream);

/* tm_heat_render: field float32 device [H][W] (field_pitch in elements) -> colour bytes [H scale][W scale], scale in
 *   {1, 2, 4, 8, 16}, through the table lut_host uint8 [N][3] on the HOST, 2 <= N <= 256.  Exact float32, every operation
 *   rounded once, nothing fused.  Pixel (y, x):
 *     sx = (x + 0.5f) * (1.0f / scale) - 0.5f, clamped to [0, W - 1]; x0 = (int)sx, x1 = min(x0 + 1, W - 1), wx = sx - x0;
 *     the same for y (bilinear, half-pixel centres: F.interpolate(align_corners=False))
 *     top = f00 + (f01 - f00) * wx; bot = f10 + (f11 - f10) * wx; g = top + (bot - top) * wy  (scale 1: g = the cell, when
 *     its right / lower neighbours are finite)
 *     i = ((g - vmin) * inv_range) * N, inv_range = float32(1 / (vmax - vmin)) formed by the caller
 *     idx = !(i >= 0) ? 0 : min(N - 1, (int)i)  (NaN -> 0): matplotlib's Colormap.__call__(bytes=True) after Normalize
 *     pixel = (0, 0, 0) when idx < floor_idx (>= 0), else lut[idx]  (the colour encoder's overlay blend treats black as
 *     transparent; inferno[0] is (0, 0, 3))
 *   Destination: either planes[0 .. 2] = R, G, B planar uint8 device with pitches[] in bytes (what tm_rgb_compose /
 *   tm_jpeg_encode_tiles_rgb take as planes), or `interleaved` uint8 device [h][w][3] with inter_pitch >= 3 w bytes (what they
 *   take as overlay); exactly one of the two is non-null.  Bytes outside the image are not written.  Asynchronous on `stream`.
 *   TM_ERR_ARG with a text before any device call: a null pointer, both or neither destination, another scale, N outside
 *   2 .. 256, floor_idx < 0, a pitch below the row, 3 W scale or H scale beyond 2^31 - 1. */
int tm_heat_render(const void* field, int H, int W, int64_t field_pitch, int scale, float vmin, float inv_range,
                   const uint8_t* lut_host, int N, int floor_idx, void* const* planes, const int64_t* pitches, void* interleaved,
                   int64_t inter_pitch, void* stream);

/* ---- ROI evaluation ("evaluation"): the measures of utils/metrics.py:201-541 for a generated / real plane pair ----
 * Pixels are uint8 or float32, chosen by `dtype`; pitches and plane strides are in bytes.  uint8 pointers need no alignment;
 * float32 pointers, pitches and strides are multiples of 4. */
enum { TM_PIX_U8 = 0, TM_PIX_F32 = 1 };

/* tm_ssim_planes: for each of the P plane pairs x[p], y[p] of [H][W] (plane p at x + p * x_plane, row r at + r * x_pitch):
 *   out[p][0] = sum of ssim_map, out[p][1] = sum of cs_map over the (H - n + 1) x (W - n + 1) valid region of `_ssim`
 *               (utils/metrics.py:266-305): the separable valid filter of x, y, x^2, y^2, x y with the n taps of win_host
 *               (float32, host; n odd, 3 .. 33), cs = (2 s12 + C2) / (s1 + s2 + C2),
 *               ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs
 *   out[p][2] = sum of (x - y)^2 over the whole plane (what PSNR needs); for uint8 the exact integer
 *   out is double [P][3] on the device.  The filters and maps are fp32, the second moments are formed about one pixel value
 *   per image and 64 x 32 tile (the variances do not depend on it; no cancellation on near-saturated planes); each lane adds its 8
 *   outputs in fp32, everything above is fp64 in a fixed tree: no atomics, two calls give the same bits.
 *   Asynchronous on `stream`; the per-tile partials are stream-ordered scratch of the call.
 *   TM_ERR_ARG with a text before any device call: a null pointer, an unknown dtype, n even or outside 3 .. 33, H or W below
 *   n, P outside 1 .. 65535, a pitch below the row, a misaligned float32 operand. */
int tm_ssim_planes(const void* x, const void* y, int dtype, int P, int H, int W, int64_t x_pitch, int64_t x_plane,
                   int64_t y_pitch, int64_t y_plane, const float* win_host, int n, float C1, float C2, double* out,
                   void* stream);

/* tm_avgpool2_pad: one MS-SSIM level (utils/metrics.py:428-430), F.avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2)):
 *   dst float32 [P][ceil(H / 2)][ceil(W / 2)], window (i, j) = rows 2 i - H % 2 .., columns 2 j - W % 2 .. of src, a row or
 *   column -1 being the zero pad; the sum (row-major) times 0.25: the pad is counted.  src uint8 or float32 by `dtype`.
 *   Asynchronous on `stream`.  TM_ERR_ARG before any device call as for tm_ssim_planes. */
int tm_avgpool2_pad(const void* src, int dtype, int P, int H, int W, int64_t src_pitch, int64_t src_plane, void* dst,
                    int64_t dst_pitch, int64_t dst_plane, void* stream);

/* tm_ssim_volumes: the 3-D window of `_ssim` on a 5-D input (conv3d along depth, rows and columns).  For each of the V volume
 * pairs x[v], y[v] of [D][H][W] (volume v at x + v * x_vol, plane z at + z * x_depth, row r at + r * x_pitch; all in bytes; the
 * depth stride is its own argument so that one stain of an '(s c)'-ordered mosaic, every n_stain-th plane, is read in place):
 *   out[v][0] = sum of ssim_map, out[v][1] = sum of cs_map over the (D - n + 1)(H - n + 1)(W - n + 1) valid region: the
 *               separable valid filter of x, y, x^2, y^2, x y with the n taps of win_host (float32, host; n odd, 3 .. 11;
 *               shorter windows run as 11 taps with zeros behind) along columns, rows and depth
 *   out[v][2] = sum of (x - y)^2 over the whole volume; for uint8 the exact integer
 *   out is double [V][3] on the device.  The filters and maps are fp32; the second moments are formed about one voxel value
 *   per image and 16 x 16 in-plane tile (the tile's first voxel of plane 0) and corrected with S = (sum of the taps)^3 and
 *   1 - S, formed in double; a lane owns 1 output per plane, so it adds none of its outputs in fp32: every output goes to an
 *   fp64 sum, in a fixed tree: no atomics, two calls give the same bits.  Asynchronous on `stream`; the per-tile partials are stream-ordered.
 *   TM_ERR_ARG with a text before any device call: a null pointer, an unknown dtype, n even or outside 3 .. 11 (a lane keeps
 *   the depth window of every output in registers: longer windows do not fit), D, H or W below n, V outside 1 .. 65535, a
 *   pitch below the row, a depth stride below the extent of one plane ((H - 1) pitch + the row), a misaligned float32
 *   operand (pointer, pitch, depth and volume strides are multiples of 4). */
int tm_ssim_volumes(const void* x, const void* y, int dtype, int V, int D, int H, int W, int64_t x_pitch, int64_t x_depth,
                    int64_t x_vol, int64_t y_pitch, int64_t y_depth, int64_t y_vol, const float* win_host, int n, float C1,
                    float C2, double* out, void* stream);

/* tm_avgpool2_pad3: one 5-D MS-SSIM level, F.avg_pool3d(kernel 2, stride 2, padding (D % 2, H % 2, W % 2)):
 *   dst float32 [V][ceil(D / 2)][ceil(H / 2)][ceil(W / 2)], window (k, i, j) = planes 2 k - D % 2 .., rows 2 i - H % 2 ..,
 *   columns 2 j - W % 2 .. of src, a plane, row or column -1 being the zero pad, which is counted: the divisor is 8 (D = 1
 *   pools to one plane of the in-plane sums / 8).  The eight values are added from 0 in the order plane, then row, then
 *   column (v000, v001, v010, v011, v100, ..., the last index the column) and the sum is multiplied by 0.125; on 8-bit data
 *   every level is exact.  src uint8 or float32 by `dtype`.  Asynchronous on `stream`.  TM_ERR_ARG before any device call as
 *   for tm_ssim_volumes (the destination is held to the float32 rules). */
int tm_avgpool2_pad3(const void* src, int dtype, int V, int D, int H, int W, int64_t src_pitch, int64_t src_depth,
                     int64_t src_vol, void* dst, int64_t dst_pitch, int64_t dst_depth, int64_t dst_vol, void* stream);

/* Measurement hooks (bench.py): while enabled, every launch of the dominant kernel
 * (conv3d_mfma<2,..> in fp32, conv27_bf16 / conv27_f16 in the 16-bit modes: the 3x3x3 implicit-GEMM conv) inside tm_unet_forward is bracketed by two
 * hipEvents recorded on the forward's stream.  tm_profile_collect synchronises on the last
 * event, adds up the bracketed durations and the per-launch work, and resets the counters.
 *   nominal_flops  = 2*Cin*Cout*27*voxels per launch (dense-conv convention; what
 *                    torch.utils.flop_counter counts for the reference's Conv3d)
 *   executed_flops = the MFMA FLOPs actually issued: for z_size 2, fp32, 1/2 of that (pair form: three in-plane products per
 *                    plane pair, 27 of the nominal 54 taps; 1/4 for a launch in the x-quad form, 54 tap-products per eight
 *                    outputs; 2/3 with TM_CONV_ZPAIR=0 and in the 16-bit modes, where only the always-zero z tap is
 *                    skipped), 1/3 for z_size 1 (centre slice only), all of it for z_size 4 / 8
 *   alg_bytes      = input + packed weights + output bytes, each counted once per launch */
typedef struct tm_prof_stats {
  uint64_t launches;
  double total_ms;
  double nominal_flops;
  double executed_flops;
  double alg_bytes;
} tm_prof_stats;
int tm_profile_enable(tm_model* m, int on);
int tm_profile_collect(tm_model* m, tm_prof_stats* out);

/* ---- single-operator entry points (parity tests of the individual kernels) -------------
 * Layout "CB8": fp32 [N][ceil(C/8)][Z][H][W][8] (channel blocks of 8, zero padded).
 *
 * These are test and training entry points (tests/test_gpu_ops.py, teramind_amd.training,
 * teramind_amd.train_model), not the product path, and they keep the conventions above
 * only in part: they take HOST weights, biases and gradient outputs where the signature
 * says so (`*_host`), allocate and free temporary device memory inside the call, and
 * synchronise `stream` before they return.  tm_op_to_cb8 and tm_op_from_cb8 only enqueue
 * (no allocation, no synchronisation).                                                   */

/* NCDHW fp32 <-> CB8 */
int tm_op_to_cb8(const void* x_ncdhw, void* y_cb8, int N, int C, int Z, int H, int W, void* stream);
int tm_op_from_cb8(const void* x_cb8, void* y_ncdhw, int N, int C, int Z, int H, int W, void* stream);

/* Conv3d on the MFMA implicit-GEMM kernels (replaces nn.Conv3d as used in ResBlock,
 * model/MBAblocks.py:146-148,182-186,220-224, the RNA pyramid convs model/unet_ours.py:290-295
 * and down_z model/MBAblocks.py:472-474).  ksize 1: 1x1x1.  ksize 3 with zmode
 *   0: 3x3x3 pad (1,1,1), any Z >= 1 (the plane-pair form at Z == 2, the three-plane form otherwise)
 *   1: 1x3x3 pad (0,1,1)      2: 3x3x3 pad (0,1,1) (Zout = Z-2)
 *   3: 3x3x3 pad (1,1,1) of the nearest-x2 UPSAMPLED x (Upsample then Conv3d as in ResBlock(up=True), model/MBAblocks.py:254-258,
 *      blocks.py:362-371), Z == 2, computed on x itself with per-phase 2x2 in-plane weights: y is [N, Cout, Z, 2S, 2S].
 * up2: nearest x2 on (H, W) applied to the output (not with zmode 3).  w [Cout][Cin][kz][3][3] HOST fp32,
 * bias [Cout] HOST fp32; x, y CB8 DEVICE.
 * tile_variant: 0 = the launcher's choice by launch size, 1 | 2 = 128- | 256-voxel workgroup tiles.  With ksize 1 also 3 = the
 * 128-cout tile of the 1x1x1 kernel whatever the launch size (tm_conv1_form; an odd count of 64-cout tiles is refused with a
 * HIP invalid-value error); with ksize 3 any other value means 1. */
int tm_op_conv_mfma(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8,
                    int N, int Cin, int Cout, int Z, int S, int ksize, int zmode, int up2,
                    int tile_variant, void* stream);
/* The same with the epilogue's residual (ksize 3, not zmode 3): y = res + conv + bias, res CB8 DEVICE in y's geometry, or with
 * res_half != 0 at half the in-plane resolution ([N][ceil(Cout/8)][Zout][S/2][S/2][8], read at (z, y >> 1, x >> 1): the
 * residual of a ResBlock(up=True)).  res_cb8 NULL: tm_op_conv_mfma.  tile_variant as there. */
int tm_op_conv_mfma_res(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                        int res_half, int N, int Cin, int Cout, int Z, int S, int ksize, int zmode, int up2,
                        int tile_variant, void* stream);

/* The fp32 3x3x3 pad-1 conv at Z == 2 in its pair form with the ResBlock mid-section fused into the epilogue (Cout == 64, the
 * 128-voxel tile): out_layers[0] RMSNorm(C) * norm_w -> x * (1 + scale) + shift -> SiLU (model/MBAblocks.py:196-203,356-367),
 * written as the fp32 CB8 tensor a2_out [N][8][2][S][S][8] (the second conv's input); the conv output itself is not stored.
 * x CB8 DEVICE; w [64][Cin][27], bias [64], norm_w [64], scale / shift [ceil(N/per_image)][64] HOST fp32; patch n uses row
 * n / per_image.  h1_out (nullable, DEVICE, a2's shape): conv + bias from a second, plain launch of the same tile.  a2_sep_out
 * (nullable, needs h1_out): the separate norm pass (prep_kernel) applied to h1_out.  tile_variant: 0 = by launch size, 1 | 2 =
 * the 64- | 128-voxel tile.  TM_ERR_ARG before any device call: Z != 2, Cout != 64, a residual (res_cb8 non-NULL), S outside
 * {8, .., 128}, a launch that takes the 64-voxel tile, the pair form switched off. */
int tm_op_conv_zpair_fused_f32(const void* x_cb8, const void* w_host, const void* bias_host, const void* norm_w_host,
                               const void* scale_host, const void* shift_host, const void* res_cb8, void* a2_out,
                               void* h1_out, void* a2_sep_out, int N, int Cin, int Cout, int Z, int S, int per_image,
                               int tile_variant, void* stream);

/* The fp32 3x3x3 pad-1 conv of the nearest-x2 UPSAMPLED x at Z == 2 (ResBlock(up=True)'s first conv), computed on x itself in
 * the pair form (conv3d_zpair_ups: per output phase three 2x2 in-plane products per plane pair).  x CB8 DEVICE
 * [N][ceil(Cin/8)][2][S][S][8]; w [Cout][Cin][27], bias [Cout] HOST; y CB8 DEVICE [N][ceil(Cout/8)][2][2S][2S][8].
 * tile_variant: 0 = by launch size, 1 | 2 = the 64- | 128-voxel tile.  TM_ERR_ARG before any device call: Z != 2, S outside
 * {4, .., 64}.  tm_op_conv_mfma with zmode 3 is the z-skip form of the same conv. */
int tm_op_conv_ups_pair_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                            int Cout, int Z, int S, int tile_variant, void* stream);

/* The fp32 3x3x3 pad-1 conv at Z == 2 in its x-quad form (conv3d_xquad: the pair form in z composed with Winograd F(4,3) along
 * x, 54 tap-products per eight outputs).  x CB8 DEVICE [N][ceil(Cin/8)][2][S][S][8]; w [Cout][Cin][27], bias [Cout] HOST; y CB8
 * DEVICE; res_cb8 (nullable): y's geometry, or S / 2 in-plane with res_half != 0 (read at (z, y >> 1, x >> 1)).  tile_variant:
 * 0 = by launch size, 1 | 2 = 64 | 128 four-column groups per workgroup.  Returns the tile launched (1 | 2) on success.
 * TM_ERR_ARG before any device call: Z != 2, S outside {8, .., 128} (so S = 4 and every S that is no multiple of 4), the form
 * switched off (TM_CONV_XQUAD=0).  tm_op_conv_mfma with zmode 0 stays the pair form of the same conv. */
int tm_op_conv_xquad_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                         int res_half, int N, int Cin, int Cout, int Z, int S, int tile_variant, void* stream);
/* tm_op_conv_xquad_f32 with the schedule of conv3d_xquad forced: sched 0 = four barriers per cin block (all eighteen q-planes of
 * a block staged in a phase of its own), 1 = the pipelined schedule (a ring of two sets of six q-planes staged under the
 * products, three barriers).  Same pack, same order of sums: the two give identical bits.  tm_op_conv_xquad_f32 itself takes
 * the launcher's choice per instantiation; TM_CONV_XQUAD_PIPE=0 (read once) keeps schedule 0 everywhere.  TM_ERR_ARG also for
 * a sched outside 0 | 1. */
int tm_op_conv_xquad_sched_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                               int res_half, int N, int Cin, int Cout, int Z, int S, int tile_variant, int sched, void* stream);
/* The dynamic LDS (bytes) of conv3d_xquad in the large | small tile (half 0 | 1), tile width tw (8 | 16) and schedule sched
 * (0 | 1); -1 if there is no such instantiation.  No device call. */
int tm_conv_xquad_lds_bytes(int half, int tw, int sched);
/* Timing hook (tools/bench_conv_xquad.py): that conv packed once for `form` (0 = the pair form, 2 = the x-quad form; any other
 * value, 1 included, is TM_ERR_ARG), then `iters` launches, each between two events of its own: ms_out[i] (HOST) = the time of
 * launch i.  sched: the schedule of conv3d_xquad (form 2 only), 0 | 1 as in tm_op_conv_xquad_sched_f32, -1 = the launcher's
 * choice. */
int tm_op_conv_pad1_time_sched_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                   int Cout, int S, int form, int tile_variant, int sched, int iters, float* ms_out, void* stream);
/* tm_op_conv_xquad_sched_f32 with the K loop split over workgroups: ksplit workgroups per (voxel tile, cout tile) run disjoint
 * ranges of the cin blocks and write raw partial sums, and a second pass (xquad_split_reduce) forms ((p0 + p1) + p2) + p3, adds
 * the bias and then the residual, one float4 per lane, so res_cb8 == y_cb8 is legal.  ksplit 0 =
 * the rule (tm_conv_xquad_ksplit), 1 | 2 | 4 force the factor; 1 is the unsplit launch, bit for bit.  Returns the factor taken.
 * TM_ERR_ARG before any device call, besides the refusals of tm_op_conv_xquad_sched_f32: a factor outside 0 | 1 | 2 | 4, a
 * factor above the count of cin blocks ceil(Cin / 8) (a split would be empty), a forced split with res_half. */
int tm_op_conv_xquad_split_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                               int res_half, int N, int Cin, int Cout, int Z, int S, int tile_variant, int sched, int ksplit,
                               void* stream);
/* The rule of the split: the factor (1 | 2) of an x-quad launch of N patches of 2 x S x S voxels.  1 wherever the launch has
 * 256 large workgroups or more, or 256 small ones, with res_half, with fewer than 8 cin blocks, and everywhere with
 * TM_CONV_XQUAD_SPLIT=0 (read once); 2 otherwise, however few the workgroups, so that one image sums in the order of its batch.
 * The rule of one launch on its own: the executor fixes the factor per layer (2 for the decoder blocks of the deepest level at
 * every patch count, 1 for every other layer), so that results do not depend on how many patches a call holds.  No device call. */
int tm_conv_xquad_ksplit(int N, int Cin, int Cout, int S, int res_half);
/* tm_op_conv_pad1_time_sched_f32 with ksplit (form 2 only; 0 = the rule, 1 | 2 | 4 forced): a launch is the conv and, when
 * split, its reduction, both between the two events. */
int tm_op_conv_pad1_time_split_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                   int Cout, int S, int form, int tile_variant, int sched, int ksplit, int iters, float* ms_out,
                                   void* stream);

/* The fp32 1x1x1 conv / Linear (conv1_mfma) in every form the model launches: y = res + gate_up * act(W x + b).
 * x_cb8: DEVICE [N][x_cbtot][Z][S][S][8]; the conv reads the channel-block slice [x_cb0, x_cb0 + ceil(Cin/8)) of it in place
 * (the patch stride stays that of the wide tensor).  w_host [Cout][Cin], bias_host [Cout]: HOST.  y_cb8: [N][ceil(Cout/8)][Z][S][S][8].
 * res_cb8 (nullable): y's geometry; res_cb8 == y_cb8 is the in-place update x <- x + gate * Linear(.).  gate_cb8 (nullable):
 * [N][gate_cbtot][Z][Sg][Sg][8], read from block gate_cb0 on; Sg = S, or S / 2 with gate_half != 0 (read at (z, y >> 1, x >> 1)).
 * gelu != 0: act = tanh-GELU.  tile_variant: 0 = the launcher's choice, 1 | 2 = 128- | 256-voxel tiles, 3 = the 128-cout tile
 * whatever the launch size.  *form_out (nullable) receives the kernel form launched (tm_conv1_form).
 * TM_ERR_ARG before any device call: gate_half without a gate or with S not a power of two >= 2, a slice that runs past its
 * tensor, tile_variant outside 0..3 or 3 with an odd count of 64-cout tiles. */
int tm_op_conv1_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                    const void* gate_cb8, int x_cbtot, int x_cb0, int gate_cbtot, int gate_cb0, int gate_half, int gelu,
                    int tile_variant, int N, int Cin, int Cout, int Z, int S, int* form_out, void* stream);
/* The form of the fp32 1x1x1 conv kernel a launch of `vox` voxels and `ntile` = ceil(Cout/64) cout tiles takes: 1 = 128 voxels
 * x 64 couts per workgroup, 2 = 256 x 64, 3 = 256 x 128; 0 = refused (tile_variant 3 with an odd ntile).  Host only. */
int tm_conv1_form(long vox, int ntile, int tile_variant);

/* Where the lanes of the fp32 LDS-DMA conv kernels address LDS (no device call; for bank-conflict models of the operand images).
 * kernel 0 = conv3d_zpair, 1 = conv3d_zpair_ups; half 0 | 1 = the large | small tile; tw = tile width (4 | 8 | 16 | 32); wave
 * 0..3.  what 0: the weight fragment (ds_read_b128) of product p (0..2), window row ky, column kx and 32-cout sub-tile sub; what
 * 1: the activation fragment of (p, ky, kx), sub = the output phase 2 py + px of kernel 1 (else 0); what 2: the staging store
 * (ds_write_b128) into plane p of the thread's ky-th item.  out64[lane] = byte address in the workgroup's dynamic LDS, -1 for a
 * lane that stores nothing.  kernel 4 = conv3d_xquad (2 and 3 are no kernels and stay refused): tw 8 | 16, wave 0..7 (0..3 in
 * the small tile), kx = the wave's q-th transform position (0..2), in what 2 ky 0 and kx = the q-plane (0..5).  kernel 5 =
 * conv3d_xquad in its pipelined schedule: as 4, but the X planes are a ring of two sets of six and sub = the plane set (0 | 1) of
 * an activation fragment or a staging store (product n of the running count reads set n & 1; sub 0 for a weight fragment).
 * Returns 0, or -1 if there is no such instantiation, fragment or item. */
int tm_conv_frag_addrs(int kernel, int half, int tw, int what, int wave, int p, int ky, int kx, int sub, int* out64);

/* 16-bit variant of the 3x3x3 pad-1 conv (Z == 2): x fp32 CB8 is rounded to `dtype` (TM_DTYPE_BF16 | TM_DTYPE_F16, RNE) on
 * the device, w rounded on the host; fp32 accumulate, fp32 CB8 output.  waves: 0 = the launcher's choice, 4 | 8 = force
 * the 4-wave (128 x 256 / 64 x 512 tile) or 8-wave (128 x 512 / 64 x 1024) workgroup form.
 * res_h16 (nullable): 16-bit CB8 residual [N][ceil(Cout/8)][2][S][S][8] added in fp32 before the final rounding;
 * y_h16 (nullable): write the result as a 16-bit CB8 tensor of that shape INSTEAD of y_cb8 (the 16-bit activation
 * stream of the model: block outputs and residuals are 16-bit tensors, as under the reference's fp16 autocast).
 * ups != 0: the conv of the nearest-x2 UPSAMPLED x (ResBlock(up=True), model/MBAblocks.py:254-258), computed on x itself with
 * per-phase 2x2 in-plane weights: outputs are [N, Cout, 2, 2S, 2S]; Cout a multiple of 128, no residual.
 * res_half != 0: res_h16 is [N][ceil(Cout/8)][2][S/2][S/2][8] and read at (z, y >> 1, x >> 1) (the residual of that block:
 * the upsampled block input, :297). */
int tm_op_conv27_bf16(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8,
                      int N, int Cin, int Cout, int S, int dtype, int waves, const void* res_h16, void* y_h16,
                      int ups, int res_half, void* stream);
/* The same on Z planes, 1 <= Z <= 8 (every tensor above with Z in place of 2): the 16x16x32 ping-pong kernel is the 8-wave
 * form at Z == 2 only, the 32x32x16 one at every other Z.  ups and res_half need Z == 2 (TM_ERR_ARG otherwise, as for a Z
 * out of range, before any device call).  tm_op_conv27_bf16 is this call with Z = 2. */
int tm_op_conv27_h16_z(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8,
                       int N, int Cin, int Cout, int S, int dtype, int waves, const void* res_h16, void* y_h16,
                       int ups, int res_half, int Z, void* stream);

/* Timing hook: `iters` launches of that conv in the forms the model uses (16-bit stream output, optional 16-bit
 * residual, fused norm epilogue, upsampled-input form) on random device data in [-1, 1); *ms_per_launch = mean launch
 * duration between two events after one warm-up launch.  waves: 0 | 4 | 8 as above, 9 = the lockstep 8-wave kernel
 * (kept for A/B against the ping-pong form that `8` selects). */
int tm_op_conv27_time(int N, int Cin, int Cout, int S, int dtype, int waves, int ups, int with_res, int fused,
                      int iters, float* ms_per_launch, void* stream);

/* The same conv with the ResBlock mid-section fused into its epilogue (Cout in {64, 128}): out_layers[0]
 * RMSNorm(C) * norm_w -> x * (1 + scale) + shift -> SiLU (model/MBAblocks.py:196-203,356-367), written as the 16-bit CB8
 * tensor a2_out [N][Cout/8][2][S][S][8] (the second conv's input).  norm_w [Cout], scale / shift [ceil(N/per_image)][Cout]
 * HOST fp32; patch n uses row n / per_image. */
int tm_op_conv27_fused(const void* x_cb8, const void* w_host, const void* bias_host, const void* norm_w_host,
                       const void* scale_host, const void* shift_host, void* a2_out, int N, int Cin, int Cout,
                       int S, int per_image, int dtype, int waves, void* stream);
/* The same on Z planes, 1 <= Z <= 8 (a2_out [N][Cout/8][Z][S][S][8]); tm_op_conv27_fused is this call with Z = 2. */
int tm_op_conv27_fused_z(const void* x_cb8, const void* w_host, const void* bias_host, const void* norm_w_host,
                         const void* scale_host, const void* shift_host, void* a2_out, int N, int Cin, int Cout,
                         int S, int per_image, int dtype, int waves, int Z, void* stream);

/* 16-bit 1x1x1 conv / Linear over '(z h w) c' tokens (x and w rounded to `dtype`, fp32 accumulate).  waves: 0 | 4 | 8
 * as above (two co-resident 4-wave workgroups per CU, or one 8-wave workgroup).  Epilogue (model/MBAblocks.py:486-489):
 * y = res + gate * gelu?(W x + b) with optional 16-bit CB8 `res_h16` / `gate_h16` and 16-bit output `y_h16`. */
int tm_op_conv1_bf16(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8,
                     int N, int Cin, int Cout, int Z, int S, int gelu, int dtype, int waves, const void* res_h16,
                     const void* gate_h16, void* y_h16, void* stream);

/* The same with the gate as a channel-block slice and / or at half resolution: gate_h16 is [N][gate_cbtot][Z][Sg][Sg][8], read
 * from block gate_cb0 on; Sg = S, or S / 2 with gate_half != 0 (read at (z, y >> 1, x >> 1); S a power of two >= 2).
 * tm_op_conv1_bf16 is this call with gate_half = 0, gate_cbtot = ceil(Cout/8), gate_cb0 = 0. */
int tm_op_conv1_h16_gate(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8,
                         int N, int Cin, int Cout, int Z, int S, int gelu, int dtype, int waves, const void* res_h16,
                         const void* gate_h16, void* y_h16, int gate_half, int gate_cbtot, int gate_cb0, void* stream);

/* The ResBlock skip conv as the 16-bit modes run it (model/MBAblocks.py:220-224,297 on x = th.cat((h, skip, rna), 1),
 * model/unet_ours.py:384,418, with to_collage :325-341 applied to the sources of the collage decoder): a 1x1x1 conv whose
 * input is the channel concat of nsrc (1..3) tensors READ IN PLACE -- the concat and the half-patch re-tiling are address
 * rules of the kernel's staging, not tensors.  x_cb8[i]: fp32 CB8 [Ni, cin[i], Z, S, S] (device), Ni = N for a plain
 * source, N / ((p1-1)(p2-1)) * p1 * p2 for a collaged one (collage[i] != 0: the source lives on the (p1 x p2) encoder
 * patch grid of each image and is read at the half-patch-shifted position).  w [Cout][sum cin] HOST.  Output fp32 CB8. */
int tm_op_conv1_concat(const void* const* x_cb8, const int* cin, const int* collage, int nsrc, const void* w_host,
                       const void* bias_host, void* y_cb8, int N, int Cout, int Z, int S, int p1, int p2,
                       int dtype, int waves, void* stream);

/* The block-input pass of the 16-bit modes on its own: th.cat of nsrc (1..3) sources (model/unet_ours.py:384,418) with
 * to_collage (:325-341) where collage[i] != 0, optional resampling (up2 = 1: nearest x2, Upsample, model/blocks.py:362-371,
 * sources at S/2; up2 = 2: the Downsample form of ResBlock(down=True), blocks.py:389-403 -- ONE plain source at 2S, every
 * source voxel normalised and activated with its own statistics, then the 2 x 2 average; raw_h16 = the 2 x 2 average of x), LlamaRMSNorm over the real channel count c_real (model/MBAblocks.py:21-43; norm_w_dev: device fp32 [padded C], or
 * null), modulation (mod 0 none; 1 per image: device fp32 scale / shift rows [b][mod_stride], image = n / per_image,
 * apply_conditions :356-367; 2 per voxel: 16-bit CB8 scale / shift tensors of the output geometry with patch stride
 * mod_stride elements, modulate :608-614), SiLU (act != 0).  Sources and outputs are 16-bit CB8 DEVICE tensors (dtype
 * TM_DTYPE_BF16 / TM_DTYPE_F16); out_h16 has ceil(Cb / 2) * 2 channel blocks (pad blocks zero), raw_h16 (optional) receives
 * the gathered, un-normalised input.  variant: 0 = the form the model picks, 1 = prep_kernel, 2 / 3 = prep_h16_kernel with one
 * wave / four waves per 64 voxels.  iters >= 1 launches; elapsed_ms (host, optional): mean time of launches 2..iters. */
int tm_op_prep_h16(const void* const* src_h16, const int* src_c, const int* collage, int nsrc, int N, int Z, int S,
                   int p1, int p2, int up2, const void* norm_w_dev, int c_real, int mod, const void* mod_scale,
                   const void* mod_shift, long mod_stride, int per_image, int act, int dtype, int variant,
                   void* out_h16, void* raw_h16, int iters, float* elapsed_ms, void* stream);

/* The fp32 block-input pass on its own, as tm_op_prep_h16 with fp32 CB8 DEVICE sources, out_cb8 and (optional) raw_cb8 of
 * exactly ceil-8 channel blocks per source: concat of nsrc (1..3) sources with to_collage where collage[i] != 0, up2 = 1 nearest
 * x2 (sources at S/2), LlamaRMSNorm over c_real channels (norm_w_dev: device fp32 [padded C], or null), modulation (mod 0 none;
 * 1 per image: device fp32 rows [b][mod_stride], image = n / per_image; 2 per voxel: fp32 CB8 scale / shift tensors with patch
 * stride mod_stride floats, of the output geometry or, mod_half != 0, of half its in-plane resolution, read at (z, y >> 1,
 * x >> 1)), SiLU (act != 0).  variant: 0 = the form the model picks, 1 = the four-wave kernels (two reads of every source above
 * 256 channels), 2 = the wide resident form, 16 waves per 64 voxels (one read; bit-identical to 1), which takes
 * 33..160 channel blocks: TM_ERR_ARG with a tm_last_error() text, before any device call, where it does not apply.
 * iters >= 1 launches; elapsed_ms (host, optional): mean time of launches 2..iters. */
int tm_op_prep_f32(const void* const* src_cb8, const int* src_c, const int* collage, int nsrc, int N, int Z, int S,
                   int p1, int p2, int up2, const void* norm_w_dev, int c_real, int mod, const void* mod_scale,
                   const void* mod_shift, long mod_stride, int mod_half, int per_image, int act, int variant,
                   void* out_cb8, void* raw_cb8, int iters, float* elapsed_ms, void* stream);

/* One block-input pass in any combination of tensor types the executor launches: tm_op_prep_f32's arguments with
 *   resample    0 same, 1 nearest x2 (sources at S / 2), 2 the 2 x 2 average (sources at 2 S; norm and SiLU per source voxel,
 *               then the mean), 3 pick (output (z, y, x) <- source (z, 2 y, 2 x) at 2 S, the collage remap in source coordinates);
 *   src_dtype, out_dtype, raw_dtype, mod_dtype (per-voxel tensors only): TM_DTYPE_F32 | TM_DTYPE_BF16 | TM_DTYPE_F16 CB8 DEVICE
 *               tensors; bf16 and f16 may not meet in one call; per-image rows are fp32;
 *   pad_blocks  all-zero channel blocks behind the last real one of a 16-bit `out` (and of a 16-bit `raw`): those tensors
 *               hold ceil-8 blocks per source + pad_blocks; an fp32 tensor holds exactly the ceil-8 blocks;
 *   variant     launch_prep's knob: 0 = the form the model takes, 1 = prep_kernel, 2 | 3 = prep_h16_kernel with one | four waves
 *               per 64 voxels (all-16-bit calls; 2: at most 32 blocks), 2 on an fp32 call = the wide form.
 * The call goes through the executor's launcher and nothing else: which kernel runs is part of what a test of it checks.
 * TM_ERR_ARG with a tm_last_error() text before any device call: the downsample form with a collage, a modulation or more than
 * one source; up2 with a collage; up2 or pick2 with an odd S; mixed 16-bit types; pad_blocks with an fp32 output; mod_half
 * without a per-voxel modulation or with an odd S; a variant whose form does not take the call. */
int tm_op_prep_form(const void* const* src, const int* src_c, const int* collage, int nsrc, int N, int Z, int S,
                    int p1, int p2, int resample, int src_dtype, int out_dtype, const void* norm_w_dev, int c_real,
                    int mod, int mod_dtype, const void* mod_scale, const void* mod_shift, long mod_stride, int mod_half,
                    int per_image, int act, int variant, int pad_blocks, void* out, void* raw, int raw_dtype,
                    int iters, float* elapsed_ms, void* stream);

/* The stem Conv3d(Cin -> Cout, (1, 3, 3), pad (0, 1, 1)) on its own (stem_kernel): x DEVICE fp32 NCHW '(s z) h w'
 * [N][Cin * Z][S][S]; w [Cout][Cin][1][3][3], bias [Cout] HOST, packed as the model loader packs them; y DEVICE CB8
 * [N][Cout / 8][Z][S][S][8] of `dtype` (fp32, bf16 or f16).  TM_ERR_ARG before any device call: Cout % 32, another dtype. */
int tm_op_stem(const void* x, const void* w_host, const void* bias_host, void* y, int N, int Cin, int Cout, int Z, int S,
               int dtype, void* stream);
/* The head Conv3d(C -> Cout, (1, 3, 3), pad (0, 1, 1)) on its own (head_kernel<dtype, 4 | 8>): x DEVICE CB8
 * [N][ceil(C / 8)][Z][S][S][8] of `dtype`, pad channels zero; w [Cout][C][1][3][3], bias [Cout] HOST; y DEVICE fp32 NCHW
 * [N][Cout * Z][S][S].  TM_ERR_ARG before any device call: Cout > 8, another dtype. */
int tm_op_head(const void* x_cb8, const void* w_host, const void* bias_host, void* y, int N, int C, int Cout, int Z, int S,
               int dtype, void* stream);
/* The timestep embedding on its own (time_embed_kernel): t DEVICE int64 [b]; w1 [E][ch], b1 [E], w2 [E][E], b2 [E] DEVICE fp32;
 * te = W2 silu(W1 sinusoid(t) + b1) + b2 and te_act = silu(te), DEVICE fp32 [b][E].  TM_ERR_ARG before any device call: odd
 * ch, more than 64 KB of ch + E floats. */
int tm_op_time_embed(const void* t_dev, const void* w1, const void* b1, const void* w2, const void* b2, void* te, void* te_act,
                     int b, int ch, int E, void* stream);
/* Every emb_layer as one matrix (emb_all_kernel): ss[b][tot] = wall [tot][E] te_act[b][E] + ball [tot], all DEVICE fp32.
 * TM_ERR_ARG before any device call: E % 64 != 0, E > 1024. */
int tm_op_emb_all(const void* te_act, const void* wall, const void* ball, void* ss, int b, int E, int tot, void* stream);

/* Windowed gene-patch cross attention core (model/MBAblocks.py:551-601 between the q/k/v Linears and proj):
 * q, k, v fp32 CB8 [N, C, Z, S, S]; qw, kw: device fp32 [C] (q_norm / k_norm weights).
 * dtype TM_DTYPE_F32: fp32 MFMA kernels, out = fp32 CB8.  TM_DTYPE_BF16: inputs are rounded to bf16 first (what the
 * bf16 q / kv Linears emit), out = bf16 CB8 [N][C/8][Z][S][S][8]. */
int tm_op_window_attn(const void* q_cb8, const void* k_cb8, const void* v_cb8, const void* qw_dev, const void* kw_dev,
                      void* out, int N, int C, int Z, int S, int dtype, void* stream);

/* The same core, reached the way the model reaches it: k and v are the two channel halves of ONE fp32 CB8 tensor
 * kv [N, 2C, Z, Sc, Sc] (channels [0, C) = k, [C, 2C) = v; the kv Linear's output), so their n stride differs from q's.
 * kv_half != 0: Sc = S / 2 and query token (z, y, x) reads k / v at (z, y >> 1, x >> 1) (the half-resolution conditioning
 * side); otherwise Sc = S.  dtype TM_DTYPE_F32: out = fp32 CB8.  TM_DTYPE_BF16 / TM_DTYPE_F16: q and kv are rounded to that
 * type on the device first, out = 16-bit CB8 [N][C/8][Z][S][S][8] of that type.
 * Every form the launchers do not take returns TM_ERR_ARG with a tm_last_error() text before any device call: C not a
 * multiple of 64, odd S, windows of more than 512 tokens; fp32: C > 512 (windows of 32 tokens with C % 128 == 0 excepted),
 * kv_half unless the window has 128 or 32 tokens, C % 128 == 0 and S is a power of two >= 4; 16-bit: C > 512, windows other
 * than 32 / 64 / 128 / 256 / 512 tokens, C > 256 or kv_half at 256 / 512 tokens, kv_half with S % 4 != 0. */
int tm_op_window_attn_kv(const void* q_cb8, const void* kv_cb8, const void* qw_dev, const void* kw_dev, void* out, int N, int C,
                         int Z, int S, int dtype, int kv_half, void* stream);

/* The gene-gene attention block (tm_attn.hip; model/MBAblocks.py:492-501, 551-601 with k = q) in one kernel form per call.
 *   rna_dense  DEVICE fp32 [B, gn, gn, zs * 500]: token g has D = gn^2 * zs features, feature z * gn^2 + hw read from
 *              [hw][z * 500 + slot(g)], slot(g) = gidx[g] (gidx HOST int32 [G], each in [0, 500)) or g without a table;
 *   w_host     twelve HOST fp32 arrays in checkpoint layout ([out][in]), in this order: attn.q.weight [D][D], attn.q.bias,
 *              attn.v.weight [D][D], attn.v.bias, attn.q_norm.weight, attn.proj.weight [D][D], attn.proj.bias, norm2.weight,
 *              mlp.fc1.weight [4D][D], mlp.fc1.bias [4D], mlp.fc2.weight [D][4D], mlp.fc2.bias;
 *   form       0 = the model's rule (the fused kernel iff D == 64, G <= 232 and no table), 1 = the fused D = 64 MFMA kernel,
 *              2 = the generic kernel (G <= 512, D <= 512; its scratch is allocated inside the call);
 *   zlo, zhi   slices outside [zlo, zhi) count as zero (the slice-pair maps of tm_gene_attn); 0, zs: none;
 *   out_tok    DEVICE fp32 CB8 [B][ceil(G/8)][zs][gn][gn][8] or NULL: the block's output; the pad slots g >= G are not written;
 *   attn_map   DEVICE fp32 [B][G][G] or NULL: the softmax.  At least one of the two outputs.
 * TM_ERR_ARG with a tm_last_error() text before any device call: a null pointer, B / gn / zs / G < 1, D > 512, G > 512, G > 500
 * without a table, a table entry outside [0, 500), a mask outside [0, zs]; form 1 with gn^2 * zs != 64, G > 232 or a table. */
int tm_op_gene_attn(const void* rna_dense_dev, const void* const* w_host, const int* gidx_host, int B, int gn, int zs, int G,
                    int form, int zlo, int zhi, void* out_tok_cb8, void* attn_map, void* stream);
/* rna_mid of tm_gene_attn alone: out DEVICE fp32 [B, G, zs - 2, gn, gn]; zs <= 2 writes nothing and succeeds. */
int tm_op_rna_mid(const void* rna_dense_dev, int B, int gn, int zs, int G, void* out, void* stream);
/* The pathway read-out of tm_gene_attn_readout (out [B, 4K, 2 gn^2], sub [4, B, K, K] or NULL, glst K HOST indices) in one form:
 * 0 = the model's rule, 1 = the fused kernel (gn = 4, zs = 4, G <= 232, no table), 2 = the generic map kernel over chunks of 8
 * patches and the gather kernel.  rna_dense, w_host, gidx_host and the refusals as for tm_op_gene_attn; also zs != 4, K outside
 * [1, 8] and a glst entry that repeats or lies outside [0, G). */
int tm_op_gene_readout(const void* rna_dense_dev, const void* const* w_host, const int* gidx_host, int B, int gn, int zs, int G,
                       const int* glst, int K, int form, void* out, void* sub, void* stream);

/* Generic direct Conv3d (stem / head / RNA path), NCDHW in, NCDHW out. */
int tm_op_conv_direct(const void* x, const void* w_host, const void* bias_host, void* y, int N,
                      int Cin, int Cout, int Zin, int S, int kz, int ky, int kx, int pz, int py,
                      int px, int silu_in, int up2_out, void* stream);

/* ---- training slice: the pieces of ONE ResBlock's training step ---------------------------------
 * ResBlock._forward in training mode (model/MBAblocks.py:237-299) is
 *   A = SiLU(RMSNorm(x) w1);  H1 = Conv3d(A);  D = Dropout(SiLU(RMSNorm(H1) w2 (1 + scale) + shift));  out = skip(x) + Conv3d(D)
 * and its backward is composed of the entry points below (teramind_amd.training.ResBlockTrain does the composition; the
 * gradient of every piece is checked against torch.autograd of the oracle, tests/test_gpu_train.py).  fp32, CB8 tensors. */

/* y = Dropout(SiLU(RMSNorm_C(x) * norm_w * (1 + scale[img]) + shift[img])) with a SUPPLIED keep mask (fp32 CB8 0/1, or NULL
 * = no dropout; nn.Dropout(p=0.1) draws it in the reference, config_parm.py:46) and drop_scale = 1 / (1 - p).
 * norm_w [C], scale / shift [ceil(N / per_image)][C] HOST (or both NULL: in_layers). */
int tm_op_prep_train(const void* x_cb8, const void* norm_w_host, const void* scale_host, const void* shift_host,
                     const void* mask_cb8, float drop_scale, int per_image, void* y_cb8, int N, int C, int Z, int S,
                     void* stream);

/* Backward of the above: g = dL/dy (CB8) -> dx (CB8), dL/dnorm_w [C], dL/dscale, dL/dshift [nimg][C] (HOST outputs). */
int tm_op_prep_bwd(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_host,
                   const void* shift_host, const void* mask_cb8, float drop_scale, int per_image, void* dx_cb8,
                   void* dw_host, void* dscale_host, void* dshift_host, int N, int C, int Z, int S, void* stream);

/* ResBlock dropout with the keep mask DRAWN on the GPU: element (n, c, z, y, x) of a [N, C, Z, S, S] activation is
 * dropped iff output word c & 3 of Philox4x32-10(counter (v lo, v hi, site, c >> 2), key (key lo, key hi)) < min(floor(p 2^32),
 * 2^32 - 1), v = ((n Z + z) S + y) S + x; kept elements are scaled by 1 / (1 - p).  0 <= p < 1; p = 0 is the no-dropout path.
 * The forward and its backward draw the same mask from (key, site, p): no mask is stored.  Arguments otherwise as above. */
int tm_op_prep_train_rng(const void* x_cb8, const void* norm_w_host, const void* scale_host, const void* shift_host,
                         unsigned long long key, unsigned site, float p, int per_image, void* y_cb8, int N, int C, int Z, int S,
                         void* stream);
int tm_op_prep_bwd_rng(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_host,
                       const void* shift_host, unsigned long long key, unsigned site, float p, int per_image, void* dx_cb8,
                       void* dw_host, void* dscale_host, void* dshift_host, int N, int C, int Z, int S, void* stream);
/* The keep mask of the two entry points above as an fp32 CB8 tensor [N][ceil(C/8)][Z][S][S][8] of 0 / 1 (pad channels 0): the
 * supplied-mask ops given this mask compute what the drawing ones compute.  Tests and debugging. */
int tm_op_dropout_mask(unsigned long long key, unsigned site, float p, void* mask_cb8, int N, int C, int Z, int S, void* stream);

/* dL/dx of Conv3d(k = 3x3x3 pad 1 (ksize 3) | 1x1x1 (ksize 1)): dy CB8 [N, Cout, Z, S, S] -> dx CB8 [N, Cin, Z, S, S];
 * w [Cout][Cin][k^3] HOST as in the reference state_dict.  Runs on the forward MFMA conv kernel with re-packed weights. */
int tm_op_conv_dgrad(const void* dy_cb8, const void* w_host, void* dx_cb8, int N, int Cin, int Cout, int Z, int S,
                     int ksize, void* stream);

/* dL/dw [Cout][Cin][k^3] and dL/dbias [Cout] (HOST outputs; db may be NULL) of the same convs. */
int tm_op_conv_wgrad(const void* x_cb8, const void* dy_cb8, void* dw_host, void* db_host_or_null, int N, int Cin,
                     int Cout, int Z, int S, int ksize, void* stream);

/* ---- resident conv ops of the training tape: weights packed on the device once, gradients to DEVICE pointers.  None of these
 * synchronises `stream` or touches host memory (scratch is stream-ordered); bad arguments return TM_ERR_ARG before any device call.
 *   role 0: the forward pack of w [Cout][Cin][k^3] (DEVICE, reference layout) -- the bytes tm_op_conv_mfma(zmode 0) packs on the host,
 *           the pair form (W1, W2 - W1, W0 - W1) at ksize 3, Z == 2;
 *   role 1: the pack tm_op_conv_dgrad builds: the filter flipped in z, y, x with cin <-> cout transposed. */
long tm_conv_pack_floats(int Cout, int Cin, int ksize, int Z, int role);      /* floats of one pack; -1: bad argument */
int tm_op_conv_pack_dev(const void* w_dev, void* pack_dev, int Cout, int Cin, int ksize, int Z, int role, void* stream);
/* tm_op_conv_mfma(..., zmode 0, up2 0, variant 0) on a role-0 pack; bias_dev [Cout] DEVICE.  Z 1 .. 4 or 8 here, in the data gradient
 * and in the weight gradient below (Z = 8: rna_slc 16); 5, 6, 7 are refused before any launch. */
int tm_op_conv_mfma_packed(const void* x_cb8, const void* pack_dev, const void* bias_dev, void* y_cb8, int N, int Cin, int Cout,
                           int Z, int S, int ksize, void* stream);
/* tm_op_conv_dgrad on a role-1 pack; Z 1 .. 4 or 8 */
int tm_op_conv_dgrad_packed(const void* dy_cb8, const void* pack_dev, void* dx_cb8, int N, int Cin, int Cout, int Z, int S,
                            int ksize, void* stream);
/* dL/dw [Cout][Cin][k^3] and dL/dbias [Cout] (may be NULL) to DEVICE pointers, on the fp32 MFMA pipe; accumulate 1 adds into what
 * is there.  Z 1 .. 4 or 8, square S x S planes: up to Z = 4 a spatial tile holds every z plane; Z = 8 runs the slab form (z tiled
 * in slabs of 4 output planes, 6 staged input planes).  Partial sums over chunks of the tile list are added in chunk order (no
 * atomics); the chunk count depends on (N, Z, S, Cin, Cout) only, so every run on every device gives the same bits. */
int tm_op_conv_wgrad_dev(const void* x_cb8, const void* dy_cb8, void* dw_dev, void* db_dev_or_null, int accumulate, int N,
                         int Cin, int Cout, int Z, int S, int ksize, void* stream);

/* Timing hook (tools/bench_train.py): the weight gradient of one layer on random device data, engine 0 = the VALU kernel of
 * tm_op_conv_wgrad, 1 = the MFMA kernel of tm_op_conv_wgrad_dev (with its chunk reduction).  After one warm-up launch,
 * ms_per_launch_host[r], r < reps, is the time per launch of `iters` launches between two events.  Z as tm_op_conv_wgrad_dev for
 * engine 1, 1 .. 4 for engine 0. */
int tm_op_conv_wgrad_time(int N, int Cin, int Cout, int Z, int S, int ksize, int engine, int iters, int reps,
                          float* ms_per_launch_host, void* stream);

/* ---- training slice, AttnBlock (model/MBAblocks.py:428-514 AttnBlock.forward, :517-601 Attention, :608-614 modulate) -----
 *   m = adaLN(SiLU(y));  (shift, scale, gate) x (msa, mlp) = m.chunk(6)
 *   x = x + gate_msa * proj(core(q(modulate(norm1(x))), k(y), v(y)));   x = x + gate_mlp * fc2(GELU(fc1(modulate(norm2(x)))))
 * Every Linear is a 1x1x1 conv (tm_op_conv_mfma / tm_op_conv_dgrad / tm_op_conv_wgrad with ksize 1); the pieces below are the
 * rest.  fp32 CB8 device tensors, norm weights HOST.  teramind_amd.training.AttnBlockTrain composes forward and backward;
 * tests/test_gpu_train.py checks every gradient against the reference module's own autograd (tests/golden/train_attn_ref.npz). */

/* Elementwise on n floats: op 0 o1 = a + b * c | 1 o1 = a * b, o2 = a * c | 2 o1 = gelu_tanh(a) | 3 o1 = a * gelu_tanh'(b) |
 * 4 o1 = silu(a) | 5 o1 = a * silu'(b) | 6 o1 = a + b | 7 o1 = 4 a | 8 o1 = a / 4. */
int tm_op_ew(int op, const void* a, const void* b, const void* c, void* o1, void* o2, long n, void* stream);

/* y = RMSNorm_C(x) * norm_w * (1 + scale) + shift with per-voxel scale / shift (CB8 tensors of x's geometry). */
int tm_op_modnorm(const void* x_cb8, const void* norm_w_host, const void* scale_cb8, const void* shift_cb8, void* y_cb8,
                  int N, int C, int Z, int S, void* stream);

/* Backward of the above: g = dL/dy -> dx, dscale, dshift (CB8) and dL/dnorm_w [C] (HOST). */
int tm_op_modnorm_bwd(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_cb8, void* dx_cb8,
                      void* dscale_cb8, void* dshift_cb8, void* dw_host, int N, int C, int Z, int S, void* stream);

/* The attention core (q/k RMSNorm, softmax(q k^T / C) v per 2 x 2 window over (h, w) and all z; one head, n_h = 2):
 * dout_cb8 == NULL: forward, writes o_cb8.  dout_cb8 != NULL: backward, writes dq / dk / dv (CB8) and the q/k norm weight
 * gradients [C] (HOST).  Windows of 4, 8 or 16 tokens, C <= 512 (one workgroup per patch, one wave per window), of 32, 64 or
 * 128 tokens, C <= 512 (one workgroup per window, P in LDS), and of 256 or 512 tokens, C <= 256 (key-blocked fp32 MFMA kernels,
 * no T x T matrix anywhere; C > 256 is refused).  Any other token count is TM_ERR_ARG.  C need not be a multiple of 8; the pad
 * channels of the last CB8 block are written as zeros (and, at 4 - 16 and 256 / 512 tokens, never read as values on the input
 * side: whatever q, k, v, dout hold there changes no bit).  Deterministic. */
int tm_op_window_attn_train(const void* q_cb8, const void* k_cb8, const void* v_cb8, const void* qw_host,
                            const void* kw_host, const void* dout_cb8, void* o_cb8, void* dq_cb8, void* dk_cb8,
                            void* dv_cb8, void* dqw_host, void* dkw_host, int N, int C, int Z, int S, void* stream);

/* ---- training slice, the small dense pieces: time embedding (model/unet_ours.py:442-476), ResBlock.emb_layers
 * (model/MBAblocks.py:178-186) and the gene-gene AttnBlock of the RNA pyramid (model/unet_ours.py:277-323) are Linears over
 * [tokens][features] rows.  DEVICE pointers throughout (fp32), deterministic. */

/* C[b](m, n) = alpha * sum_k A[b](m, k) B[b](k, n) (+ bias[n] if bias_mode 1, bias[m] if 2) (+ C if accumulate), every operand
 * addressed through element strides strides9 = {sam, sak, sbk, sbn, scm, scn, sab, sbb, scb} (HOST array). */
int tm_op_gemm_f32(const void* A_dev, const void* B_dev, const void* bias_dev, void* C_dev, int M, int N, int K,
                   const long* strides9_host, int batch, int bias_mode, int accumulate, float alpha, void* stream);

/* Row-wise ops on [rows][D]: 0 y = RMSNorm_D(x) * w | 1 y = dL/dx of op 0 given g (and dw_dev[D] = dL/dw) | 2 y = softmax_D(x) |
 * 3 y = x * (g - sum_D(g x)) (softmax backward, x = the saved probabilities). */
int tm_op_rows(int op, const void* x_dev, const void* w_dev, const void* g_dev, void* y_dev, void* dw_dev, long rows, int D,
               void* stream);

/* (h, w) resampling of a CB8 tensor: mode 1 nearest x2 (source at S_out / 2), mode 2 AvgPool(1,2,2) (source at 2 S_out)
 * (model/blocks.py:362-403). */
int tm_op_resample(const void* x_cb8, void* y_cb8, int N, int C, int Z, int S_out, int mode, void* stream);

/* ---- training slice, the optimizer step (experiment.py:207-219 clip_grad_norm_, :394-414 torch.optim.Adam) on one flat fp32
 * device arena of parameters / gradients / first and second moments. */

/* *out_host = sum of x[i]^2 (two-stage, fixed order). */
int tm_op_sumsq(const void* x_dev, long n, float* out_host, void* stream);

/* One torch.optim.Adam step (amsgrad off): g' = g * grad_scale + weight_decay * p; m, v, p updated in place; step >= 1. */
int tm_op_adam(void* p_dev, const void* g_dev, void* m_dev, void* v_dev, long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ---- data-parallel training: the rank-ordered sum of the gradient exchange (teramind_amd.train_dist.GradExchange) ---------- */

/* parts_dev [W][n] fp32 contiguous -> out_dev [n]:  out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...  -- plain fp32
 * additions in slice order, starting from slice 0's value and not from zero (W = 1 is a bit copy; -0.0 stays -0.0).  One owner
 * thread per element, no atomics: the same inputs give the same bits on every device.  Queued on `stream`; nothing is
 * synchronised.  1 <= W <= 64, n >= 0 (n = 0: nothing is written).  out_dev must not overlap parts_dev: an overlapping call, a
 * null pointer or a bad W / n is TM_ERR_ARG before any launch.  Pointers need 4-byte alignment; 16-byte aligned pointers with
 * n % 4 == 0 give aligned 16-byte accesses throughout. */
int tm_op_rank_sum(const void* parts_dev, void* out_dev, int W, long n, void* stream);

/* Timing hook (tools/bench_rank_sum.py): tm_op_rank_sum's kernel on random device data.  After one warm-up launch,
 * ms_per_launch_host[r], r < reps, is the time per launch of `iters` launches between two events.  Z as tm_op_conv_wgrad_dev for
 * engine 1, 1 .. 4 for engine 0. */
int tm_op_rank_sum_time(int W, long n, int iters, int reps, float* ms_per_launch_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TERAMIND_HIP_H */
