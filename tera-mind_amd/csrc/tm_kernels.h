// Internal launcher interface between the host side (the executor tm_model.hip, the single-operator
// hooks tm_ops.hip) and the kernels.  Not part of the public ABI (include/teramind_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/teramind_hip.h"

namespace tmk {

// CB8 activation tensor view: fp32 [N][Cb][Z][H][W][8]; channel c lives in block c/8,
// slot c%8; padded slots are kept at exactly 0.
struct TV {
  float* p = nullptr;
  int N = 0, C = 0, Cb = 0, Z = 0, H = 0, W = 0;
  long nstride = 0;                 // floats between consecutive n (>= Cb*Z*H*W*8)
  long plane() const { return (long)Z * H * W * 8; }   // floats per channel block
  // view of channel blocks [cb0, cb0+ncb) (C is set to ncb*8)
  TV blocks(int cb0, int ncb) const {
    TV v = *this;
    v.p = p + (long)cb0 * plane();
    v.Cb = ncb;
    v.C = ncb * 8;
    return v;
  }
};
// a dense CB8 tensor at p: the one place that computes Cb and nstride (p == nullptr: a geometry-only descriptor)
inline TV cb8_view(void* p, int N, int C, int Z, int H, int W) {
  TV t;
  t.p = (float*)p; t.N = N; t.C = C; t.Cb = (C + 7) / 8; t.Z = Z; t.H = H; t.W = W;
  t.nstride = (long)t.Cb * t.plane();
  return t;
}
inline int pair_cb(int cb) { return (cb + 1) / 2 * 2; }   // the even block count of a 16-bit conv operand (zero pad block)

// ---- packed conv weights for the MFMA implicit-GEMM kernels ----------------------------
// layout: [n_tile][cblk][tap][64 cout][8 cin] fp32, cout padded to a multiple of 64,
// cin padded per concat segment to multiples of 8 ("virtual" cin order).
// The form of a conv: which kernel reads the pack, hence its tap count and layout.  Decided by conv_pick_form and nowhere else.
enum ConvForm {
  CF_1X1 = 0,        // 1x1x1 conv / Linear (conv1_mfma), 1 tap
  CF_INPLANE,        // 9 in-plane taps on one plane: 1x3x3, or the centre slice of a 3x3x3 pad-1 conv at Z == 1 (conv3d_mfma<1>)
  CF_PLANES3,        // 27 taps over three staged planes: pad 1 (any Z but 2) or valid in z, by ConvLaunch.zmode (conv3d_mfma<3>)
  CF_ZSKIP,          // the same 27-tap pack at Z == 2: 18 of the 27 taps per output plane (conv3d_mfma<2>)
  CF_ZSKIP_UPS,      // z-skip of the nearest-x2 upsampled input: 4 phases x 12 phase-sum taps (conv3d_mfma<2, .., true>)
  CF_PAIR,           // pair form at Z == 2: W1, W2 - W1, W0 - W1, 27 taps (conv3d_zpair)
  CF_PAIR_UPS,       // pair form of the upsampled input: the z difference of the phase sums, 4 x 12 taps (conv3d_zpair_ups)
  CF_XQUAD,          // pair form in z with Winograd F(4,3) along x: 54 transformed taps, 32-cout tiles (conv3d_xquad)
};
struct ConvW {
  const float* w = nullptr;     // device
  const float* bias = nullptr;  // device, [ntile*64]
  int Cout = 0, Cbi = 0, taps = 0, ntile = 0;     // taps = conv_form_taps(form): set by conv_w only
  int form = CF_1X1;
};
int conv_form_taps(int form);                            // taps per (cout tile, cin block) of the pack: 1 / 9 / 27 / 12 / 54
size_t conv_pack_floats(int form, int Cout, int Cbi);    // floats of the whole pack (the upsampled forms hold four phases)
ConvW conv_w(int form, int Cout, int Cbi);               // the weight geometry of a form; w / bias are left for the caller
// Which form a conv runs in, from what its caller knows: the kernel size (1 or 3), the z semantics (ZM_*), the input planes Z,
// whether the model's deepest plane is at least 8 x 8 (the x-quad kernel has no 4 x 4 tile) and the role of the layer.  The one
// reader of the A/B switches TM_CONV_ZPAIR, TM_CONV_XQUAD and TM_CONV_FUSE_MID (each read once; =0 switches the form off, for
// timing in separate processes only: TM_CONV_XQUAD=0 leaves its layers on the pair form).  *fuse_mid (nullable): the layer runs
// the ResBlock mid-section in its epilogue wherever a launch takes the 128-voxel tile.
enum { ROLE_OP = 0,             // single-operator hooks and the training tape: pair form at Z == 2, never x-quad
       ROLE_RES = 1,            // a ResBlock 3x3x3 conv of the executor: centre slice at Z == 1; at Z == 2 x-quad, or pair
                                //   (TM_CONV_XQUAD=0)
       ROLE_DEEP = 2,           // + a decoder block of the deepest level: x-quad only with its K loop split over workgroups
                                //   (xquad_ksplit); TM_CONV_XQUAD_SPLIT=0 keeps it on the pair form
       ROLE_C1_64 = 4,          // + the first conv of a 64-channel block: on the pair form it runs the fused mid-section
       ROLE_OP_PAIR_UPS = 16,   // the hook of the upsampled pair form: under no switch
       ROLE_OP_XQUAD = 32 };    // the hooks of the x-quad form: under TM_CONV_XQUAD alone
int conv_pick_form(int ksize, int zmode, int Z, bool deep8, int role, bool* fuse_mid = nullptr);
// host-side packing (tm_conv_pack.cpp); w [Cout][Cin][9 (CF_INPLANE) | 1 (CF_1X1) | 27], seg_c[i] = real channels of concat
// segment i (each padded to x8)
void conv_pack_host(int form, const float* w, int Cout, const int* seg_c, int nseg, float* out);
void vec_pack_host(const float* v, const int* seg_c, int nseg, float* out);  // per-cin vector -> virtual order
void transpose_host(const float* w, int rows, int cols, float* out);         // [rows][cols] -> [cols][rows] (Linear weights of GeneW)
// the direct kernels' weights (conv_direct, stem, head): w [Cout][Cin][taps] -> out [taps][Cin][ceil(Cout / 8) * 8], pad couts zero
void direct_pack_host(const float* w, int Cout, int Cin, int taps, float* out);

enum { EPI_NONE = 0, EPI_GELU = 1, EPI_UP2 = 2 };
enum { ZM_PAD1 = 0, ZM_INPLANE = 1, ZM_VALID = 2,    // z structure of a k x 3 x 3 conv (see conv3d_mfma)
       ZM_UPS = 3 };                                   // 3x3x3 pad 1 of nearest-x2 upsampled x, computed on x (phase weights)
struct ConvLaunch {
  TV x;                  // activated input, Cb == w.Cbi
  ConvW w;
  TV y;                  // output (for EPI_UP2: H,W = 2*x.H)
  const TV* res = nullptr;   // optional residual (same geometry as y)
  const TV* gate = nullptr;  // optional gate: y = res + gate * (conv + bias)
  int flags = 0;
  int tile_variant = 0;  // 0 auto, 1 = 128-voxel blocks, 2 = 256-voxel blocks; CF_1X1 also 3 = the 128-cout tile (conv1_form)
  int gate_half = 0;     // CF_1X1 only: `gate` lives at S/2 and is read at (z, y >> 1, x >> 1) (S a power of two)
  int res_half = 0;      // k x 3 x 3 only: `res` lives at S/2 and is read at (z, y >> 1, x >> 1): the residual of a ResBlock(up=True)
                         // is the nearest-x2 upsampled block input (model/MBAblocks.py:254-258,297)
  int zmode = ZM_PAD1;   // the caller's statement of the z semantics; must agree with w.form (ignored for CF_1X1)
  int xquad_sched = -1;  // CF_XQUAD only: 0 = the four-barrier schedule of conv3d_xquad, 1 = the pipelined one, -1 = the launcher's
                         // choice per instantiation and launch size (TM_CONV_XQUAD_PIPE=0: the four-barrier schedule everywhere)
  // CF_XQUAD only: split K.  1 = one workgroup runs the whole K loop; 2 | 4 = that many workgroups per (voxel tile, cout tile),
  // each over its own range of cin blocks, their raw sums in `part` (xquad_part_floats(...) floats), then xquad_split_reduce adds
  // them, the bias, the GELU flag and the residual into y.  The caller decides (xquad_ksplit is the rule); no res_half
  int xquad_ksplit = 1;
  float* part = nullptr;
  // CF_PAIR, Cout == 64, the 128-voxel tile, no residual / gate / flags: fuse RMSNorm(C) * norm_w -> x (1 + scale) +
  // shift -> SiLU into the epilogue and write `a2` (the next conv's input) instead of y; y carries the geometry only
  int fuse_norm = 0;
  const float *norm_w = nullptr, *mod_scale = nullptr, *mod_shift = nullptr;
  float inv_c = 0.f;
  long mod_stride = 0;
  int per_image = 1;
  TV a2;
};
hipError_t launch_conv_mfma(const ConvLaunch& L, hipStream_t s);
// The tile of a k x 3 x 3 launch of `ovox` output voxels (N * Z * S * S of the launched plane): 2 = the large tile (256 voxels; 128
// in the pair forms, 128 four-column groups in the x-quad form), 1 = the small one.  tile_variant 0 chooses by launch size
// (conv_fills_chip), 1 / 2 force it; a 4 x 4 plane has the small tile only; the x-quad form takes its large tile from 256 large
// workgroups on, except at S >= 64 from 2048 on.  The one statement of the rule, for the launcher and for whoever must know the
// tile beforehand (the fused mid-section exists in the large tile only).  No device call.
int conv_tile(int form, long ovox, int ntile, int S, int tile_variant);
// The split-K factor of an x-quad launch of ovox = N * 2 * S * S output voxels, Cout couts and Cbi cin blocks: 1 where the
// launch has 256 large workgroups or more, with res_half and with TM_CONV_XQUAD_SPLIT=0 (xquad_split_on, read once); otherwise 2
// where the launch has fewer than XQUAD_SPLIT_WGS small-tile workgroups and both splits keep XQUAD_SPLIT_FLOOR cin blocks (4
// is a factor of the kernel and the hooks; the rule never takes it).  A pure function of the shapes: the dry pass and the real
// pass agree.  It is the rule of a launch on its own (the hooks, the op table).  The executor gives the factor to the layer, not
// to the launch: the decoder blocks of the deepest level take 2 at every patch count (split_k, tm_model.hip).  No device call.
constexpr int XQUAD_SPLIT_WGS = 256, XQUAD_SPLIT_FLOOR = 4;
int xquad_ksplit(long ovox, int Cout, int Cbi, int S, bool res_half);
bool xquad_split_on();
// floats of the partial sums of a split launch into y: ksplit slices of y's own geometry
inline size_t xquad_part_floats(int ksplit, const TV& y) { return ksplit > 1 ? (size_t)ksplit * y.N * y.nstride : 0; }
// byte addresses in LDS of the 64 lanes of wave wv for one fragment read or staging store of conv3d_zpair (kernel 0),
// conv3d_zpair_ups (1), conv3d_xquad (4; 2 and 3 are no kernels: waves 0 .. 7 in the large tile, kx = the wave's q 0 .. 2, in a
// staging store the q-plane 0 .. 5), its pipelined schedule (5: as 4, `sub` = the plane set 0 | 1 of an X fragment or a staging store),
// instantiation <half, tw> (tm_kernels.hip); -1: no such thing; no device call
int conv_frag_addrs(int kernel, int half, int tw, int what, int wv, int p, int ky, int kx, int sub, int* out);
// the dynamic LDS of conv3d_xquad<half, tw> in schedule sched (0 | 1), bytes; -1: no such instantiation; no device call
int conv_xquad_lds_bytes(int half, int tw, int sched);
// which conv1_mfma instantiation a CF_1X1 launch takes (1 <1, 2>, 2 <2, 2>, 3 <2, 4>; 0 = refused); no device call
int conv1_form(long vox, int ntile, int tile_variant);

// ---- bf16 3x3x3 conv (tm_conv_bf16.hip) --------------------------------------------------
struct TVH {                        // bf16 CB8 tensor [N][Cb (even)][Z][H][W][8]; strides in elements
  uint16_t* p = nullptr;
  int N = 0, C = 0, Cb = 0, Z = 0, H = 0, W = 0;
  long nstride = 0;
  TVH blocks(int cb0, int ncb) const {          // channel-block slice sharing the storage
    TVH t = *this;
    t.p = p + (long)cb0 * Z * H * W * 8;
    t.Cb = ncb; t.C = ncb * 8;
    return t;
  }
};
struct ConvLaunchH {
  TVH x;
  const uint16_t* w = nullptr;      // packed by conv_bf16_pack_host
  const float* bias = nullptr;      // [ceil(Cout/64)*64] fp32
  int Cout = 0;
  TV y;                             // fp32 CB8 output (geometry is also used for the bf16 output)
  const TV* res = nullptr;
  const TV* gate = nullptr;         // conv1 only
  const TVH* gate_h = nullptr;      // conv1 only: bf16 gate instead of `gate`
  int flags = 0;                    // conv1 only: EPI_GELU
  uint16_t* y_h = nullptr;          // write 16-bit CB8 INSTEAD of y (the 16-bit activation stream / next Linear's input)
  long yh_nstride = 0;
  const TVH* res_h = nullptr;       // 16-bit CB8 residual instead of `res`
  // conv27 only, Cout in {64, 128}: fuse RMSNorm(C)*w -> x(1+scale)+shift -> SiLU into the epilogue and write
  // the bf16 tensor `a2` (the next conv's input) instead of y
  int fuse_norm = 0;
  const float *norm_w = nullptr, *mod_scale = nullptr, *mod_shift = nullptr;
  long mod_stride = 0;
  int per_image = 1;
  TVH a2;
  int force_waves = 0;              // 0 = auto, 4 | 8 = workgroup form (tests / A-B; TM_CONV27_WAVES, TM_CONV1_WAVES)
  int gate_half = 0;                // conv1 only: gate_h lives at S/2 and is read at (z, y >> 1, x >> 1) (S a power of two)
  int res_half = 0;                 // conv27 only: res_h lives at S/2 and is read at (z, y >> 1, x >> 1)
  int ups = 0;                      // conv27 only: x is the LOW-resolution tensor (y.H == 2 x.H), w = conv_bf16_pack_ups_host weights:
                                    // the conv of the nearest-x2 upsampled x (Cout a multiple of 128, Z == 2, no residual)
  // conv1 only: input = channel concat of nsrc (1..3) 16-bit CB8 tensors read in place, each optionally through the collage
  // remap of a (p1 x p2) source patch grid; `x` then only carries N, Z, H, W and the even-padded block count (x.p unused)
  int nsrc = 0;
  TVH xs[3];
  int xs_collage[3] = {0, 0, 0};
  int p1 = 0, p2 = 0;
};
hipError_t init_bf16_device();      // per-device set-up that must not happen lazily inside a stream capture
hipError_t init_f16_device();
int conv_bf16_tn(int Cout);
size_t conv1_bf16_pack_elems(int Cout, int Cbi);
void conv1_bf16_pack_host(const float* w, int Cout, const int* seg_c, int nseg, uint16_t* out);
hipError_t launch_conv1_bf16(const ConvLaunchH& L, hipStream_t s);
size_t conv_bf16_pack_elems(int Cout, int Cbi);
void conv_bf16_pack_host(const float* w, int Cout, const int* seg_c, int nseg, uint16_t* out);
size_t conv_bf16_pack_ups_elems(int Cout, int Cbi);
void conv_bf16_pack_ups_host(const float* w, int Cout, const int* seg_c, int nseg, uint16_t* out);
void conv_f16_pack_ups_host(const float* w, int Cout, const int* seg_c, int nseg, uint16_t* out);
hipError_t launch_conv27_bf16(const ConvLaunchH& L, hipStream_t s);
hipError_t launch_window_attn_bf16(const TVH& q, const TVH& k, const TVH& v, const float* qnorm_w, const float* knorm_w,
                                   TVH o, hipStream_t s);
// IEEE-half twins of the five functions above (tm_conv_bf16.hip built with -DTM_H16_F16): same layouts, fp16 elements
void conv1_f16_pack_host(const float* w, int Cout, const int* seg_c, int nseg, uint16_t* out);
hipError_t launch_conv1_f16(const ConvLaunchH& L, hipStream_t s);
void conv_f16_pack_host(const float* w, int Cout, const int* seg_c, int nseg, uint16_t* out);
hipError_t launch_conv27_f16(const ConvLaunchH& L, hipStream_t s);
hipError_t launch_window_attn_f16(const TVH& q, const TVH& k, const TVH& v, const float* qnorm_w, const float* knorm_w,
                                  TVH o, hipStream_t s);

// ---- prep: concat + resample + RMSNorm(C) * w -> modulate -> act ---------------------
struct PrepSrc {
  const float* p = nullptr;
  long nstride = 0;
  int Cb = 0;
  int collage = 0;
};
enum { RS_SAME = 0, RS_UP2 = 1, RS_DOWN2 = 2,
       RS_PICK2 = 3 };   // output (z, y, x) at S <- source (z, 2y, 2x) at 2S (then the collage remap, if any): the distinct values of
                         // a nearest-x2 upsampled tensor
enum { MOD_NONE = 0, MOD_IMAGE = 1, MOD_VOXEL = 2 };
struct PrepLaunch {
  PrepSrc src[3];
  int nsrc = 1;
  int resample = RS_SAME;
  int N = 0, Z = 0, S = 0;          // OUTPUT patches / plane size
  int p1 = 0, p2 = 0;               // source patch grid per image (collage only)
  const float* norm_w = nullptr;    // [Cbtot*8] virtual order, or null (no norm)
  float inv_c = 0.f;                // 1 / real channel count
  int mod = MOD_NONE;
  const float* mod_scale = nullptr; // MOD_IMAGE: [b][..] row stride mod_stride; MOD_VOXEL: CB8 tensor
  const float* mod_shift = nullptr;
  long mod_stride = 0;              // MOD_IMAGE: floats per image row; MOD_VOXEL: nstride
  const uint16_t* mod_scale_h = nullptr;   // MOD_VOXEL with a bf16 CB8 modulation tensor (instead of mod_scale/shift)
  const uint16_t* mod_shift_h = nullptr;
  int mod_half = 0;                 // MOD_VOXEL: the modulation tensors live at S/2 and are read at (z, y >> 1, x >> 1)
  int per_image = 1;                // output patches per image (n -> image index)
  int act = 0;                      // 1 = SiLU
  float* out = nullptr;
  long out_nstride = 0;
  float* raw = nullptr;             // optional un-normalised (resampled, concatenated) copy
  long raw_nstride = 0;
  uint16_t* out_h = nullptr;        // bf16 output instead of `out` (conv27_bf16 input), nstride in elements
  long out_h_nstride = 0;
  int pad_blocks = 0;               // extra all-zero channel blocks appended to the bf16 output (pair padding)
  uint16_t* raw_h = nullptr;        // bf16 instead of `raw` (input of the bf16 skip conv); same pad_blocks
  long raw_h_nstride = 0;
  int h_f16 = 0;                    // the 16-bit tensors (out_h, raw_h, mod_*_h, sources with src_h) are IEEE half instead of bf16
  int src_h = 0;                    // the SOURCES are 16-bit CB8 tensors (src[k].p reinterpreted; nstride in elements)
  // training forward (nn.Dropout(p) of ResBlock.out_layers, model/MBAblocks.py:196-203) with a SUPPLIED keep mask:
  // out = act(...) * drop_mask * drop_scale; drop_mask is an fp32 CB8 tensor of the output geometry (0 / 1) or null
  const float* drop_mask = nullptr;
  long drop_ns = 0;
  float drop_scale = 1.f;
};
hipError_t launch_prep(const PrepLaunch& L, hipStream_t s);
// The builder: a launch starts with its output geometry and no source, and each helper states one thing.  Sources are added in
// concat order; all sources of a launch have one element type (a TVH source makes them 16-bit: src_h).
inline PrepLaunch prep_start(int N, int Z, int S) {
  PrepLaunch P;
  P.nsrc = 0; P.N = N; P.Z = Z; P.S = S;
  return P;
}
inline void prep_add_src(PrepLaunch& P, const void* p, long nstride, int Cb, bool collage, bool h16) {
  const int i = P.nsrc++;
  P.src[i].p = (const float*)p; P.src[i].nstride = nstride; P.src[i].Cb = Cb; P.src[i].collage = collage ? 1 : 0;
  P.src_h = h16 ? 1 : 0;
}
inline void prep_src(PrepLaunch& P, const TV& t, bool collage = false) { prep_add_src(P, t.p, t.nstride, t.Cb, collage, false); }
inline void prep_src(PrepLaunch& P, const TVH& t, bool collage = false) { prep_add_src(P, t.p, t.nstride, t.Cb, collage, true); }
inline void prep_out(PrepLaunch& P, const TV& y) { P.out = y.p; P.out_nstride = y.nstride; }
// 16-bit output; real_cb: the channel blocks the sources fill, the rest of y's are the zero pad blocks
inline void prep_out_h(PrepLaunch& P, const TVH& y, int real_cb) { P.out_h = y.p; P.out_h_nstride = y.nstride; P.pad_blocks = y.Cb - real_cb; }
inline void prep_raw(PrepLaunch& P, const TV& r) { P.raw = r.p; P.raw_nstride = r.nstride; }
inline void prep_raw_h(PrepLaunch& P, const TVH& r) { P.raw_h = r.p; P.raw_h_nstride = r.nstride; }
inline void prep_norm(PrepLaunch& P, const float* norm_w, int c_real) { P.norm_w = norm_w; P.inv_c = 1.0f / (float)c_real; }
// per-image rows [b][emb_tot] of all emb_layers: scale at emb_off, shift at emb_off + cout
inline void prep_mod_image(PrepLaunch& P, const float* ss, int emb_off, int cout, int emb_tot) {
  P.mod = MOD_IMAGE; P.mod_scale = ss + emb_off; P.mod_shift = ss + emb_off + cout; P.mod_stride = emb_tot;
}
// per-voxel: two channel-block slices of one modulation tensor (they share its nstride)
inline void prep_mod_voxel(PrepLaunch& P, const TV& scale, const TV& shift, bool half) {
  P.mod = MOD_VOXEL; P.mod_scale = scale.p; P.mod_shift = shift.p; P.mod_stride = scale.nstride; P.mod_half = half ? 1 : 0;
}
inline void prep_mod_voxel(PrepLaunch& P, const TVH& scale, const TVH& shift, bool half) {
  P.mod = MOD_VOXEL; P.mod_scale_h = scale.p; P.mod_shift_h = shift.p; P.mod_stride = scale.nstride; P.mod_half = half ? 1 : 0;
}
// training forward with the keep mask DRAWN in the kernel instead of supplied (drop_keep8: Philox4x32-10; drop_mask
// null): out = act(...) * keep * L.drop_scale.  One fp32 source, fp32 out, RS_SAME, no collage (prep_kernel<1, *, true>).  The draw
// parameters travel beside PrepLaunch (PrepDropArgs), so that the inference instantiations keep their arguments and code.
struct DropRng { unsigned long long key; uint32_t site, thr; };    // drop iff word < thr
hipError_t launch_prep_drop(const PrepLaunch& L, const DropRng& r, hipStream_t s);
// the keep mask of drop_keep8 as an fp32 CB8 tensor of 0 / 1 (pad channels 0)
hipError_t launch_dropout_mask(float* mask, int N, int C, int Z, int S, unsigned long long key, uint32_t site, uint32_t thr,
                               hipStream_t s);
// test / measurement knob (tm_op_prep_h16, tm_op_prep_f32): 0 automatic, 1 prep_kernel's four-wave forms, 2 / 3 the two forms of
// prep_h16_kernel (16-bit calls), 2 the wide form of prep_kernel (fp32 calls, where it is also the automatic choice); process-wide,
// set and reset around the op's own launches only
void set_prep_variant(int v);
// launch_prep takes the call in the wide resident form of prep_kernel (fp32 sources and fp32 out, 33..160 channel blocks)
bool prep_wide_applies(const PrepLaunch& L);
constexpr int PREP_WIDE_MAX_CB = 160;      // channel blocks (1280 channels) the wide form keeps resident

// ---- generic direct conv (VALU) with strided accessors --------------------------------
struct Acc5 {                        // address = n*sN + (c/8)*sCb + (c%8)*sC8 + z*sZ + y*sY + x*sX
  long sN = 0, sCb = 0, sC8 = 0, sZ = 0, sY = 0, sX = 0;
};
Acc5 acc_ncdhw(int C, int Z, int H, int W);
Acc5 acc_cb8(const TV& t);
struct DirectLaunch {
  const float* x = nullptr; Acc5 ax;
  float* y = nullptr; Acc5 ay;
  const float* w = nullptr;          // device [Cout][Cin][kz][ky][kx]
  const float* bias = nullptr;       // device [Cout]
  int N = 0, Cin = 0, Cout = 0;
  int Zin = 0, Zout = 0, S = 0;      // in-plane size S x S (same in/out)
  int kz = 1, ky = 1, kx = 1, pz = 0, py = 0, px = 0;
  int silu_in = 0, up2_out = 0;
};
hipError_t launch_conv_direct(const DirectLaunch& L, hipStream_t s);

// stem: x NCHW '(s z) h w' [N][Cin*Z][S][S] -> y CB8; w [9][Cin][y.Cb*8]
// y_h != null: write the 16-bit CB8 tensor (geometry of y, nstride in elements) instead of y
hipError_t launch_stem(const float* x, TV y, const float* w, const float* bias, int Cin, hipStream_t s,
                       uint16_t* y_h = nullptr, long yh_nstride = 0, int h_f16 = 0);
// head: x CB8 (Cb blocks) -> y NCHW [N][Cout*Z][S][S]; w [9][x.Cb*8][8]
// h16: 0 = x is fp32 CB8; 1 / 2 = x.p points at a bf16 / fp16 CB8 tensor of the same geometry (nstride in elements)
hipError_t launch_head(TV x, float* y, const float* w, const float* bias, int Cout, hipStream_t s, int h16 = 0);

// ---- layout converters ----------------------------------------------------------------
hipError_t launch_to_cb8(const float* x, TV y, hipStream_t s);        // NCDHW -> CB8 (zero pads)
hipError_t launch_from_cb8(TV x, float* y, hipStream_t s);            // CB8 -> NCDHW

// ---- time embedding --------------------------------------------------------------------
// te[b][E] = W2 * silu(W1 * sinusoid(t) + b1) + b2, te_act[b][E] = silu(te) ; then ss[b][tot] = Wall * te_act + ball
hipError_t launch_time_embed(const int64_t* t, int b, int ch, int E, const float* w1,
                             const float* b1, const float* w2, const float* b2, float* te, float* te_act,
                             hipStream_t s);
hipError_t launch_emb_all(const float* te_act, int b, int E, const float* wall, const float* ball,
                          int tot, float* ss, hipStream_t s);

// ---- gene-gene attention ---------------------------------------------------------------
struct GeneW {       // all device pointers; matrices stored TRANSPOSED [in][out]
  const float *wq_t, *bq, *wv_t, *bv, *qnorm, *wp_t, *bp, *norm2, *w1_t, *b1, *w2_t, *b2;
};
// rna dense [B][gn][gn][zs*500] -> tokens out as CB8 [B][ceil(G/8)][zs][gn][gn][8] (pad slots untouched);
// zmask_lo/hi: slices outside [lo,hi) are treated as zero (attention-map variants).
hipError_t launch_gene_attn(const float* rna, int B, int gn, int zs, int G, const GeneW& w,
                            float* out_tok /*nullable*/, float* attn_map /*nullable [B][G][G]*/,
                            int zmask_lo, int zmask_hi, hipStream_t s);
// generic G <= 512, D <= 512 form (global scratch `ws`: B * gene_generic_split(B) * gene_generic_ws_floats(G, D) floats;
// gidx: gene slot table or null)
int gene_generic_split(int B);
size_t gene_generic_ws_floats(int G, int D);
hipError_t launch_gene_attn_generic(const float* rna, int B, int gn, int zs, int G, int D, const GeneW& w, const int* gidx,
                                    float* out_tok, float* attn_map, int zmask_lo, int zmask_hi, float* ws, hipStream_t s);
hipError_t launch_rna_mid(const float* rna, int B, int gn, int zs, int G, float* out, hipStream_t s);
// pathway read-out (attention driver): out [B][4K][2 gn gn], sub [4][B][K][K] or null; glst = K host gene indices.
// launch_gene_readout: fused, no map is formed (gn = 4, zs = 4, G <= 232); launch_gene_readout_gather finishes a batch chunk whose
// four maps [4][Bc][G][G] the map kernels wrote (out / sub / rna point at the chunk)
hipError_t launch_gene_readout(const float* rna, int B, int gn, int zs, int G, const GeneW& w, const int* glst, int K,
                               float* out, float* sub, hipStream_t s);
hipError_t launch_gene_readout_gather(const float* maps, const float* rna, int Bc, int gn, int zs, int G, const int* gidx,
                                      const int* glst, int K, float* out, float* sub, long sub_map_stride, hipStream_t s);
// the model's choice of the fused D = 64 kernels (launch_gene_attn, launch_gene_readout): no gene slot table, G <= 232
inline bool gene_mfma_rule(int D, int G, bool has_gidx) { return D == 64 && G <= 232 && !has_gidx; }
// the read-out wherever the fused kernel does not apply: the generic map kernel over chunks of GENE_RO_CHUNK patches (the four maps
// of a chunk, then the generic kernel's slabs, in `ws` of gene_readout_ws_floats(B, G, D) floats), then gather-and-contract
constexpr int GENE_RO_CHUNK = 8;
size_t gene_readout_ws_floats(int B, int G, int D);
hipError_t launch_gene_readout_chunks(const float* rna, int B, int gn, int zs, int G, int D, const GeneW& w, const int* gidx,
                                      const int* glst, int K, float* out, float* sub, float* ws, hipStream_t s);

// ---- windowed cross attention core -----------------------------------------------------
// q, k, v: CB8 token tensors (tokens = voxels (z h w)); n_h x n_h windows over (H, W).
// o_h != null: write the result as bf16 CB8 (nstride in elements) instead of into `o`.
hipError_t launch_window_attn(const TV& q, const TV& k, const TV& v, const float* qnorm_w,
                              const float* knorm_w, TV o, hipStream_t s, uint16_t* o_h = nullptr,
                              long o_h_nstride = 0);

// ---- sampler ---------------------------------------------------------------------------
struct StepCoefs { float c_recip, c_recipm1, pm1, pm2, sigma, sab_prev, s1m_ab_prev; };
hipError_t launch_sampler_step(const StepCoefs& c, const float* x_patches, const float* eps,
                               const float* noise, float* out, int b, int P1, int P2, int C, int ps,
                               int mode, hipStream_t s);
hipError_t launch_pad_patchify(const float* img, float* patches, int b, int C, int P1, int P2,
                               int ps, float pad, hipStream_t s);

// ---- training slice (tm_train.hip): backward of the prep chain, conv weight gradient, bias gradient ----
hipError_t launch_prep_bwd(const float* x, long x_ns, const float* g, long g_ns, const float* mask, long mask_ns, float drop_scale,
                           const float* w, const float* scale, const float* shift, long mod_stride, int per_image, float* dx,
                           long dx_ns, float* dw, float* dscale, float* dshift, int N, int Cb, int C_real, int Z, int S,
                           float* scratch, hipStream_t s,             // scratch: prep_bwd_scratch_floats(...) floats (two-stage sums)
                           const DropRng* rng = nullptr);             // non-null: mask drawn in the kernel (mask must be null)
size_t prep_bwd_scratch_floats(int N, int Cb, int Z, int S, bool with_mod);
hipError_t launch_conv_wgrad(const TV& x, const TV& dy, float* dw, int Cin, int Cout, int taps, hipStream_t s);
hipError_t launch_chan_sum(const TV& x, float* out, int C, hipStream_t s, int accumulate = 0);
// the same dW on the matrix pipe, to a device pointer (Z 1 .. 4, or 8: the z-slab form); scratch: conv_wgrad_scratch_floats(...) floats
// (0: none needed)
hipError_t launch_conv_wgrad_mfma(const TV& x, const TV& dy, float* dw, int Cin, int Cout, int taps, int accumulate, float* scratch,
                                  hipStream_t s);
int conv_wgrad_chunks(int N, int Z, int S, int Cin, int Cout, int* per_out);
size_t conv_wgrad_scratch_floats(int N, int Z, int S, int Cin, int Cout, int taps);
// device twin of conv_pack_host for CF_1X1, CF_PLANES3, CF_ZSKIP and CF_PAIR; role 1: the data-gradient filter (flipped, cin <-> cout)
hipError_t launch_conv_pack(const float* w, float* out, int Cout, int Cin, int form, int role, hipStream_t s);
// AttnBlock pieces (model/MBAblocks.py:428-614)
hipError_t launch_ew(int op, const float* a, const float* b, const float* c, float* o1, float* o2, long n, hipStream_t s);
hipError_t launch_modnorm_bwd(const TV& x, const float* g, const float* w, const float* scale, float* dx, float* dscale, float* dshift,
                              float* dw, int C_real, float* scratch, hipStream_t s);   // scratch: ceil(voxels / 64) * Cb * 8 floats
hipError_t launch_attn_train(const TV& q, const TV& k, const TV& v, const float* qw, const float* kw, const float* dout, float* o,
                             float* dq, float* dk, float* dv, float* dqw, float* dkw, float* scratch, bool bwd,
                             hipStream_t s);                                            // scratch (bwd): 2 * N * 4 * Cb * 8 floats
// windows of 4 / 8 / 16 tokens, C <= 512 (one workgroup per patch, one wave per window); scratch (bwd): 2 * N * 4 * Cb * 8 floats
hipError_t launch_attn_train_short(const TV& q, const TV& k, const TV& v, const float* qw, const float* kw, const float* dout, float* o,
                                   float* dq, float* dk, float* dv, float* dqw, float* dkw, float* scratch, bool bwd, hipStream_t s);
// windows of 256 / 512 tokens, C <= 256 (key-blocked fp32 MFMA form); scratch: attn_train_long_scratch_floats(...) floats, always
hipError_t launch_attn_train_long(const TV& q, const TV& k, const TV& v, const float* qw, const float* kw, const float* dout, float* o,
                                  float* dq, float* dk, float* dv, float* dqw, float* dkw, float* scratch, bool bwd, hipStream_t s);
size_t attn_train_long_scratch_floats(int N, int Cb, int Z, int S, bool bwd);

hipError_t launch_gemm_f32(const float* A, const float* B, const float* bias, float* C, int M, int N, int K, const long* strides9, int batch,
                           int bias_mode, int accumulate, float alpha, hipStream_t s);   // strides: sam sak sbk sbn scm scn sab sbb scb
hipError_t launch_rows(int op, const float* x, const float* w, const float* g, float* y, float* dw, float* scratch, long rows, int D,
                       hipStream_t s);                                                   // scratch (op 1): ceil(rows / 4) * D floats
hipError_t launch_sumsq(const float* x, long n, float* out, float* scratch, int nwg, hipStream_t s);      // scratch: nwg floats
hipError_t launch_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd, int step,
                       float gscale, hipStream_t s);
// out[i] = ((parts[0][i] + parts[1][i]) + ...) over W slices of n floats, in slice order; queued on s, nothing awaited
hipError_t launch_rank_sum(const float* parts, float* out, int W, long n, hipStream_t s);

// ---- tile I/O (tm_io.hip) --------------------------------------------------------------
hipError_t launch_gene_tile_scatter(const int32_t* crd, const float* dat, long nnz, int gblk, int shift_h, int shift_w,
                                    int gsz, int chan_in, int zpad_ch, float* out, hipStream_t s);
int blosc_decompress(const void* src, size_t src_bytes, void* dst, size_t dst_cap, size_t* out_bytes);

// ---- slice export (tm_export.hip) -------------------------------------------------------
// dst [ceil(Hs / 2)][ceil(Ws / 2)] = rounded mean of the 2 x 2 blocks of src, the last row / column repeated at odd sizes
hipError_t launch_u8_shrink2(const uint8_t* src, int Hs, int Ws, long spitch, uint8_t* dst, long dpitch, hipStream_t s);
// baseline-JPEG scans of tiles [tile0, tile0 + ntiles) of the plane's 256 x 256 grid: need[k] always, the bytes into slot k if
// they fit; with `packed` the filled slots back to back at offsets[k] (offsets[ntiles] = their sum).  `scratch`: the
// workgroups' bit buffers, jpeg_scratch_bytes(ntiles) bytes.
constexpr int JPEG_MAX_WGS = 512;
size_t jpeg_scratch_bytes(int ntiles);
hipError_t launch_jpeg_tiles(const uint8_t* plane, int H, int W, long pitch, int quality, int tile0, int ntiles, uint32_t* scratch,
                             uint8_t* slots, long slot_bytes, int32_t* need, uint8_t* packed, int64_t* offsets, hipStream_t s);
int jpeg_tables(int quality, void* buf, size_t cap, size_t* out_bytes);
// Colour composite of three planar uint8 planes as R, G, B (a null plane is all zeros): brightness, then an optional
// interleaved uint8 [oh][ow][3] overlay sampled nearest by the level's own H and W and blended with alpha / 255 where it is
// not black.  H oh and W ow must stay below 2^31 (32-bit index arithmetic in the kernels).
struct RgbSrc {
  const uint8_t* p[3];
  long pitch[3];
  int H, W;
  float bright;
  const uint8_t* ov;
  int oh, ow, alpha;
};
// the composite as interleaved [H][W][3]
hipError_t launch_rgb_compose(const RgbSrc& src, uint8_t* dst, long dpitch, hipStream_t s);
// launch_jpeg_tiles for the composite: 4:4:4 YCbCr scans, Y Cb Cr interleaved per 8 x 8 MCU; jpeg_rgb_scratch_bytes(ntiles) of scratch
size_t jpeg_rgb_scratch_bytes(int ntiles);
hipError_t launch_jpeg_tiles_rgb(const RgbSrc& src, int quality, int tile0, int ntiles, uint32_t* scratch, uint8_t* slots,
                                 long slot_bytes, int32_t* need, uint8_t* packed, int64_t* offsets, hipStream_t s);
int jpeg_tables_rgb(int quality, void* buf, size_t cap, size_t* out_bytes);

// ---- Blosc-lz4 frames (tm_blosc.hip) --------------------------------------------------------
constexpr int BLOSC_ENC_MIN_BLOCK = 256, BLOSC_ENC_MAX_BLOCK = 65536;
struct BloscGeo {                              // the layout of one frame; every frame of a call has the same
  int nbytes, typesize, bs;                    // bs: effective block size = min(blocksize, nbytes), a multiple of the typesize above it
  int nblocks, nfull, leftover;                // nfull blocks of bs bytes, then one of `leftover` bytes if that is not 0
  int split, nsplits, nstreams;                // bs / typesize >= 128: full blocks are split, into nsplits = typesize streams (else 1); streams per frame
  size_t bound;                                // 16 + 4 nblocks + 4 nstreams + nbytes: every stream stored
};
enum { BLOSC_SRC_BYTES = 0, BLOSC_SRC_F16 = 1, BLOSC_SRC_F32 = 2 };
struct BloscSrc {                              // where the frames' bytes come from
  const uint8_t* base;                         // BYTES: the buffer of the one frame; F16 / F32: the canvas the tiles are cut from
  int mode, TH, TW;                            // tiles [C][TH][TW], written as IEEE half (F32: rounded to nearest even)
  long cstride, pitch;                         // channel stride and row pitch of the canvas in elements
  const int64_t* origins;                      // device, per frame: element offset of the tile's first element
};
// false: nbytes < 1, typesize not 1 / 2 / 4, blocksize no multiple of 4 in [256, 65536], or a frame that could pass 2^31 - 1 bytes
bool blosc_geometry(size_t nbytes, int typesize, int blocksize, BloscGeo* g);
size_t blosc_scratch_bytes(const BloscGeo& g, int nframes);
// nframes <= 65535 frames back to back into `packed` (nframes * g.bound bytes always suffice); offsets [nframes + 1] and
// *total (device) are optional; scratch: blosc_scratch_bytes(g, nframes) bytes, 4-byte aligned
hipError_t launch_blosc_frames(const BloscSrc& src, const BloscGeo& g, int nframes, void* scratch, uint8_t* packed, int64_t* offsets,
                               int64_t* total, hipStream_t s);

// Blosc-lz4 decoder (tm_blosc.hip).  The host walks the frames' headers, bstarts and stream lengths (blosc_dec_walk: every
// range checked against the frame) into a stream table; the device never parses a frame.
struct BloscStream {                           // one LZ4 (or stored: clen == plen) stream
  long long src, dst;                          // byte offsets: in the device copy of the frames, in the scratch
  int clen, plen, frame, pad;
};
struct BloscDecFrame {                         // one frame for blosc_unshuffle_kernel
  long long scratch, dst;                      // bytes in the scratch (16-byte aligned); plain sink: byte offset, canvas sink: element origin
  int nbytes, typesize, blocksize, shuffled;
  int chunk[3], clip[3];                       // canvas sink: the chunk [C][H][W] and the part of it inside the array
};
struct BloscDecInfo { long long nbytes; int typesize, blocksize, nstreams, longest, flags, gpu; };
enum { BLOSC_SINK_BYTES = 0, BLOSC_SINK_F16 = 1, BLOSC_SINK_F32 = 2 };
struct BloscSink {
  void* base;                                  // BYTES: dst; F16 / F32: the canvas
  int mode;
  long cstride, pitch;                         // canvas: channel stride and row pitch in elements
};
// One frame of `len` bytes at f (host).  TM_OK with info->gpu = 0: a frame the host decoder may read and the GPU decoder does
// not take (nothing appended); TM_ERR_ARG with a text: a range outside the frame.  Otherwise the frame's streams are appended
// to *tab (if given) with src relative to src_base and dst to dst_base, and *longest_lz4 (if given) is raised to the longest
// plain size of a stream that is not stored.
int blosc_dec_walk(const char* fn, int k, const uint8_t* f, size_t len, BloscDecInfo* info, std::vector<BloscStream>* tab, long long src_base,
                   long long dst_base, int* longest_lz4);
// decode `nstreams` streams into the scratch, then unshuffle `nframes` frames into the sink; status [nframes] is zeroed first
hipError_t launch_blosc_decode(const uint8_t* frames, const BloscStream* tab, int nstreams, int longest_lz4, const BloscDecFrame* fr,
                               int nframes, int max_nbytes, uint8_t* scratch, const BloscSink& sink, int32_t* status, hipStream_t s);

// ---- ROI evaluation (tm_metrics.hip) -----------------------------------------------------
// SSIM statistics of P plane pairs: the valid output is cut into SSIM_TW x SSIM_TH tiles, one workgroup each
constexpr int SSIM_TW = 64, SSIM_TH = 32, SSIM_MAX_TAPS = 33, SSIM_TAP_PAD = 7;
struct SsimTaps {                              // by value in the kernel arguments: every tap is a scalar operand
  float w[SSIM_TAP_PAD + SSIM_MAX_TAPS + SSIM_TAP_PAD];   // tap t at w[SSIM_TAP_PAD + t], zeros around
  float sum, one_minus_sum;                    // S = (sum of the taps)^2, the weight of the n x n window, and 1 - S: from double, rounded once
  int n;
};
size_t ssim_lds_bytes(int n);
size_t ssim_partial_doubles(int P, int H, int W, int n);      // per tile and plane: sum ssim, sum cs, sum (x - y)^2
// out[p][3] = the three sums of plane p in fp64; pitches and plane strides in bytes; partials: ssim_partial_doubles(...) doubles
hipError_t launch_ssim_planes(const void* x, const void* y, bool is_f32, int P, int H, int W, long xpitch, long xplane, long ypitch,
                              long yplane, const SsimTaps& taps, float C1, float C2, double* partials, double* out, hipStream_t s);
// dst fp32 [P][ceil(H / 2)][ceil(W / 2)] = avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2)) with the pad counted
hipError_t launch_avgpool2_pad(const void* src, bool is_f32, int P, int H, int W, long spitch, long splane, void* dst, long dpitch,
                               long dplane, hipStream_t s);
// SSIM statistics of V volume pairs (the 3-D window): SSIM3_TW x SSIM3_TH tiles of the valid in-plane output, one workgroup
// each, marching along the depth with the SSIM3_TAPS - 1 open windows of its output held in registers
constexpr int SSIM3_TW = 16, SSIM3_TH = 16, SSIM3_TAPS = 11;
struct Ssim3Taps {
  float w[SSIM3_TAPS];                         // the n taps, zeros behind
  float sum, one_minus_sum;                    // S = (sum of the taps)^3, the weight of the n^3 window, and 1 - S: from double, rounded once
  int n;
};
size_t ssim3_partial_doubles(int V, int H, int W, int n);
// out[v][3] in fp64; pitches, depth strides (plane to plane) and volume strides in bytes
hipError_t launch_ssim_volumes(const void* x, const void* y, bool is_f32, int V, int D, int H, int W, long xpitch, long xdepth, long xvol,
                               long ypitch, long ydepth, long yvol, const Ssim3Taps& taps, float C1, float C2, double* partials,
                               double* out, hipStream_t s);
// dst fp32 [V][ceil(D / 2)][ceil(H / 2)][ceil(W / 2)] = avg_pool3d(kernel 2, stride 2, padding (D % 2, H % 2, W % 2)), the pad counted
hipError_t launch_avgpool2_pad3(const void* src, bool is_f32, int V, int D, int H, int W, long spitch, long sdepth, long svol, void* dst,
                                long dpitch, long ddepth, long dvol, hipStream_t s);

// ---- host helpers of the C-ABI units (tm_model.hip, tm_ops.hip, tm_io.hip) ---------------
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // sets the tm_last_error() text, returns code
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(TM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
// the read-out's argument rules (tm_gene_attn_readout, tm_op_gene_readout): TM_OK, or TM_ERR_ARG with the text
int gene_readout_args(int zs, const int* glst, int K, int G);
inline bool is_h16(int dtype) { return dtype == TM_DTYPE_BF16 || dtype == TM_DTYPE_F16; }   // 16-bit operand modes
inline TVH as_h(const TV& t) {      // the same geometry and strides over 16-bit storage
  TVH v;
  v.p = (uint16_t*)t.p; v.N = t.N; v.C = t.C; v.Cb = t.Cb; v.Z = t.Z; v.H = t.H; v.W = t.W; v.nstride = t.nstride;
  return v;
}

}  // namespace tmk
