// Single-operator entry points of the C-ABI (include/teramind_hip.h): one kernel form per call, for the parity tests
// (tests/test_gpu_ops.py) and the training step (teramind_amd.training / train_model).  Unlike the executor (tm_model.hip)
// these hooks take HOST weights where the signature says so, own their device scratch for the duration of the call
// (DevTmp) and synchronise `stream` before returning (finish); tm_op_to_cb8 / tm_op_from_cb8 only enqueue.
#include "../../include/teramind_hip.h"
#include "tm_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>
#include <string.h>

using namespace tmk;

// Device scratch of one call: buffers and events, released on every return path.  After a failed HIP call every further
// request returns nullptr; the hook checks `err` once after allocating and returns report().
struct DevTmp {
  std::vector<void*> ptrs;
  std::vector<hipEvent_t> events;
  hipError_t err = hipSuccess;
  const char* what = "";
  // stream-ordered form (the resident hooks, which may neither synchronise nor touch host memory): buffers come from the
  // device's memory pool in `st`'s order and go back to it in that order when the call returns
  bool ordered = false;
  hipStream_t st = nullptr;
  DevTmp() = default;
  explicit DevTmp(hipStream_t stream) : ordered(true), st(stream) { keep_pool(); }
  // The pool's default release threshold is 0: it would hand its memory back to the system at every synchronisation and map it
  // again at the next call.  Raised once per device, so the scratch of a step (at most 64 MB, conv_wgrad_chunks) is reused.
  // This is a setting of the process's default pool, not of this library: once a resident hook has run, every other
  // hipMallocAsync user of the process keeps its freed memory in the pool too (hipMemPoolTrimTo gives it back).  The `done`
  // flags are unguarded: two threads racing here set the same value twice, which is harmless.
  static void keep_pool() {
    static bool done[64] = {};
    int dev = 0;
    hipMemPool_t pool = nullptr;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || done[dev]) return;
    uint64_t keep = UINT64_MAX;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) == hipSuccess)
      done[dev] = true;
  }
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() {
    for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
    for (void* p : ptrs) (void)(ordered ? hipFreeAsync(p, st) : hipFree(p));
  }
  float* ordered_floats(size_t n, bool zero) {
    void* p = nullptr;
    if (err != hipSuccess || !ok(hipMallocAsync(&p, n * sizeof(float), st), "hipMallocAsync")) return nullptr;
    ptrs.push_back(p);
    return !zero || ok(hipMemsetAsync(p, 0, n * sizeof(float), st), "hipMemsetAsync") ? (float*)p : nullptr;
  }
  // n floats copied from `host` in `st`'s order; `host` must stay alive until the stream is synchronised (finish)
  float* ordered_upload(const void* host, size_t n) {
    float* p = ordered_floats(n, false);
    return p && ok(hipMemcpyAsync(p, host, n * sizeof(float), hipMemcpyHostToDevice, st), "hipMemcpyAsync") ? p : nullptr;
  }
  bool ok(hipError_t e, const char* call) {
    if (e != hipSuccess) { err = e; what = call; }
    return e == hipSuccess;
  }
  // n elements of T, copied from `host` if given
  template <class T> T* alloc(size_t n, const T* host = nullptr) {
    void* p = nullptr;
    if (err != hipSuccess || !ok(hipMalloc(&p, n * sizeof(T)), "hipMalloc")) return nullptr;
    ptrs.push_back(p);
    if (host && !ok(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy")) return nullptr;
    return (T*)p;
  }
  float* zeros(size_t n) {
    float* p = alloc<float>(n);
    return p && ok(hipMemset(p, 0, n * sizeof(float)), "hipMemset") ? p : nullptr;
  }
  hipEvent_t event() {
    hipEvent_t ev = nullptr;
    if (err != hipSuccess || !ok(hipEventCreate(&ev), "hipEventCreate")) return nullptr;
    events.push_back(ev);
    return ev;
  }
  int report() const { return fail(TM_ERR_HIP, "%s failed: %s", what, hipGetErrorString(err)); }
};

// the tail of every synchronising hook: wait for `stream`, report the first error as "<what>: <HIP error>"
static int finish(hipStream_t st, hipError_t e, const char* what) {
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? TM_OK : fail(TM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

static TVH view_h16(void* p, int N, int C, int Z, int H, int W) { return as_h(cb8_view(p, N, C, Z, H, W)); }

// the sources of the prep hooks: nsrc dense CB8 tensors of src_c[i] channels on Ss x Ss planes (the patch count of a source plays
// no part in its view); returns their channel blocks
static int prep_op_sources(PrepLaunch& P, const void* const* src, const int* src_c, const int* collage, int nsrc, int Z, int Ss,
                           bool h16) {
  int cbtot = 0;
  for (int i = 0; i < nsrc; ++i) {
    const TV t = cb8_view(const_cast<void*>(src[i]), 0, src_c[i], Z, Ss, Ss);
    if (h16) prep_src(P, as_h(t), collage[i] != 0);
    else prep_src(P, t, collage[i] != 0);
    cbtot += t.Cb;
  }
  return cbtot;
}

// fp32 CB8 x -> a 16-bit CB8 copy in `tmp` (prep kernel, no norm / act); `pair`: even block count (zero pad blocks), the
// operand form of the 16-bit conv kernels.  Launches nothing once `e` holds an error.
static TVH to_h16(DevTmp& tmp, const TV& x, bool f16, bool pair, hipStream_t st, hipError_t& e) {
  if (e != hipSuccess) return TVH();
  const int Cb = pair ? pair_cb(x.Cb) : x.Cb;
  const TVH h = view_h16(tmp.alloc<uint16_t>((size_t)x.N * Cb * x.plane()), x.N, Cb * 8, x.Z, x.H, x.W);
  if (tmp.err) { e = tmp.err; return h; }
  PrepLaunch P = prep_start(x.N, x.Z, x.H);
  prep_src(P, x);
  P.h_f16 = f16 ? 1 : 0;
  prep_out_h(P, h, x.Cb);
  e = launch_prep(P, st);
  return h;
}

// packed conv weights and the bias zero padded to ceil(Cout / 64) * 64 floats (what the MFMA epilogues read), in `tmp`
template <class T>
static std::pair<const T*, const float*> upload_conv(DevTmp& tmp, const std::vector<T>& w, const void* bias_host, int Cout) {
  std::vector<float> b((size_t)(Cout + 63) / 64 * 64, 0.f);
  memcpy(b.data(), bias_host, Cout * sizeof(float));
  return {tmp.alloc(w.size(), w.data()), tmp.alloc(b.size(), b.data())};
}

// per-channel vectors: [rows][C] host <-> [rows][Cp] zero padded device rows
static const float* upload_rows(DevTmp& tmp, const void* host, int rows, int C, int Cp) {
  std::vector<float> o((size_t)rows * Cp, 0.f);
  for (int r = 0; r < rows; ++r) memcpy(o.data() + (size_t)r * Cp, (const float*)host + (size_t)r * C, C * sizeof(float));
  return tmp.alloc(o.size(), o.data());
}
static hipError_t download_rows(void* host, const float* dev, int rows, int C, int Cp) {
  std::vector<float> h((size_t)rows * Cp);
  const hipError_t e = hipMemcpy(h.data(), dev, h.size() * sizeof(float), hipMemcpyDeviceToHost);
  for (int r = 0; r < rows && e == hipSuccess; ++r) memcpy((float*)host + (size_t)r * C, h.data() + (size_t)r * Cp, C * sizeof(float));
  return e;
}

// ------------------------------------------------------------------------------------------
// single-operator entry points (tests)
// ------------------------------------------------------------------------------------------
extern "C" int tm_op_to_cb8(const void* x, void* y, int N, int C, int Z, int H, int W, void* stream) {
  HIP_TRY(launch_to_cb8((const float*)x, cb8_view(y, N, C, Z, H, W), (hipStream_t)stream));
  return TM_OK;
}
extern "C" int tm_op_from_cb8(const void* x, void* y, int N, int C, int Z, int H, int W, void* stream) {
  HIP_TRY(launch_from_cb8(cb8_view(const_cast<void*>(x), N, C, Z, H, W), (float*)y, (hipStream_t)stream));
  return TM_OK;
}
extern "C" int tm_op_conv_mfma(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                               int Cout, int Z, int S, int ksize, int zmode, int up2, int tile_variant, void* stream) {
  return tm_op_conv_mfma_res(x_cb8, w_host, bias_host, y_cb8, nullptr, 0, N, Cin, Cout, Z, S, ksize, zmode, up2, tile_variant, stream);
}
// One conv of a single-operator hook: the host weights packed for `form` and uploaded with the bias (into `tmp`), and the launch
// filled in: x [N][Cin][Z][S][S], y [N][Cout][Zout][So][So], the residual (optional) of y's geometry, or with res_half at half its
// plane size.  The caller adds what is its own and launches L.
struct ConvOp {
  DevTmp tmp;
  ConvLaunch L;
  TV res;
};
static int conv_op(ConvOp& op, int form, const void* w_host, const void* bias_host, const void* x_cb8, void* y_cb8, int N, int Cin,
                   int Cout, int Z, int S, int Zout, int So, int zmode, int tile_variant, const void* res_cb8 = nullptr,
                   int res_half = 0) {
  ConvW cw = conv_w(form, Cout, (Cin + 7) / 8);
  std::vector<float> pk(conv_pack_floats(form, Cout, cw.Cbi));
  conv_pack_host(form, (const float*)w_host, Cout, &Cin, 1, pk.data());
  std::tie(cw.w, cw.bias) = upload_conv(op.tmp, pk, bias_host, Cout);
  if (op.tmp.err) return op.tmp.report();
  ConvLaunch& L = op.L;
  L.x = cb8_view(const_cast<void*>(x_cb8), N, Cin, Z, S, S);
  L.w = cw;
  L.y = cb8_view(y_cb8, N, Cout, Zout, So, So);
  L.tile_variant = tile_variant;
  L.zmode = zmode;
  if (res_cb8) {
    op.res = cb8_view(const_cast<void*>(res_cb8), N, Cout, Zout, res_half ? So / 2 : So, res_half ? So / 2 : So);
    L.res = &op.res;
    L.res_half = res_half ? 1 : 0;
  }
  return TM_OK;
}

extern "C" int tm_op_conv_mfma_res(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                                   int res_half, int N, int Cin, int Cout, int Z, int S, int ksize, int zmode, int up2,
                                   int tile_variant, void* stream) {
  if (ksize != 1 && ksize != 3) return fail(TM_ERR_ARG, "ksize must be 1 or 3");
  if (zmode != ZM_PAD1 && zmode != ZM_INPLANE && zmode != ZM_VALID && zmode != ZM_UPS) return fail(TM_ERR_ARG, "bad zmode");
  const bool ups = ksize == 3 && zmode == ZM_UPS;       // w [Cout][Cin][27]: conv of the nearest-x2 upsampled x (y at 2S)
  if (zmode == ZM_UPS && (ksize != 3 || up2)) return fail(TM_ERR_ARG, "ZM_UPS: ksize 3, no fused upsample of the output");
  if (res_cb8 && (ksize != 3 || zmode == ZM_UPS)) return fail(TM_ERR_ARG, "residual: k x 3 x 3 forms other than ZM_UPS only");
  if (res_half && (!res_cb8 || up2 || S < 2)) return fail(TM_ERR_ARG, "res_half: needs a residual, S >= 2 and no fused upsample");
  const int Zout = (ksize == 3 && zmode == ZM_VALID) ? Z - 2 : Z;
  ConvOp op;                                            // the pair form at Z == 2, as tm_model_finalize packs c1 / c2 there
  if (const int rc = conv_op(op, conv_pick_form(ksize, zmode, Z, false, ROLE_OP), w_host, bias_host, x_cb8, y_cb8, N, Cin, Cout, Z, S,
                             Zout, (up2 || ups) ? 2 * S : S, zmode, tile_variant, res_cb8, res_half))
    return rc;
  op.L.flags = up2 ? EPI_UP2 : 0;
  return finish((hipStream_t)stream, launch_conv_mfma(op.L, (hipStream_t)stream), "conv_mfma");
}

// The fp32 pair-form conv with the ResBlock mid-section in its epilogue (conv3d_zpair<0, *, true>), alone.  The forms the kernel
// does not take are refused here, before any device call, with the launcher's own rule for the tile (conv_tile).
extern "C" int tm_op_conv_zpair_fused_f32(const void* x_cb8, const void* w_host, const void* bias_host, const void* norm_w_host,
                                          const void* scale_host, const void* shift_host, const void* res_cb8, void* a2_out,
                                          void* h1_out, void* a2_sep_out, int N, int Cin, int Cout, int Z, int S, int per_image,
                                          int tile_variant, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || !norm_w_host || !scale_host || !shift_host || !a2_out) return fail(TM_ERR_ARG, "null argument");
  if (N < 1 || Cin < 1 || per_image < 1) return fail(TM_ERR_ARG, "N, Cin, per_image must be positive");
  if (Z != 2) return fail(TM_ERR_ARG, "the pair form exists at Z == 2 only (got Z = %d)", Z);
  if (Cout != 64) return fail(TM_ERR_ARG, "the fused mid-section needs Cout == 64: one wave holds every channel (got %d)", Cout);
  if (res_cb8) return fail(TM_ERR_ARG, "the fused mid-section takes no residual");
  if (S != 8 && S != 16 && S != 32 && S != 64 && S != 128) return fail(TM_ERR_ARG, "S must be 8, 16, 32, 64 or 128 (got %d)", S);
  if (tile_variant < 0 || tile_variant > 2) return fail(TM_ERR_ARG, "tile_variant must be 0 (auto), 1 or 2 (got %d)", tile_variant);
  if (conv_tile(CF_PAIR, (long)N * Z * S * S, 1, S, tile_variant) != 2)
    return fail(TM_ERR_ARG, "the fused mid-section exists in the 128-voxel tile only; this launch takes the 64-voxel one");
  if (a2_sep_out && !h1_out) return fail(TM_ERR_ARG, "a2_sep_out needs h1_out");
  if (conv_pick_form(3, ZM_PAD1, Z, false, ROLE_OP) != CF_PAIR) return fail(TM_ERR_ARG, "the pair form is switched off (TM_CONV_ZPAIR=0)");
  ConvOp op;
  if (const int rc = conv_op(op, CF_PAIR, w_host, bias_host, x_cb8, a2_out, N, Cin, Cout, Z, S, Z, S, ZM_PAD1, tile_variant)) return rc;
  const int nimg = (N + per_image - 1) / per_image;
  const float* nw = op.tmp.alloc((size_t)Cout, (const float*)norm_w_host);
  const float* sc = op.tmp.alloc((size_t)nimg * Cout, (const float*)scale_host);
  const float* sh = op.tmp.alloc((size_t)nimg * Cout, (const float*)shift_host);
  if (op.tmp.err) return op.tmp.report();
  hipStream_t st = (hipStream_t)stream;
  ConvLaunch& L = op.L;
  L.fuse_norm = 1; L.a2 = L.y; L.norm_w = nw; L.mod_scale = sc; L.mod_shift = sh; L.mod_stride = Cout; L.per_image = per_image;
  L.inv_c = 1.0f / (float)Cout;
  hipError_t e = launch_conv_mfma(L, st);
  if (e == hipSuccess && h1_out) {                      // the same conv, plain epilogue, then (a2_sep_out) the separate pass on it
    ConvLaunch U = L;
    U.fuse_norm = 0; U.y = cb8_view(h1_out, N, Cout, Z, S, S);
    e = launch_conv_mfma(U, st);
    if (e == hipSuccess && a2_sep_out) {
      PrepLaunch P = prep_start(N, Z, S);
      prep_src(P, U.y);
      prep_norm(P, nw, Cout);
      P.mod = MOD_IMAGE; P.mod_scale = sc; P.mod_shift = sh; P.mod_stride = Cout;   // rows of their own, not slices of one matrix
      P.act = 1; P.per_image = per_image;
      prep_out(P, cb8_view(a2_sep_out, N, Cout, Z, S, S));
      e = launch_prep(P, st);
    }
  }
  return finish(st, e, "conv_zpair_fused (fp32)");
}

// The pair form of the upsampled-input conv (conv3d_zpair_ups), alone: y [N][ceil(Cout/8)][2][2S][2S][8] = conv3d(pad 1) of the
// nearest-x2 upsampled x, computed on x.  tm_op_conv_mfma with zmode 3 stays the z-skip form of the same conv.
extern "C" int tm_op_conv_ups_pair_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                       int Cout, int Z, int S, int tile_variant, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || !y_cb8) return fail(TM_ERR_ARG, "null argument");
  if (N < 1 || Cin < 1 || Cout < 1) return fail(TM_ERR_ARG, "N, Cin, Cout must be positive");
  if (Z != 2) return fail(TM_ERR_ARG, "the pair form exists at Z == 2 only (got Z = %d)", Z);
  if (S != 4 && S != 8 && S != 16 && S != 32 && S != 64) return fail(TM_ERR_ARG, "S must be 4, 8, 16, 32 or 64 (got %d)", S);
  if (tile_variant < 0 || tile_variant > 2) return fail(TM_ERR_ARG, "tile_variant must be 0 (auto), 1 or 2 (got %d)", tile_variant);
  ConvOp op;
  if (const int rc = conv_op(op, conv_pick_form(3, ZM_UPS, Z, false, ROLE_OP_PAIR_UPS), w_host, bias_host, x_cb8, y_cb8, N, Cin, Cout, Z,
                             S, Z, 2 * S, ZM_UPS, tile_variant))
    return rc;
  return finish((hipStream_t)stream, launch_conv_mfma(op.L, (hipStream_t)stream), "conv_ups_pair (fp32)");
}

// What the two forms of the fp32 3x3x3 pad-1 conv at Z == 2 with a hook of their own take (form: CF_PAIR | CF_XQUAD); what the
// kernels do not take is refused here, before any device call.
static int pad1_z2_args(int form, const void* x, const void* w, const void* b, const void* y, int N, int Cin, int Cout, int Z, int S,
                        int tile_variant) {
  const bool xq = form == CF_XQUAD;
  if (!x || !w || !b || !y) return fail(TM_ERR_ARG, "null argument");
  if (N < 1 || Cin < 1 || Cout < 1) return fail(TM_ERR_ARG, "N, Cin, Cout must be positive");
  if (Z != 2) return fail(TM_ERR_ARG, "the %s form exists at Z == 2 only (got Z = %d)", xq ? "x-quad" : "pair", Z);
  if (S != 8 && S != 16 && S != 32 && S != 64 && S != 128) return fail(TM_ERR_ARG, "S must be 8, 16, 32, 64 or 128 (got %d)", S);
  if (tile_variant < 0 || tile_variant > 2) return fail(TM_ERR_ARG, "tile_variant must be 0 (auto), 1 or 2 (got %d)", tile_variant);
  if (conv_pick_form(3, ZM_PAD1, 2, true, xq ? ROLE_OP_XQUAD : ROLE_OP) != form)
    return fail(TM_ERR_ARG, "the %s form is switched off (%s=0)", xq ? "x-quad" : "pair", xq ? "TM_CONV_XQUAD" : "TM_CONV_ZPAIR");
  return TM_OK;
}

// The x-quad form (conv3d_xquad, Winograd F(4,3) along x), alone.  Returns the tile it launched (1 = 64 four-column groups per
// workgroup, 2 = 128) or a negative error.
// The split-K factor of a hook's x-quad launch from its argument (0 = the rule, 1 | 2 | 4 forced) into *ksplit, or TM_ERR_ARG
// with the text, before any device call
static int xquad_split_arg(int arg, int N, int Cin, int Cout, int S, int res_half, int* ksplit) {
  const int Cbi = (Cin + 7) / 8;
  if (arg != 0 && arg != 1 && arg != 2 && arg != 4) return fail(TM_ERR_ARG, "ksplit must be 0 (the rule), 1, 2 or 4 (got %d)", arg);
  if (arg > Cbi) return fail(TM_ERR_ARG, "ksplit %d is above the %d cin blocks: a split would be empty", arg, Cbi);
  if (arg > 1 && res_half) return fail(TM_ERR_ARG, "a split launch takes no half-resolution residual (res_half)");
  *ksplit = arg ? arg : xquad_ksplit((long)N * 2 * S * S, Cout, Cbi, S, res_half != 0);
  return TM_OK;
}
// the partial sums of a split launch, from the op's scratch
static int xquad_split_scratch(ConvOp& op, int ksplit) {
  op.L.xquad_ksplit = ksplit;
  if (ksplit > 1) op.L.part = op.tmp.alloc<float>(xquad_part_floats(ksplit, op.L.y));
  return op.tmp.err ? op.tmp.report() : TM_OK;
}
// ksplit: 1 | 2 | 4 (xquad_split_arg)
static int xquad_op(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8, int res_half, int N,
                    int Cin, int Cout, int Z, int S, int tile_variant, int sched, int ksplit, void* stream) {
  if (const int rc = pad1_z2_args(CF_XQUAD, x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, Z, S, tile_variant)) return rc;
  if (res_half && !res_cb8) return fail(TM_ERR_ARG, "res_half needs a residual");
  ConvOp op;
  if (const int rc = conv_op(op, CF_XQUAD, w_host, bias_host, x_cb8, y_cb8, N, Cin, Cout, Z, S, Z, S, ZM_PAD1, tile_variant, res_cb8,
                             res_half))
    return rc;
  op.L.xquad_sched = sched;
  if (const int rc = xquad_split_scratch(op, ksplit)) return rc;
  const int rc = finish((hipStream_t)stream, launch_conv_mfma(op.L, (hipStream_t)stream), "conv_xquad (fp32)");
  return rc ? rc : conv_tile(CF_XQUAD, (long)N * Z * S * S, op.L.w.ntile, S, tile_variant);
}
extern "C" int tm_op_conv_xquad_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                                    int res_half, int N, int Cin, int Cout, int Z, int S, int tile_variant, void* stream) {
  return xquad_op(x_cb8, w_host, bias_host, y_cb8, res_cb8, res_half, N, Cin, Cout, Z, S, tile_variant, -1, 1, stream);
}
// The same with the schedule of conv3d_xquad forced: 0 = the four-barrier schedule, 1 = the pipelined one (same pack, same bits).
extern "C" int tm_op_conv_xquad_sched_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                                          int res_half, int N, int Cin, int Cout, int Z, int S, int tile_variant, int sched, void* stream) {
  if (sched != 0 && sched != 1) return fail(TM_ERR_ARG, "sched must be 0 (four barriers) or 1 (pipelined) (got %d)", sched);
  return xquad_op(x_cb8, w_host, bias_host, y_cb8, res_cb8, res_half, N, Cin, Cout, Z, S, tile_variant, sched, 1, stream);
}
// ... and with the K loop split over ksplit workgroups per tile (0 = the rule): returns the factor taken
extern "C" int tm_op_conv_xquad_split_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                                          int res_half, int N, int Cin, int Cout, int Z, int S, int tile_variant, int sched, int ksplit,
                                          void* stream) {
  if (const int rc = pad1_z2_args(CF_XQUAD, x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, Z, S, tile_variant)) return rc;
  if (sched != 0 && sched != 1) return fail(TM_ERR_ARG, "sched must be 0 (four barriers) or 1 (pipelined) (got %d)", sched);
  int k = 1;
  if (const int rc = xquad_split_arg(ksplit, N, Cin, Cout, S, res_half, &k)) return rc;
  const int rc = xquad_op(x_cb8, w_host, bias_host, y_cb8, res_cb8, res_half, N, Cin, Cout, Z, S, tile_variant, sched, k, stream);
  return rc < 0 ? rc : k;
}
extern "C" int tm_conv_xquad_ksplit(int N, int Cin, int Cout, int S, int res_half) {
  return xquad_ksplit((long)N * 2 * S * S, Cout, (Cin + 7) / 8, S, res_half != 0);
}

// Timing hook (tools/bench_conv_xquad.py): the 3x3x3 pad-1 conv at Z == 2 packed once for `form` (0 = the pair form, 2 = the
// x-quad form; 1 is no form any more), then `iters` launches, each between two events of its own; ms_out[i] (host) = the time of
// launch i.  sched: the schedule of conv3d_xquad (form 2 only): -1 = the launcher's choice, 0 | 1 forced.
// ksplit: the split-K factor of the x-quad form as in tm_op_conv_xquad_split_f32 (a launch is then the conv and its reduction)
static int conv_pad1_time(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin, int Cout, int S,
                          int form, int tile_variant, int sched, int ksplit, int iters, float* ms_out, void* stream) {
  const int cf = form == 2 ? CF_XQUAD : CF_PAIR;
  if (const int rc = pad1_z2_args(cf, x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, 2, S, tile_variant)) return rc;
  if ((form != 0 && form != 2) || iters < 1 || !ms_out) return fail(TM_ERR_ARG, "form must be 0 or 2, iters >= 1, ms_out non-null");
  if (sched < -1 || sched > 1 || (sched >= 0 && form != 2)) return fail(TM_ERR_ARG, "sched must be -1, or 0 | 1 with form 2 (got %d)", sched);
  if (ksplit != 1 && form != 2) return fail(TM_ERR_ARG, "ksplit other than 1 needs form 2 (got %d)", ksplit);
  int k = 1;
  if (const int rc = xquad_split_arg(ksplit, N, Cin, Cout, S, 0, &k)) return rc;
  ConvOp op;
  if (const int rc = conv_op(op, cf, w_host, bias_host, x_cb8, y_cb8, N, Cin, Cout, 2, S, 2, S, ZM_PAD1, tile_variant)) return rc;
  op.L.xquad_sched = sched;
  if (const int rc = xquad_split_scratch(op, k)) return rc;
  hipEvent_t e0 = op.tmp.event(), e1 = op.tmp.event();
  if (op.tmp.err) return op.tmp.report();
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < iters; ++i) {
    HIP_TRY(hipEventRecord(e0, st));
    HIP_TRY(launch_conv_mfma(op.L, st));
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(ms_out + i, e0, e1));
  }
  return finish(st, hipSuccess, "conv_pad1_time (fp32)");
}
extern "C" int tm_op_conv_pad1_time_sched_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                              int Cout, int S, int form, int tile_variant, int sched, int iters, float* ms_out,
                                              void* stream) {
  return conv_pad1_time(x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, S, form, tile_variant, sched, 1, iters, ms_out, stream);
}
extern "C" int tm_op_conv_pad1_time_split_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                              int Cout, int S, int form, int tile_variant, int sched, int ksplit, int iters,
                                              float* ms_out, void* stream) {
  return conv_pad1_time(x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, S, form, tile_variant, sched, ksplit, iters, ms_out, stream);
}

// power of two >= 2: what a half-resolution gate needs of S (read at (z, y >> 1, x >> 1))
static bool half_gate_ok(int S) { return S >= 2 && (S & (S - 1)) == 0; }

extern "C" int tm_conv1_form(long vox, int ntile, int tile_variant) { return conv1_form(vox, ntile, tile_variant); }
extern "C" int tm_conv_xquad_lds_bytes(int half, int tw, int sched) { return conv_xquad_lds_bytes(half, tw, sched); }
extern "C" int tm_conv_frag_addrs(int kernel, int half, int tw, int what, int wave, int p, int ky, int kx, int sub, int* out64) {
  return conv_frag_addrs(kernel, half, tw, what, wave, p, ky, kx, sub, out64);
}

extern "C" int tm_op_conv1_f32(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, const void* res_cb8,
                               const void* gate_cb8, int x_cbtot, int x_cb0, int gate_cbtot, int gate_cb0, int gate_half, int gelu,
                               int tile_variant, int N, int Cin, int Cout, int Z, int S, int* form_out, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || !y_cb8) return fail(TM_ERR_ARG, "null argument");
  if (N < 1 || Cin < 1 || Cout < 1 || Z < 1 || S < 1) return fail(TM_ERR_ARG, "N, Cin, Cout, Z, S must be positive");
  const int Cbi = (Cin + 7) / 8, Cob = (Cout + 7) / 8;
  if (x_cb0 < 0 || x_cb0 + Cbi > x_cbtot)
    return fail(TM_ERR_ARG, "x slice: blocks [%d, %d) run past the %d blocks of the tensor", x_cb0, x_cb0 + Cbi, x_cbtot);
  if (gate_half && !gate_cb8) return fail(TM_ERR_ARG, "gate_half without a gate");
  if (gate_half && !half_gate_ok(S)) return fail(TM_ERR_ARG, "gate_half: S must be a power of two >= 2 (got %d)", S);
  if (gate_cb8 && (gate_cb0 < 0 || gate_cb0 + Cob > gate_cbtot))
    return fail(TM_ERR_ARG, "gate slice: blocks [%d, %d) run past the %d blocks of the tensor", gate_cb0, gate_cb0 + Cob, gate_cbtot);
  if (tile_variant < 0 || tile_variant > 3) return fail(TM_ERR_ARG, "tile_variant must be 0 (auto), 1, 2 or 3 (got %d)", tile_variant);
  ConvW cw = conv_w(CF_1X1, Cout, Cbi);
  const int form = conv1_form((long)N * Z * S * S, cw.ntile, tile_variant);
  if (!form) return fail(TM_ERR_ARG, "tile_variant 3 (128-cout tile) needs an even number of 64-cout tiles (got %d)", cw.ntile);
  if (form_out) *form_out = form;
  std::vector<float> pk(conv_pack_floats(CF_1X1, Cout, Cbi));
  conv_pack_host(CF_1X1, (const float*)w_host, Cout, &Cin, 1, pk.data());
  DevTmp tmp;
  std::tie(cw.w, cw.bias) = upload_conv(tmp, pk, bias_host, Cout);
  if (tmp.err) return tmp.report();
  ConvLaunch L;
  L.x = cb8_view(const_cast<void*>(x_cb8), N, x_cbtot * 8, Z, S, S).blocks(x_cb0, Cbi);
  L.w = cw;
  L.y = cb8_view(y_cb8, N, Cout, Z, S, S);
  L.tile_variant = tile_variant;
  L.flags = gelu ? EPI_GELU : 0;
  TV res = L.y, gate;
  if (res_cb8) { res.p = (float*)const_cast<void*>(res_cb8); L.res = &res; }      // res_cb8 == y_cb8: x <- x + gate * Linear(.)
  if (gate_cb8) {
    const int Sg = gate_half ? S / 2 : S;
    gate = cb8_view(const_cast<void*>(gate_cb8), N, gate_cbtot * 8, Z, Sg, Sg).blocks(gate_cb0, Cob);
    L.gate = &gate;
    L.gate_half = gate_half ? 1 : 0;
  }
  return finish((hipStream_t)stream, launch_conv_mfma(L, (hipStream_t)stream), "conv1 (fp32)");
}

// The ConvLaunchH of the 16-bit 3x3x3 conv hooks: x N x Cin channels (blocks paired) on Z planes of S x S, y Cout channels at
// So = S, or 2S in the upsampled-input form (Z == 2 only, as the half-resolution residual); fused: the norm epilogue writes the
// 16-bit a2 at y's geometry.  Rejects the forms the kernels do not take, before any device call; the caller sets the pointers.
static int conv27_launch(ConvLaunchH& L, int N, int Cin, int Cout, int Z, int S, int waves, int ups, bool res, bool fused,
                         int res_half = 0) {
  if (Z < 1 || Z > 8) return fail(TM_ERR_ARG, "Z must be in 1 .. 8 (got %d)", Z);
  if (ups && Z != 2) return fail(TM_ERR_ARG, "upsampled-input form (ups): Z == 2 only (got Z = %d)", Z);
  if (res_half && Z != 2) return fail(TM_ERR_ARG, "half-resolution residual (res_half): Z == 2 only (got Z = %d)", Z);
  if (waves != 0 && waves != 4 && waves != 8 && waves != 9) return fail(TM_ERR_ARG, "waves must be 0 (auto), 4, 8 or 9 (lockstep 8-wave form)");
  if (fused && Cout != 64 && Cout != 128) return fail(TM_ERR_ARG, "fused epilogue needs Cout in {64, 128}");
  if (ups && (Cout % 128 || res)) return fail(TM_ERR_ARG, "upsampled-input form: Cout a multiple of 128, no residual");
  const int So = ups ? 2 * S : S;
  L.x = view_h16(nullptr, N, ((Cin + 7) / 8 + 1) / 2 * 16, Z, S, S);
  L.Cout = Cout; L.force_waves = waves; L.ups = ups;
  L.y = cb8_view(nullptr, N, Cout, Z, So, So);
  if (fused) { L.fuse_norm = 1; L.a2 = view_h16(nullptr, N, Cout, Z, So, So); }
  return TM_OK;
}
// shared body of the 16-bit 3x3x3 conv test entry points: fp32 CB8 input -> 16-bit CB8 (prep kernel), then the conv
static int op_conv27_h16(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin, int Cout,
                         int Z, int S, int dtype, int waves, const void* norm_w_host, const void* scale_host, const void* shift_host,
                         int per_image, void* a2_out, void* stream, const void* res_h16 = nullptr, void* y_h16 = nullptr,
                         int ups = 0, int res_half = 0) {
  if (!is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_BF16 or TM_DTYPE_F16");
  const bool f16 = dtype == TM_DTYPE_F16, fused = norm_w_host != nullptr;
  if (fused && (!scale_host || !shift_host || !a2_out || per_image < 1))
    return fail(TM_ERR_ARG, "fused epilogue needs scale / shift / a2 and per_image >= 1");
  ConvLaunchH L;
  if (int rc = conv27_launch(L, N, Cin, Cout, Z, S, waves, ups, res_h16 != nullptr, fused, res_half)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Cbi = (Cin + 7) / 8, nimg = (N + per_image - 1) / per_image;
  std::vector<uint16_t> pk(ups ? conv_bf16_pack_ups_elems(Cout, Cbi) : conv_bf16_pack_elems(Cout, Cbi));
  if (ups) (f16 ? conv_f16_pack_ups_host : conv_bf16_pack_ups_host)((const float*)w_host, Cout, &Cin, 1, pk.data());
  else (f16 ? conv_f16_pack_host : conv_bf16_pack_host)((const float*)w_host, Cout, &Cin, 1, pk.data());
  DevTmp tmp;
  std::tie(L.w, L.bias) = upload_conv(tmp, pk, bias_host, Cout);
  if (fused) {                                          // norm_w [Cout], scale / shift [nimg][Cout]
    L.norm_w = tmp.alloc(Cout, (const float*)norm_w_host);
    L.mod_scale = tmp.alloc((size_t)nimg * Cout, (const float*)scale_host);
    L.mod_shift = tmp.alloc((size_t)nimg * Cout, (const float*)shift_host);
    L.mod_stride = Cout; L.per_image = per_image; L.a2.p = (uint16_t*)a2_out;
  }
  if (tmp.err) return tmp.report();
  hipError_t e = hipSuccess;
  L.x = to_h16(tmp, cb8_view(const_cast<void*>(x_cb8), N, Cin, Z, S, S), f16, true, st, e);
  L.y.p = (float*)y_cb8;
  L.res_half = res_half;
  TVH resh = as_h(L.y);
  if (res_h16) {
    resh.p = (uint16_t*)const_cast<void*>(res_h16); L.res_h = &resh;
    if (res_half) { resh.H = L.y.H / 2; resh.W = L.y.W / 2; resh.nstride = L.y.nstride / 4; }
  }
  if (y_h16) { L.y_h = (uint16_t*)y_h16; L.yh_nstride = L.y.nstride; }
  if (e == hipSuccess) e = (f16 ? launch_conv27_f16 : launch_conv27_bf16)(L, st);
  return finish(st, e, "conv27 (16-bit)");
}
extern "C" int tm_op_conv27_h16_z(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                  int Cout, int S, int dtype, int waves, const void* res_h16, void* y_h16, int ups, int res_half,
                                  int Z, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || (!y_cb8 && !y_h16)) return fail(TM_ERR_ARG, "null argument");
  return op_conv27_h16(x_cb8, w_host, bias_host, y_cb8 ? y_cb8 : y_h16, N, Cin, Cout, Z, S, dtype, waves, nullptr, nullptr, nullptr, 1,
                       nullptr, stream, res_h16, y_h16, ups, res_half);
}
extern "C" int tm_op_conv27_bf16(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                 int Cout, int S, int dtype, int waves, const void* res_h16, void* y_h16, int ups, int res_half,
                                 void* stream) {
  return tm_op_conv27_h16_z(x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, S, dtype, waves, res_h16, y_h16, ups, res_half, 2, stream);
}
extern "C" int tm_op_conv27_fused_z(const void* x_cb8, const void* w_host, const void* bias_host, const void* norm_w_host,
                                    const void* scale_host, const void* shift_host, void* a2_out, int N, int Cin, int Cout,
                                    int S, int per_image, int dtype, int waves, int Z, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || !norm_w_host || !a2_out) return fail(TM_ERR_ARG, "null argument");
  // the launcher takes the output geometry from `y`; the fused form never writes it
  return op_conv27_h16(x_cb8, w_host, bias_host, a2_out, N, Cin, Cout, Z, S, dtype, waves, norm_w_host, scale_host, shift_host,
                       per_image, a2_out, stream);
}
extern "C" int tm_op_conv27_fused(const void* x_cb8, const void* w_host, const void* bias_host, const void* norm_w_host,
                                  const void* scale_host, const void* shift_host, void* a2_out, int N, int Cin, int Cout,
                                  int S, int per_image, int dtype, int waves, void* stream) {
  return tm_op_conv27_fused_z(x_cb8, w_host, bias_host, norm_w_host, scale_host, shift_host, a2_out, N, Cin, Cout, S, per_image,
                              dtype, waves, 2, stream);
}
// Timing hook of the 16-bit 3x3x3 conv on random device data (uniform in [-1, 1): the clock the chip holds depends on the
// operand bits, cdna guide rule 25): the model's launch forms -- 16-bit stream output with an optional 16-bit residual, the
// fused norm epilogue, the upsampled-input form -- `iters` launches between two events after one warm-up launch.
__global__ void fill_h16_kernel(uint16_t* p, size_t n, unsigned seed, int f16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned hsh = (unsigned)i * 2654435761u ^ (unsigned)(i >> 32) * 40503u ^ seed;
    hsh ^= hsh >> 15; hsh *= 2246822519u; hsh ^= hsh >> 13; hsh *= 3266489917u; hsh ^= hsh >> 16;
    const float v = (float)(hsh >> 8) * (1.0f / 8388608.0f) - 1.0f;
    uint16_t u;
    if (f16) { const _Float16 hf = (_Float16)v; u = __builtin_bit_cast(uint16_t, hf); }
    else { const __bf16 bf = (__bf16)v; u = __builtin_bit_cast(uint16_t, bf); }
    p[i] = u;
  }
}
extern "C" int tm_op_conv27_time(int N, int Cin, int Cout, int S, int dtype, int waves, int ups, int with_res, int fused,
                                 int iters, float* ms_per_launch, void* stream) {
  if (!is_h16(dtype) || iters < 1 || !ms_per_launch || N < 1) return fail(TM_ERR_ARG, "bad argument");
  ConvLaunchH L;
  if (int rc = conv27_launch(L, N, Cin, Cout, 2, S, waves, ups, with_res, fused)) return rc;
  const bool f16 = dtype == TM_DTYPE_F16;
  hipStream_t st = (hipStream_t)stream;
  const int Cbi = (Cin + 7) / 8, nt64 = (Cout + 63) / 64;
  const size_t nw = ups ? conv_bf16_pack_ups_elems(Cout, Cbi) : conv_bf16_pack_elems(Cout, Cbi);
  const size_t nx = (size_t)N * L.x.nstride, ny = (size_t)N * L.y.nstride;
  const size_t nf = (size_t)nt64 * 64 + (size_t)Cout * 3;                  // bias | norm_w | scale | shift
  std::vector<float> fp(nf);
  for (size_t i = 0; i < nf; ++i) fp[i] = 0.01f * (float)((int)(i * 37 % 101) - 50);
  for (int i = 0; i < Cout; ++i) fp[(size_t)nt64 * 64 + i] = 1.0f + 0.001f * (float)(i % 17);      // norm_w
  DevTmp tmp;
  uint16_t *dw = tmp.alloc<uint16_t>(nw), *dx = tmp.alloc<uint16_t>(nx), *dy = tmp.alloc<uint16_t>(ny);
  uint16_t* dr = with_res ? tmp.alloc<uint16_t>(ny) : nullptr;
  const float* df = tmp.alloc(nf, fp.data());
  hipEvent_t e0 = tmp.event(), e1 = tmp.event();
  if (tmp.err) return tmp.report();
  hipLaunchKernelGGL(fill_h16_kernel, dim3(2048), dim3(256), 0, st, dw, nw, 11u, f16 ? 1 : 0);
  hipLaunchKernelGGL(fill_h16_kernel, dim3(2048), dim3(256), 0, st, dx, nx, 23u, f16 ? 1 : 0);
  if (with_res) hipLaunchKernelGGL(fill_h16_kernel, dim3(2048), dim3(256), 0, st, dr, ny, 37u, f16 ? 1 : 0);
  HIP_TRY(hipStreamSynchronize(st));
  L.x.p = dx; L.w = dw; L.bias = df;
  L.y.p = (float*)dy; L.y_h = dy; L.yh_nstride = L.y.nstride;
  TVH resh = as_h(L.y);
  if (with_res) { resh.p = dr; L.res_h = &resh; }
  if (fused) {
    L.norm_w = df + nt64 * 64; L.mod_scale = L.norm_w + Cout; L.mod_shift = L.mod_scale + Cout;
    L.mod_stride = 0; L.per_image = N; L.a2.p = dy;
  }
  const auto conv = f16 ? launch_conv27_f16 : launch_conv27_bf16;
  hipError_t e = conv(L, st);                                             // warm-up
  if (e == hipSuccess) e = hipEventRecord(e0, st);
  for (int i = 0; i < iters && e == hipSuccess; ++i) e = conv(L, st);
  if (e == hipSuccess) e = hipEventRecord(e1, st);
  *ms_per_launch = 0.f;
  const int rc = finish(st, e, "conv27 (16-bit)");
  if (rc == TM_OK) { (void)hipEventElapsedTime(ms_per_launch, e0, e1); *ms_per_launch /= (float)iters; }
  return rc;
}
extern "C" int tm_op_conv1_bf16(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                int Cout, int Z, int S, int gelu, int dtype, int waves, const void* res_h16, const void* gate_h16,
                                void* y_h16, void* stream) {
  return tm_op_conv1_h16_gate(x_cb8, w_host, bias_host, y_cb8, N, Cin, Cout, Z, S, gelu, dtype, waves, res_h16, gate_h16, y_h16, 0,
                              (Cout + 7) / 8, 0, stream);
}
extern "C" int tm_op_conv1_h16_gate(const void* x_cb8, const void* w_host, const void* bias_host, void* y_cb8, int N, int Cin,
                                    int Cout, int Z, int S, int gelu, int dtype, int waves, const void* res_h16,
                                    const void* gate_h16, void* y_h16, int gate_half, int gate_cbtot, int gate_cb0, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || (!y_cb8 && !y_h16)) return fail(TM_ERR_ARG, "null argument");
  if (!y_cb8) y_cb8 = y_h16;                              // geometry carrier only
  if (!is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_BF16 or TM_DTYPE_F16");
  if (waves != 0 && waves != 4 && waves != 8) return fail(TM_ERR_ARG, "waves must be 0 (auto), 4 or 8");
  if (gate_half && !gate_h16) return fail(TM_ERR_ARG, "gate_half without a gate");
  if (gate_half && !half_gate_ok(S)) return fail(TM_ERR_ARG, "gate_half: S must be a power of two >= 2 (got %d)", S);
  if (gate_h16 && (gate_cb0 < 0 || gate_cb0 + (Cout + 7) / 8 > gate_cbtot))
    return fail(TM_ERR_ARG, "gate slice: blocks [%d, %d) run past the %d blocks of the tensor", gate_cb0, gate_cb0 + (Cout + 7) / 8,
                gate_cbtot);
  const bool f16 = dtype == TM_DTYPE_F16;
  hipStream_t st = (hipStream_t)stream;
  std::vector<uint16_t> pk(conv1_bf16_pack_elems(Cout, (Cin + 7) / 8));
  (f16 ? conv1_f16_pack_host : conv1_bf16_pack_host)((const float*)w_host, Cout, &Cin, 1, pk.data());
  DevTmp tmp;
  ConvLaunchH L;
  std::tie(L.w, L.bias) = upload_conv(tmp, pk, bias_host, Cout);
  if (tmp.err) return tmp.report();
  hipError_t e = hipSuccess;
  L.x = to_h16(tmp, cb8_view(const_cast<void*>(x_cb8), N, Cin, Z, S, S), f16, true, st, e);
  L.Cout = Cout; L.flags = gelu ? EPI_GELU : 0; L.force_waves = waves;
  L.y = cb8_view(y_cb8, N, Cout, Z, S, S);
  TVH resh = as_h(L.y), gateh;
  if (res_h16) { resh.p = (uint16_t*)const_cast<void*>(res_h16); L.res_h = &resh; }
  if (gate_h16) {                                         // [N][gate_cbtot][Z][Sg][Sg][8], blocks from gate_cb0
    const int Sg = gate_half ? S / 2 : S;
    gateh = view_h16(const_cast<void*>(gate_h16), N, gate_cbtot * 8, Z, Sg, Sg).blocks(gate_cb0, L.y.Cb);
    L.gate_h = &gateh;
    L.gate_half = gate_half ? 1 : 0;
  }
  if (y_h16) { L.y_h = (uint16_t*)y_h16; L.yh_nstride = L.y.nstride; }
  if (e == hipSuccess) e = (f16 ? launch_conv1_f16 : launch_conv1_bf16)(L, st);
  return finish(st, e, "conv1 (16-bit)");
}
extern "C" int tm_op_conv1_concat(const void* const* x_cb8, const int* cin, const int* collage, int nsrc, const void* w_host,
                                  const void* bias_host, void* y_cb8, int N, int Cout, int Z, int S, int p1, int p2,
                                  int dtype, int waves, void* stream) {
  if (!x_cb8 || !cin || !collage || !w_host || !bias_host || !y_cb8 || nsrc < 1 || nsrc > 3) return fail(TM_ERR_ARG, "bad argument");
  if (!is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_BF16 or TM_DTYPE_F16");
  const bool f16 = dtype == TM_DTYPE_F16;
  hipStream_t st = (hipStream_t)stream;
  bool any_col = false;
  for (int i = 0; i < nsrc; ++i) any_col = any_col || collage[i];
  const int q = any_col ? (p1 - 1) * (p2 - 1) : 1;
  if (any_col && (p1 < 2 || p2 < 2 || N % q)) return fail(TM_ERR_ARG, "collage needs N = b * (p1-1) * (p2-1)");
  const int Nsrc_col = any_col ? N / q * p1 * p2 : N;      // a collaged source lives on the (p1 x p2) grid
  int Cbi = 0;
  for (int i = 0; i < nsrc; ++i) Cbi += (cin[i] + 7) / 8;
  std::vector<uint16_t> pk(conv1_bf16_pack_elems(Cout, Cbi));
  (f16 ? conv1_f16_pack_host : conv1_bf16_pack_host)((const float*)w_host, Cout, cin, nsrc, pk.data());
  DevTmp tmp;
  ConvLaunchH L;
  std::tie(L.w, L.bias) = upload_conv(tmp, pk, bias_host, Cout);
  if (tmp.err) return tmp.report();
  hipError_t e = hipSuccess;
  for (int i = 0; i < nsrc; ++i) {
    L.xs[i] = to_h16(tmp, cb8_view(const_cast<void*>(x_cb8[i]), collage[i] ? Nsrc_col : N, cin[i], Z, S, S), f16, false, st, e);
    L.xs_collage[i] = collage[i] ? 1 : 0;
  }
  L.nsrc = nsrc; L.p1 = p1; L.p2 = p2;
  L.x = view_h16(nullptr, N, (Cbi + 1) / 2 * 16, Z, S, S);
  L.x.nstride = 0;
  L.Cout = Cout; L.force_waves = waves;
  L.y = cb8_view(y_cb8, N, Cout, Z, S, S);
  if (e == hipSuccess) e = (f16 ? launch_conv1_f16 : launch_conv1_bf16)(L, st);
  return finish(st, e, "conv1 concat");
}
// the tail of the three prep hooks: `iters` launches of P under launch_prep's variant knob (set and reset around them only);
// elapsed_ms (host, optional): mean time of launches 2..iters
static int prep_run(const PrepLaunch& P, int variant, int iters, float* elapsed_ms, hipStream_t st, const char* what) {
  DevTmp tmp;
  hipEvent_t e0 = elapsed_ms ? tmp.event() : nullptr, e1 = elapsed_ms ? tmp.event() : nullptr;
  if (tmp.err) return tmp.report();
  set_prep_variant(variant);
  hipError_t e = launch_prep(P, st);                                   // warm-up / the result
  if (elapsed_ms && e == hipSuccess) e = hipEventRecord(e0, st);
  for (int i = 1; i < iters && e == hipSuccess; ++i) e = launch_prep(P, st);
  if (elapsed_ms && e == hipSuccess) e = hipEventRecord(e1, st);
  set_prep_variant(0);
  const int rc = finish(st, e, what);
  if (elapsed_ms) {
    *elapsed_ms = 0.f;
    if (rc == TM_OK && iters > 1) { (void)hipEventElapsedTime(elapsed_ms, e0, e1); *elapsed_ms /= (float)(iters - 1); }
  }
  return rc;
}
extern "C" int tm_op_prep_h16(const void* const* src_h16, const int* src_c, const int* collage, int nsrc, int N, int Z, int S,
                              int p1, int p2, int up2, const void* norm_w_dev, int c_real, int mod, const void* mod_scale,
                              const void* mod_shift, long mod_stride, int per_image, int act, int dtype, int variant,
                              void* out_h16, void* raw_h16, int iters, float* elapsed_ms, void* stream) {
  if (!src_h16 || !src_c || !collage || !out_h16 || nsrc < 1 || nsrc > 3 || iters < 1) return fail(TM_ERR_ARG, "bad argument");
  if (!is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_BF16 or TM_DTYPE_F16");
  if (mod != MOD_NONE && (!mod_scale || !mod_shift)) return fail(TM_ERR_ARG, "modulation tensors missing");
  hipStream_t st = (hipStream_t)stream;
  bool any_col = false;
  for (int i = 0; i < nsrc; ++i) any_col = any_col || collage[i];
  const int q = any_col ? (p1 - 1) * (p2 - 1) : 1;
  if (any_col && (p1 < 2 || p2 < 2 || N % q)) return fail(TM_ERR_ARG, "collage needs N = b * (p1-1) * (p2-1)");
  if (up2 < 0 || up2 > 2) return fail(TM_ERR_ARG, "up2: 0 same, 1 nearest x2, 2 = 2 x 2 average (Downsample)");
  if (up2 == 1 && (any_col || (S & 1))) return fail(TM_ERR_ARG, "up2 takes plain sources and an even S");
  if (up2 == 2 && (any_col || nsrc != 1 || mod != MOD_NONE)) return fail(TM_ERR_ARG, "the downsample form takes one plain source, no modulation");
  const int Ss = up2 == 1 ? S / 2 : (up2 == 2 ? 2 * S : S);
  PrepLaunch P = prep_start(N, Z, S);
  const int cbtot = prep_op_sources(P, src_h16, src_c, collage, nsrc, Z, Ss, true);
  const int cbe = pair_cb(cbtot);
  P.h_f16 = dtype == TM_DTYPE_F16;
  P.resample = up2 == 1 ? RS_UP2 : (up2 == 2 ? RS_DOWN2 : RS_SAME); P.p1 = p1; P.p2 = p2;
  prep_norm(P, (const float*)norm_w_dev, c_real);
  P.act = act; P.per_image = per_image > 0 ? per_image : 1;
  P.mod = mod; P.mod_stride = mod_stride;
  if (mod == MOD_IMAGE) { P.mod_scale = (const float*)mod_scale; P.mod_shift = (const float*)mod_shift; }
  if (mod == MOD_VOXEL) { P.mod_scale_h = (const uint16_t*)mod_scale; P.mod_shift_h = (const uint16_t*)mod_shift; }
  prep_out_h(P, view_h16(out_h16, N, cbe * 8, Z, S, S), cbtot);
  if (raw_h16) prep_raw_h(P, view_h16(raw_h16, N, cbe * 8, Z, S, S));
  return prep_run(P, variant, iters, elapsed_ms, st, "prep");
}
extern "C" int tm_op_prep_f32(const void* const* src_cb8, const int* src_c, const int* collage, int nsrc, int N, int Z, int S,
                              int p1, int p2, int up2, const void* norm_w_dev, int c_real, int mod, const void* mod_scale,
                              const void* mod_shift, long mod_stride, int mod_half, int per_image, int act, int variant,
                              void* out_cb8, void* raw_cb8, int iters, float* elapsed_ms, void* stream) {
  if (!src_cb8 || !src_c || !collage || !out_cb8 || nsrc < 1 || nsrc > 3 || iters < 1) return fail(TM_ERR_ARG, "bad argument");
  if (N < 1 || Z < 1 || S < 1) return fail(TM_ERR_ARG, "N, Z and S must be positive");
  if (variant < 0 || variant > 2) return fail(TM_ERR_ARG, "variant: 0 automatic, 1 four-wave kernel, 2 wide form");
  if (mod != MOD_NONE && (!mod_scale || !mod_shift)) return fail(TM_ERR_ARG, "modulation tensors missing");
  if (mod_half && (mod != MOD_VOXEL || (S & 1))) return fail(TM_ERR_ARG, "mod_half takes a per-voxel modulation and an even S");
  hipStream_t st = (hipStream_t)stream;
  bool any_col = false;
  for (int i = 0; i < nsrc; ++i) any_col = any_col || collage[i];
  const int q = any_col ? (p1 - 1) * (p2 - 1) : 1;
  if (any_col && (p1 < 2 || p2 < 2 || N % q)) return fail(TM_ERR_ARG, "collage needs N = b * (p1-1) * (p2-1)");
  if (up2 < 0 || up2 > 1) return fail(TM_ERR_ARG, "up2: 0 same, 1 nearest x2");
  if (up2 == 1 && (any_col || (S & 1))) return fail(TM_ERR_ARG, "up2 takes plain sources and an even S");
  const int Ss = up2 == 1 ? S / 2 : S;
  PrepLaunch P = prep_start(N, Z, S);
  const int cbtot = prep_op_sources(P, src_cb8, src_c, collage, nsrc, Z, Ss, false);
  P.resample = up2 == 1 ? RS_UP2 : RS_SAME; P.p1 = p1; P.p2 = p2;
  prep_norm(P, (const float*)norm_w_dev, c_real);
  P.act = act; P.per_image = per_image > 0 ? per_image : 1;
  P.mod = mod; P.mod_stride = mod_stride; P.mod_half = mod_half ? 1 : 0;
  P.mod_scale = (const float*)mod_scale; P.mod_shift = (const float*)mod_shift;
  prep_out(P, cb8_view(out_cb8, N, cbtot * 8, Z, S, S));
  if (raw_cb8) prep_raw(P, cb8_view(raw_cb8, N, cbtot * 8, Z, S, S));
  if (variant == 2 && !prep_wide_applies(P))
    return fail(TM_ERR_ARG, "the wide form takes 33..%d channel blocks (this call has %d)", PREP_WIDE_MAX_CB, cbtot);
  return prep_run(P, variant, iters, elapsed_ms, st, "prep (fp32)");
}
// One PrepLaunch as the executor fills it, in every combination of types launch_prep takes; the form is launch_prep's choice.
extern "C" int tm_op_prep_form(const void* const* src, const int* src_c, const int* collage, int nsrc, int N, int Z, int S,
                               int p1, int p2, int resample, int src_dtype, int out_dtype, const void* norm_w_dev, int c_real,
                               int mod, int mod_dtype, const void* mod_scale, const void* mod_shift, long mod_stride, int mod_half,
                               int per_image, int act, int variant, int pad_blocks, void* out, void* raw, int raw_dtype,
                               int iters, float* elapsed_ms, void* stream) {
  if (!src || !src_c || !collage || !out || nsrc < 1 || nsrc > 3 || iters < 1) return fail(TM_ERR_ARG, "bad argument");
  if (N < 1 || Z < 1 || S < 1 || c_real < 1) return fail(TM_ERR_ARG, "N, Z, S and c_real must be positive");
  if (variant < 0 || variant > 3) return fail(TM_ERR_ARG, "variant: 0 automatic, 1 generic kernel, 2 | 3 the 16-bit forms (2: the wide fp32 form)");
  const bool voxel = mod == MOD_VOXEL;
  const int types[4] = {src_dtype, out_dtype, voxel ? mod_dtype : TM_DTYPE_F32, raw ? raw_dtype : TM_DTYPE_F32};
  int h = TM_DTYPE_F32;
  for (int t : types) {
    if (t != TM_DTYPE_F32 && !is_h16(t)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_F32, TM_DTYPE_BF16 or TM_DTYPE_F16");
    if (is_h16(t) && h != TM_DTYPE_F32 && t != h) return fail(TM_ERR_ARG, "bf16 and f16 tensors may not be mixed in one call");
    if (is_h16(t)) h = t;
  }
  if (mod < MOD_NONE || mod > MOD_VOXEL) return fail(TM_ERR_ARG, "mod: 0 none, 1 per image, 2 per voxel");
  if (mod != MOD_NONE && (!mod_scale || !mod_shift)) return fail(TM_ERR_ARG, "modulation tensors missing");
  if (mod == MOD_IMAGE && mod_dtype != TM_DTYPE_F32) return fail(TM_ERR_ARG, "per-image modulation rows are fp32");
  if (mod_half && (!voxel || (S & 1))) return fail(TM_ERR_ARG, "mod_half takes a per-voxel modulation and an even S");
  if (pad_blocks < 0 || (pad_blocks && !is_h16(out_dtype))) return fail(TM_ERR_ARG, "pad_blocks belong to a 16-bit output");
  bool any_col = false;
  for (int i = 0; i < nsrc; ++i) any_col = any_col || collage[i];
  const int q = any_col ? (p1 - 1) * (p2 - 1) : 1;
  if (any_col && (p1 < 2 || p2 < 2 || N % q)) return fail(TM_ERR_ARG, "collage needs N = b * (p1-1) * (p2-1)");
  if (resample < RS_SAME || resample > RS_PICK2) return fail(TM_ERR_ARG, "resample: 0 same, 1 up2, 2 down2, 3 pick2");
  if (resample == RS_UP2 && (any_col || (S & 1))) return fail(TM_ERR_ARG, "up2 takes plain sources and an even S");
  if (resample == RS_PICK2 && (S & 1)) return fail(TM_ERR_ARG, "pick2 takes an even S");
  if (resample == RS_DOWN2 && (any_col || nsrc != 1 || mod != MOD_NONE))
    return fail(TM_ERR_ARG, "the downsample form takes one plain source, no modulation");
  const int Ss = resample == RS_UP2 ? S / 2 : (resample == RS_SAME ? S : 2 * S);
  for (int i = 0; i < nsrc; ++i)
    if (!src[i] || src_c[i] < 1) return fail(TM_ERR_ARG, "bad source %d", i);
  PrepLaunch P = prep_start(N, Z, S);
  const int cbtot = prep_op_sources(P, src, src_c, collage, nsrc, Z, Ss, is_h16(src_dtype));
  P.h_f16 = h == TM_DTYPE_F16;
  P.resample = resample; P.p1 = p1; P.p2 = p2;
  prep_norm(P, (const float*)norm_w_dev, c_real);
  P.act = act ? 1 : 0; P.per_image = per_image > 0 ? per_image : 1;
  P.mod = mod; P.mod_stride = mod_stride; P.mod_half = mod_half ? 1 : 0;
  if (voxel && is_h16(mod_dtype)) { P.mod_scale_h = (const uint16_t*)mod_scale; P.mod_shift_h = (const uint16_t*)mod_shift; }
  else if (mod != MOD_NONE) { P.mod_scale = (const float*)mod_scale; P.mod_shift = (const float*)mod_shift; }
  const int cb_h = cbtot + pad_blocks;                 // blocks of a 16-bit output / raw copy: the pad blocks behind the real ones
  if (is_h16(out_dtype)) prep_out_h(P, view_h16(out, N, cb_h * 8, Z, S, S), cbtot);
  else prep_out(P, cb8_view(out, N, cbtot * 8, Z, S, S));
  if (raw && is_h16(raw_dtype)) prep_raw_h(P, view_h16(raw, N, cb_h * 8, Z, S, S));
  else if (raw) prep_raw(P, cb8_view(raw, N, cbtot * 8, Z, S, S));
  // the forms a forced variant names must be the form launch_prep then takes
  const bool h16_call = P.src_h && P.out_h && !P.raw && resample != RS_DOWN2 && (!voxel || P.mod_scale_h);
  if (variant == 3 && !(h16_call && cbtot <= 160)) return fail(TM_ERR_ARG, "variant 3 takes an all-16-bit call of at most 160 blocks");
  if (variant == 2 && !(h16_call && cbtot <= 32) && !prep_wide_applies(P))
    return fail(TM_ERR_ARG, "variant 2 takes an all-16-bit call of at most 32 blocks, or the wide form's 33..%d fp32 blocks (this call has %d)",
                PREP_WIDE_MAX_CB, cbtot);
  hipStream_t st = (hipStream_t)stream;
  return prep_run(P, variant, iters, elapsed_ms, st, "prep (form)");
}

// The stem and the head on their own, weights packed as the model loader packs them (direct_pack_host)
extern "C" int tm_op_stem(const void* x, const void* w_host, const void* bias_host, void* y, int N, int Cin, int Cout, int Z, int S,
                          int dtype, void* stream) {
  if (!x || !w_host || !bias_host || !y) return fail(TM_ERR_ARG, "null pointer");
  if (N < 1 || Cin < 1 || Cout < 1 || Z < 1 || S < 1) return fail(TM_ERR_ARG, "N, Cin, Cout, Z and S must be positive");
  if (Cout % 32) return fail(TM_ERR_ARG, "the stem computes 32 couts per thread: Cout = %d is no multiple of 32", Cout);
  if (dtype != TM_DTYPE_F32 && !is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_F32, TM_DTYPE_BF16 or TM_DTYPE_F16");
  std::vector<float> wt((size_t)9 * Cin * Cout);
  direct_pack_host((const float*)w_host, Cout, Cin, 9, wt.data());
  DevTmp tmp;
  const float* w = tmp.alloc(wt.size(), wt.data());
  const float* bias = tmp.alloc((size_t)Cout, (const float*)bias_host);
  if (tmp.err) return tmp.report();
  const bool h16 = is_h16(dtype);
  const TV yv = cb8_view(h16 ? nullptr : y, N, Cout, Z, S, S);
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_stem((const float*)x, yv, w, bias, Cin, st, h16 ? (uint16_t*)y : nullptr, yv.nstride, dtype == TM_DTYPE_F16), "stem");
}
extern "C" int tm_op_head(const void* x_cb8, const void* w_host, const void* bias_host, void* y, int N, int C, int Cout, int Z, int S,
                          int dtype, void* stream) {
  if (!x_cb8 || !w_host || !bias_host || !y) return fail(TM_ERR_ARG, "null pointer");
  if (N < 1 || C < 1 || Cout < 1 || Z < 1 || S < 1) return fail(TM_ERR_ARG, "N, C, Cout, Z and S must be positive");
  if (Cout > 8) return fail(TM_ERR_ARG, "the head computes at most 8 couts: Cout = %d", Cout);
  if (dtype != TM_DTYPE_F32 && !is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_F32, TM_DTYPE_BF16 or TM_DTYPE_F16");
  // the kernel walks whole channel blocks: cin zero padded to ceil(C / 8) * 8 before the loader's transpose
  const int Cp = (C + 7) / 8 * 8;
  std::vector<float> wp((size_t)Cout * Cp * 9, 0.f), wt((size_t)9 * Cp * 8);
  for (int co = 0; co < Cout; ++co)
    memcpy(wp.data() + (size_t)co * Cp * 9, (const float*)w_host + (size_t)co * C * 9, (size_t)C * 9 * sizeof(float));
  direct_pack_host(wp.data(), Cout, Cp, 9, wt.data());
  DevTmp tmp;
  const float* w = tmp.alloc(wt.size(), wt.data());
  const float* bias = tmp.alloc((size_t)Cout, (const float*)bias_host);
  if (tmp.err) return tmp.report();
  hipStream_t st = (hipStream_t)stream;
  const TV xv = cb8_view(const_cast<void*>(x_cb8), N, C, Z, S, S);
  return finish(st, launch_head(xv, (float*)y, w, bias, Cout, st, dtype == TM_DTYPE_F32 ? 0 : (dtype == TM_DTYPE_F16 ? 2 : 1)), "head");
}

// The timestep embedding and the emb_layers matrix on their own; every pointer is a device pointer
extern "C" int tm_op_time_embed(const void* t_dev, const void* w1, const void* b1, const void* w2, const void* b2, void* te,
                                void* te_act, int b, int ch, int E, void* stream) {
  if (!t_dev || !w1 || !b1 || !w2 || !b2 || !te || !te_act) return fail(TM_ERR_ARG, "null pointer");
  if (b < 1 || ch < 2 || (ch & 1) || E < 1) return fail(TM_ERR_ARG, "b and E must be positive, ch even and at least 2");
  if ((long)(ch + E) * 4 > 65536) return fail(TM_ERR_ARG, "ch + E = %d floats do not fit 64 KB of LDS", ch + E);
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_time_embed((const int64_t*)t_dev, b, ch, E, (const float*)w1, (const float*)b1, (const float*)w2,
                                      (const float*)b2, (float*)te, (float*)te_act, st), "time_embed");
}
extern "C" int tm_op_emb_all(const void* te_act, const void* wall, const void* ball, void* ss, int b, int E, int tot, void* stream) {
  if (!te_act || !wall || !ball || !ss) return fail(TM_ERR_ARG, "null pointer");
  if (b < 1 || tot < 1 || E < 64) return fail(TM_ERR_ARG, "b and tot must be positive, E at least 64");
  if (E % 64 || E > 1024) return fail(TM_ERR_ARG, "a wave splits a row over 64 lanes, 16 floats each: E = %d must be a multiple of 64, at most 1024", E);
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_emb_all((const float*)te_act, b, E, (const float*)wall, (const float*)ball, tot, (float*)ss, st), "emb_all");
}

extern "C" int tm_op_window_attn(const void* q_cb8, const void* k_cb8, const void* v_cb8, const void* qw_dev,
                                 const void* kw_dev, void* out, int N, int C, int Z, int S, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (C % 64) return fail(TM_ERR_ARG, "C must be a multiple of 64");
  const TV q = cb8_view(const_cast<void*>(q_cb8), N, C, Z, S, S), k = cb8_view(const_cast<void*>(k_cb8), N, C, Z, S, S);
  const TV v = cb8_view(const_cast<void*>(v_cb8), N, C, Z, S, S);
  const float *qw = (const float*)qw_dev, *kw = (const float*)kw_dev;
  if (dtype == TM_DTYPE_F32) return finish(st, launch_window_attn(q, k, v, qw, kw, cb8_view(out, N, C, Z, S, S), st), "window attention");
  DevTmp tmp;
  hipError_t e = hipSuccess;
  const TVH hq = to_h16(tmp, q, false, false, st, e), hk = to_h16(tmp, k, false, false, st, e), hv = to_h16(tmp, v, false, false, st, e);
  TVH o = hq;
  o.p = (uint16_t*)out;
  if (e == hipSuccess) e = launch_window_attn_bf16(hq, hk, hv, qw, kw, o, st);
  return finish(st, e, "window attention");
}
// The forms launch_window_attn / launch_window_attn_bf16 / _f16 take, as one readable list: TM_OK, or TM_ERR_ARG with the reason
// (the launchers themselves only answer hipErrorInvalidValue)
static int window_attn_form(int N, int C, int Z, int S, int dtype, int kv_half) {
  if (dtype != TM_DTYPE_F32 && !is_h16(dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_F32, TM_DTYPE_BF16 or TM_DTYPE_F16");
  if (N < 1 || Z < 1 || S < 2 || (S & 1)) return fail(TM_ERR_ARG, "N = %d, Z = %d, S = %d: N, Z >= 1 and an even S >= 2 (2 x 2 windows)", N, Z, S);
  if (C < 64 || C % 64) return fail(TM_ERR_ARG, "C = %d must be a positive multiple of 64", C);
  const long Tl = (long)Z * (S / 2) * (S / 2);
  if (Tl > 512) return fail(TM_ERR_ARG, "window of %ld tokens: the attention cores take at most 512", Tl);
  const int T = (int)Tl;
  const bool pow2 = !(S & (S - 1));
  if (dtype == TM_DTYPE_F32) {
    const bool mfma = T == 128 && C % 128 == 0, t32 = T == 32 && C % 128 == 0, lng = (T == 256 || T == 512) && C <= 256;
    if (mfma && C > 512) return fail(TM_ERR_ARG, "C = %d > 512 at a window of 128 tokens", C);
    if (!mfma && !t32 && !lng && C > 512) return fail(TM_ERR_ARG, "C = %d > 512: the generic fp32 core keeps C floats per query in LDS", C);
    if (kv_half && !((mfma || t32) && pow2 && S >= 4))
      return fail(TM_ERR_ARG, "half-resolution k / v (fp32): windows of 128 or 32 tokens, C a multiple of 128 and S a power of two >= 4 "
                              "(got %d tokens, C = %d, S = %d)", T, C, S);
    return TM_OK;
  }
  if (C > 512) return fail(TM_ERR_ARG, "C = %d > 512 (16-bit attention core)", C);
  if (T == 256 || T == 512) {
    if (C > 256) return fail(TM_ERR_ARG, "C = %d > 256 at a long window of %d tokens (16-bit two-pass core)", C, T);
    if (kv_half) return fail(TM_ERR_ARG, "half-resolution k / v is not implemented for long windows (%d tokens)", T);
    return TM_OK;
  }
  if (T != 128 && T != 64 && T != 32) return fail(TM_ERR_ARG, "window of %d tokens: the 16-bit attention cores take 32, 64, 128, 256 or 512", T);
  if (kv_half && (S & 3)) return fail(TM_ERR_ARG, "half-resolution k / v (16-bit): S = %d must be a multiple of 4", S);
  return TM_OK;
}

extern "C" int tm_op_window_attn_kv(const void* q_cb8, const void* kv_cb8, const void* qw_dev, const void* kw_dev, void* out, int N,
                                    int C, int Z, int S, int dtype, int kv_half, void* stream) {
  if (!q_cb8 || !kv_cb8 || !qw_dev || !kw_dev || !out) return fail(TM_ERR_ARG, "null argument");
  if (int rc = window_attn_form(N, C, Z, S, dtype, kv_half)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int cb = C / 8, Sc = kv_half ? S / 2 : S;
  const TV q = cb8_view(const_cast<void*>(q_cb8), N, C, Z, S, S), kv = cb8_view(const_cast<void*>(kv_cb8), N, 2 * C, Z, Sc, Sc);
  const float *qw = (const float*)qw_dev, *kw = (const float*)kw_dev;
  // k and v are the two channel-block halves of kv, as attn_block (tm_model.hip) hands them over: their n stride is kv's
  if (dtype == TM_DTYPE_F32)
    return finish(st, launch_window_attn(q, kv.blocks(0, cb), kv.blocks(cb, cb), qw, kw, cb8_view(out, N, C, Z, S, S), st), "window attention");
  const bool f16 = dtype == TM_DTYPE_F16;
  DevTmp tmp;
  hipError_t e = hipSuccess;
  const TVH hq = to_h16(tmp, q, f16, false, st, e), hkv = to_h16(tmp, kv, f16, false, st, e);
  TVH o = hq;
  o.p = (uint16_t*)out;
  if (e == hipSuccess) e = (f16 ? launch_window_attn_f16 : launch_window_attn_bf16)(hq, hkv.blocks(0, cb), hkv.blocks(cb, cb), qw, kw, o, st);
  return finish(st, e, "window attention");
}
// ---- gene-gene attention block (tm_attn.hip), one kernel form per call --------------------------------------------------------
// The twelve host arrays of the block in checkpoint layout ([out][in]) in the order tm_model_finalize packs them -> GeneW in `tmp`,
// the Linear weights transposed to [in][out].  `keep` holds the transposed host copies until the hook has synchronised.
static GeneW upload_gene_w(DevTmp& tmp, const void* const* wh, int D, std::vector<std::vector<float>>& keep) {
  auto mat = [&](int i, int rows, int cols) {
    keep.emplace_back((size_t)rows * cols);
    transpose_host((const float*)wh[i], rows, cols, keep.back().data());
    return (const float*)tmp.ordered_upload(keep.back().data(), keep.back().size());
  };
  auto vec = [&](int i, int n) { return (const float*)tmp.ordered_upload(wh[i], (size_t)n); };
  GeneW w;
  w.wq_t = mat(0, D, D); w.bq = vec(1, D);
  w.wv_t = mat(2, D, D); w.bv = vec(3, D);
  w.qnorm = vec(4, D);
  w.wp_t = mat(5, D, D); w.bp = vec(6, D);
  w.norm2 = vec(7, D);
  w.w1_t = mat(8, 4 * D, D); w.b1 = vec(9, 4 * D);
  w.w2_t = mat(10, D, 4 * D); w.b2 = vec(11, D);
  return w;
}
// The geometries launch_gene_attn / launch_gene_attn_generic / launch_gene_readout take, as one readable list: TM_OK and the
// resolved form in *f (1 = the fused D = 64 kernels, 2 = the generic kernel), or TM_ERR_ARG with the reason (the launchers
// themselves only answer hipErrorInvalidValue).  Beyond their rules: without a slot table gene g reads slot g of the 500 a slice
// of the dense tensor has, so G > 500 needs one, and its entries must be slots.
static int gene_attn_form(const void* rna, const void* const* wh, const int* gidx, int B, int gn, int zs, int G, int form, int* f) {
  if (!rna || !wh) return fail(TM_ERR_ARG, "null argument");
  for (int i = 0; i < 12; ++i)
    if (!wh[i]) return fail(TM_ERR_ARG, "null argument: w_host[%d]", i);
  if (form < 0 || form > 2) return fail(TM_ERR_ARG, "form = %d: 0 (the model's rule), 1 (fused D = 64 kernel) or 2 (generic kernel)", form);
  if (B < 1 || gn < 1 || zs < 1 || G < 1) return fail(TM_ERR_ARG, "B = %d, gn = %d, zs = %d, G = %d must all be >= 1", B, gn, zs, G);
  const long D = (long)gn * gn * zs;
  if (D > 512) return fail(TM_ERR_ARG, "D = gn^2 * zs = %ld > 512", D);
  if (G > 512) return fail(TM_ERR_ARG, "G = %d > 512", G);
  if (!gidx && G > 500) return fail(TM_ERR_ARG, "G = %d > 500 needs a gene slot table (a slice of the dense tensor has 500 slots)", G);
  for (int g = 0; gidx && g < G; ++g)
    if (gidx[g] < 0 || gidx[g] >= 500) return fail(TM_ERR_ARG, "gene slot gidx[%d] = %d outside [0, 500)", g, gidx[g]);
  *f = form ? form : (gene_mfma_rule((int)D, G, gidx != nullptr) ? 1 : 2);
  if (*f == 1) {
    if (D != 64) return fail(TM_ERR_ARG, "gn^2 * zs = %ld != D = 64 of the fused kernel", D);
    if (G > 232) return fail(TM_ERR_ARG, "G = %d > 232 (fused kernel: the tokens of a patch live in LDS)", G);
    if (gidx) return fail(TM_ERR_ARG, "the fused kernel takes no gene slot table");
  }
  return TM_OK;
}

extern "C" int tm_op_gene_attn(const void* rna_dense_dev, const void* const* w_host, const int* gidx_host, int B, int gn, int zs,
                               int G, int form, int zlo, int zhi, void* out_tok_cb8, void* attn_map, void* stream) {
  int f = 0;
  if (int rc = gene_attn_form(rna_dense_dev, w_host, gidx_host, B, gn, zs, G, form, &f)) return rc;
  if (!out_tok_cb8 && !attn_map) return fail(TM_ERR_ARG, "null argument: one of out_tok_cb8 and attn_map is required");
  if (zlo < 0 || zlo > zhi || zhi > zs) return fail(TM_ERR_ARG, "slice mask [%d, %d) outside [0, %d]", zlo, zhi, zs);
  const int D = gn * gn * zs;
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp(st);
  std::vector<std::vector<float>> keep;
  const GeneW w = upload_gene_w(tmp, w_host, D, keep);
  const int* gidx = gidx_host ? (const int*)tmp.ordered_upload(gidx_host, (size_t)G) : nullptr;
  float* ws = f == 2 ? tmp.ordered_floats((size_t)B * gene_generic_split(B) * gene_generic_ws_floats(G, D), false) : nullptr;
  if (tmp.err) return (void)hipStreamSynchronize(st), tmp.report();      // `keep` may still be the source of a queued copy
  const float* rna = (const float*)rna_dense_dev;
  const hipError_t e = f == 1 ? launch_gene_attn(rna, B, gn, zs, G, w, (float*)out_tok_cb8, (float*)attn_map, zlo, zhi, st)
                              : launch_gene_attn_generic(rna, B, gn, zs, G, D, w, gidx, (float*)out_tok_cb8, (float*)attn_map, zlo, zhi, ws, st);
  return finish(st, e, "gene attention");
}

extern "C" int tm_op_rna_mid(const void* rna_dense_dev, int B, int gn, int zs, int G, void* out, void* stream) {
  if (!rna_dense_dev || !out) return fail(TM_ERR_ARG, "null argument");
  if (B < 1 || gn < 1 || zs < 1 || G < 1 || G > 500) return fail(TM_ERR_ARG, "B = %d, gn = %d, zs = %d >= 1 and 1 <= G = %d <= 500", B, gn, zs, G);
  return finish((hipStream_t)stream, launch_rna_mid((const float*)rna_dense_dev, B, gn, zs, G, (float*)out, (hipStream_t)stream), "rna_mid");
}

extern "C" int tm_op_gene_readout(const void* rna_dense_dev, const void* const* w_host, const int* gidx_host, int B, int gn, int zs,
                                  int G, const int* glst, int K, int form, void* out, void* sub, void* stream) {
  if (!glst || !out) return fail(TM_ERR_ARG, "null argument");
  int f = 0;
  if (int rc = gene_attn_form(rna_dense_dev, w_host, gidx_host, B, gn, zs, G, form, &f)) return rc;
  if (int rc = gene_readout_args(zs, glst, K, G)) return rc;
  const int D = gn * gn * zs;
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp(st);
  std::vector<std::vector<float>> keep;
  const GeneW w = upload_gene_w(tmp, w_host, D, keep);
  const int* gidx = gidx_host ? (const int*)tmp.ordered_upload(gidx_host, (size_t)G) : nullptr;
  float* ws = f == 2 ? tmp.ordered_floats(gene_readout_ws_floats(B, G, D), false) : nullptr;
  if (tmp.err) return (void)hipStreamSynchronize(st), tmp.report();
  const float* rna = (const float*)rna_dense_dev;
  const hipError_t e = f == 1 ? launch_gene_readout(rna, B, gn, zs, G, w, glst, K, (float*)out, (float*)sub, st)
                              : launch_gene_readout_chunks(rna, B, gn, zs, G, D, w, gidx, glst, K, (float*)out, (float*)sub, ws, st);
  return finish(st, e, "gene read-out");
}

extern "C" int tm_op_conv_direct(const void* x, const void* w_host, const void* bias_host, void* y, int N, int Cin,
                                 int Cout, int Zin, int S, int kz, int ky, int kx, int pz, int py, int px, int silu_in,
                                 int up2_out, void* stream) {
  const int taps = kz * ky * kx, Cop = (Cout + 7) / 8 * 8;
  const int Zout = Zin + 2 * pz - kz + 1;
  if (Zout < 1 || py != ky / 2 || px != kx / 2) return fail(TM_ERR_ARG, "unsupported geometry");
  std::vector<float> wt((size_t)taps * Cin * Cop);
  direct_pack_host((const float*)w_host, Cout, Cin, taps, wt.data());
  DevTmp tmp;
  DirectLaunch L;
  std::tie(L.w, L.bias) = upload_conv(tmp, wt, bias_host, Cout);
  if (tmp.err) return tmp.report();
  L.x = (const float*)x; L.ax = acc_ncdhw(Cin, Zin, S, S);
  const int So = up2_out ? 2 * S : S;
  L.y = (float*)y; L.ay = acc_ncdhw(Cout, Zout, So, So);
  L.N = N; L.Cin = Cin; L.Cout = Cout; L.Zin = Zin; L.Zout = Zout; L.S = S;
  L.kz = kz; L.ky = ky; L.kx = kx; L.pz = pz; L.py = py; L.px = px; L.silu_in = silu_in; L.up2_out = up2_out;
  return finish((hipStream_t)stream, launch_conv_direct(L, (hipStream_t)stream), "conv_direct");
}

// ------------------------------------------------------------------------------------------
// training slice: forward with dropout + backward of one ResBlock's pieces
// ------------------------------------------------------------------------------------------
// dropout probability p -> the drawn mask's threshold (drop iff word < thr) and 1 / (1 - p), both as DESIGN §8 fixes them
static bool drop_rng_of(unsigned long long key, unsigned site, float p, DropRng& r, float& scale) {
  if (!(p >= 0.f && p < 1.f)) return false;
  r.key = key; r.site = site;
  r.thr = (uint32_t)std::min(std::floor((double)p * 4294967296.0), 4294967295.0);
  scale = 1.0f / (float)(1.0 - (double)p);
  return true;
}

static int prep_train_impl(const void* x_cb8, const void* norm_w_host, const void* scale_host, const void* shift_host,
                           const void* mask_cb8, float drop_scale, const DropRng* rng, int per_image, void* y_cb8, int N, int C, int Z,
                           int S, void* stream) {
  if (!x_cb8 || !norm_w_host || !y_cb8 || per_image < 1) return fail(TM_ERR_ARG, "bad argument");
  const int Cb = (C + 7) / 8, Cp = Cb * 8, nimg = (N + per_image - 1) / per_image;
  DevTmp tmp;
  const float* dw = upload_rows(tmp, norm_w_host, 1, C, Cp);
  const float *dsc = nullptr, *dsh = nullptr;
  if (scale_host) { dsc = upload_rows(tmp, scale_host, nimg, C, Cp); dsh = upload_rows(tmp, shift_host, nimg, C, Cp); }
  if (tmp.err) return tmp.report();
  TV x = cb8_view(const_cast<void*>(x_cb8), N, C, Z, S, S), y = cb8_view(y_cb8, N, C, Z, S, S);
  PrepLaunch P = prep_start(N, Z, S);
  prep_src(P, x);
  prep_norm(P, dw, C);
  P.act = 1; P.per_image = per_image;
  if (dsc) { P.mod = MOD_IMAGE; P.mod_scale = dsc; P.mod_shift = dsh; P.mod_stride = Cp; }
  if (mask_cb8) { P.drop_mask = (const float*)mask_cb8; P.drop_ns = x.nstride; P.drop_scale = drop_scale; }
  if (rng) P.drop_scale = drop_scale;
  prep_out(P, y);
  hipStream_t st = (hipStream_t)stream;
  return finish(st, rng ? launch_prep_drop(P, *rng, st) : launch_prep(P, st), "prep (training forward)");
}

extern "C" int tm_op_prep_train(const void* x_cb8, const void* norm_w_host, const void* scale_host, const void* shift_host,
                                const void* mask_cb8, float drop_scale, int per_image, void* y_cb8, int N, int C, int Z, int S,
                                void* stream) {
  return prep_train_impl(x_cb8, norm_w_host, scale_host, shift_host, mask_cb8, drop_scale, nullptr, per_image, y_cb8, N, C, Z, S, stream);
}

extern "C" int tm_op_prep_train_rng(const void* x_cb8, const void* norm_w_host, const void* scale_host, const void* shift_host,
                                    unsigned long long key, unsigned site, float p, int per_image, void* y_cb8, int N, int C, int Z,
                                    int S, void* stream) {
  DropRng r;
  float ds = 1.f;
  if (!drop_rng_of(key, site, p, r, ds)) return fail(TM_ERR_ARG, "dropout p must lie in [0, 1)");
  return prep_train_impl(x_cb8, norm_w_host, scale_host, shift_host, nullptr, p > 0.f ? ds : 1.0f, p > 0.f ? &r : nullptr, per_image,
                         y_cb8, N, C, Z, S, stream);
}

static int prep_bwd_impl(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_host,
                         const void* shift_host, const void* mask_cb8, float drop_scale, const DropRng* rng, int per_image, void* dx_cb8,
                         void* dw_host, void* dscale_host, void* dshift_host, int N, int C, int Z, int S, void* stream) {
  if (!x_cb8 || !g_cb8 || !norm_w_host || !dx_cb8 || !dw_host || per_image < 1) return fail(TM_ERR_ARG, "bad argument");
  if (scale_host && (!shift_host || !dscale_host || !dshift_host)) return fail(TM_ERR_ARG, "scale without shift / gradient outputs");
  const int Cb = (C + 7) / 8, Cp = Cb * 8, nimg = (N + per_image - 1) / per_image;
  DevTmp tmp;
  const float* dwt = upload_rows(tmp, norm_w_host, 1, C, Cp);
  float* ddw = tmp.zeros(Cp);
  const float *dsc = nullptr, *dsh = nullptr;
  float *ddsc = nullptr, *ddsh = nullptr;
  if (scale_host) {
    dsc = upload_rows(tmp, scale_host, nimg, C, Cp); dsh = upload_rows(tmp, shift_host, nimg, C, Cp);
    ddsc = tmp.zeros((size_t)(nimg + 1) * Cp); ddsh = tmp.zeros((size_t)(nimg + 1) * Cp);
  }
  float* scratch = tmp.zeros(prep_bwd_scratch_floats(N, Cb, Z, S, scale_host != nullptr));
  if (tmp.err) return tmp.report();
  TV x = cb8_view(const_cast<void*>(x_cb8), N, C, Z, S, S);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_prep_bwd(x.p, x.nstride, (const float*)g_cb8, x.nstride, (const float*)mask_cb8, x.nstride, drop_scale, dwt,
                                 dsc, dsh, Cp, per_image, (float*)dx_cb8, x.nstride, ddw, ddsc, ddsh, N, Cb, C, Z, S, scratch, st, rng);
  if (int rc = finish(st, e, "prep backward")) return rc;
  HIP_TRY(download_rows(dw_host, ddw, 1, C, Cp));
  if (scale_host) {
    HIP_TRY(download_rows(dscale_host, ddsc, nimg, C, Cp));
    HIP_TRY(download_rows(dshift_host, ddsh, nimg, C, Cp));
  }
  return TM_OK;
}

extern "C" int tm_op_prep_bwd(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_host,
                              const void* shift_host, const void* mask_cb8, float drop_scale, int per_image, void* dx_cb8,
                              void* dw_host, void* dscale_host, void* dshift_host, int N, int C, int Z, int S, void* stream) {
  return prep_bwd_impl(x_cb8, g_cb8, norm_w_host, scale_host, shift_host, mask_cb8, drop_scale, nullptr, per_image, dx_cb8, dw_host,
                       dscale_host, dshift_host, N, C, Z, S, stream);
}

extern "C" int tm_op_prep_bwd_rng(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_host,
                                  const void* shift_host, unsigned long long key, unsigned site, float p, int per_image, void* dx_cb8,
                                  void* dw_host, void* dscale_host, void* dshift_host, int N, int C, int Z, int S, void* stream) {
  DropRng r;
  float ds = 1.f;
  if (!drop_rng_of(key, site, p, r, ds)) return fail(TM_ERR_ARG, "dropout p must lie in [0, 1)");
  return prep_bwd_impl(x_cb8, g_cb8, norm_w_host, scale_host, shift_host, nullptr, p > 0.f ? ds : 1.0f, p > 0.f ? &r : nullptr, per_image,
                       dx_cb8, dw_host, dscale_host, dshift_host, N, C, Z, S, stream);
}

extern "C" int tm_op_dropout_mask(unsigned long long key, unsigned site, float p, void* mask_cb8, int N, int C, int Z, int S,
                                  void* stream) {
  DropRng r;
  float ds = 1.f;
  if (!mask_cb8 || N < 0 || C < 1 || Z < 1 || S < 1) return fail(TM_ERR_ARG, "bad argument");
  if (!drop_rng_of(key, site, p, r, ds)) return fail(TM_ERR_ARG, "dropout p must lie in [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_dropout_mask((float*)mask_cb8, N, C, Z, S, r.key, r.site, r.thr, st), "dropout mask");
}

// ---- AttnBlock training pieces (teramind_amd.training.AttnBlockTrain composes them) ----
extern "C" int tm_op_ew(int op, const void* a, const void* b, const void* c, void* o1, void* o2, long n, void* stream) {
  if (op < 0 || op > 8 || !a || !o1 || n < 0) return fail(TM_ERR_ARG, "bad argument");
  if ((op == 0 || op == 1) && (!b || !c)) return fail(TM_ERR_ARG, "op %d needs b and c", op);
  if ((op == 3 || op == 5 || op == 6) && !b) return fail(TM_ERR_ARG, "op %d needs b", op);
  if (op == 1 && !o2) return fail(TM_ERR_ARG, "op 1 needs two outputs");
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_ew(op, (const float*)a, (const float*)b, (const float*)c, (float*)o1, (float*)o2, n, st), "elementwise op");
}

extern "C" int tm_op_modnorm(const void* x_cb8, const void* norm_w_host, const void* scale_cb8, const void* shift_cb8, void* y_cb8, int N,
                             int C, int Z, int S, void* stream) {
  if (!x_cb8 || !norm_w_host || !scale_cb8 || !shift_cb8 || !y_cb8) return fail(TM_ERR_ARG, "bad argument");
  const int Cb = (C + 7) / 8, Cp = Cb * 8;
  DevTmp tmp;
  const float* dw = upload_rows(tmp, norm_w_host, 1, C, Cp);
  if (tmp.err) return tmp.report();
  TV x = cb8_view(const_cast<void*>(x_cb8), N, C, Z, S, S), y = cb8_view(y_cb8, N, C, Z, S, S);
  PrepLaunch P = prep_start(N, Z, S);
  prep_src(P, x);
  prep_norm(P, dw, C);
  prep_mod_voxel(P, cb8_view(const_cast<void*>(scale_cb8), N, C, Z, S, S), cb8_view(const_cast<void*>(shift_cb8), N, C, Z, S, S), false);
  prep_out(P, y);
  return finish((hipStream_t)stream, launch_prep(P, (hipStream_t)stream), "modulate(norm)");
}

extern "C" int tm_op_modnorm_bwd(const void* x_cb8, const void* g_cb8, const void* norm_w_host, const void* scale_cb8, void* dx_cb8,
                                 void* dscale_cb8, void* dshift_cb8, void* dw_host, int N, int C, int Z, int S, void* stream) {
  if (!x_cb8 || !g_cb8 || !norm_w_host || !scale_cb8 || !dx_cb8 || !dscale_cb8 || !dshift_cb8 || !dw_host)
    return fail(TM_ERR_ARG, "bad argument");
  const int Cb = (C + 7) / 8, Cp = Cb * 8;
  DevTmp tmp;
  const float* dwt = upload_rows(tmp, norm_w_host, 1, C, Cp);
  float* ddw = tmp.zeros(Cp);
  const long vox = (long)N * Z * S * S;
  float* scratch = tmp.zeros((size_t)((vox + 63) / 64) * Cp);
  if (tmp.err) return tmp.report();
  TV x = cb8_view(const_cast<void*>(x_cb8), N, C, Z, S, S);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_modnorm_bwd(x, (const float*)g_cb8, dwt, (const float*)scale_cb8, (float*)dx_cb8, (float*)dscale_cb8,
                                    (float*)dshift_cb8, ddw, C, scratch, st);
  if (int rc = finish(st, e, "modulate(norm) backward")) return rc;
  HIP_TRY(download_rows(dw_host, ddw, 1, C, Cp));
  return TM_OK;
}

extern "C" int tm_op_window_attn_train(const void* q_cb8, const void* k_cb8, const void* v_cb8, const void* qw_host, const void* kw_host,
                                       const void* dout_cb8, void* o_cb8, void* dq_cb8, void* dk_cb8, void* dv_cb8, void* dqw_host,
                                       void* dkw_host, int N, int C, int Z, int S, void* stream) {
  const bool bwd = dout_cb8 != nullptr;
  if (!q_cb8 || !k_cb8 || !v_cb8 || !qw_host || !kw_host) return fail(TM_ERR_ARG, "bad argument");
  if (bwd ? (!dq_cb8 || !dk_cb8 || !dv_cb8 || !dqw_host || !dkw_host) : !o_cb8) return fail(TM_ERR_ARG, "missing output");
  const int T = Z * (S / 2) * (S / 2);
  const bool lng = T == 256 || T == 512, shrt = T == 4 || T == 8 || T == 16;
  if ((S & 1) || (T != 32 && T != 64 && T != 128 && !lng && !shrt) || C > 512 || C < 1)
    return fail(TM_ERR_ARG, "window of %d tokens / C = %d: the training attention core takes 4, 8, 16, 32, 64, 128, 256 or 512 tokens and "
                "C <= 512", T, C);
  if (lng && C > 256)
    return fail(TM_ERR_ARG, "window of %d tokens / C = %d: the long-window core holds a token's output in eight 32-channel accumulator "
                "tiles, C <= 256", T, C);
  const int Cb = (C + 7) / 8, Cp = Cb * 8;
  DevTmp tmp;
  const float *dqw_in = upload_rows(tmp, qw_host, 1, C, Cp), *dkw_in = upload_rows(tmp, kw_host, 1, C, Cp);
  float *gq = bwd ? tmp.zeros(Cp) : nullptr, *gk = bwd ? tmp.zeros(Cp) : nullptr;
  float* scratch = lng ? tmp.alloc<float>(attn_train_long_scratch_floats(N, Cb, Z, S, bwd)) : bwd ? tmp.zeros((size_t)2 * N * 4 * Cp) : nullptr;
  if (tmp.err) return tmp.report();
  TV q = cb8_view(const_cast<void*>(q_cb8), N, C, Z, S, S), k = cb8_view(const_cast<void*>(k_cb8), N, C, Z, S, S),
     v = cb8_view(const_cast<void*>(v_cb8), N, C, Z, S, S);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = (lng ? launch_attn_train_long : shrt ? launch_attn_train_short : launch_attn_train)(q, k, v, dqw_in, dkw_in, (const float*)dout_cb8, (float*)o_cb8,
                                                                    (float*)dq_cb8, (float*)dk_cb8, (float*)dv_cb8, gq, gk, scratch, bwd, st);
  if (int rc = finish(st, e, "window attention (training)")) return rc;
  if (bwd) {
    HIP_TRY(download_rows(dqw_host, gq, 1, C, Cp));
    HIP_TRY(download_rows(dkw_host, gk, 1, C, Cp));
  }
  return TM_OK;
}

extern "C" int tm_op_gemm_f32(const void* A_dev, const void* B_dev, const void* bias_dev, void* C_dev, int M, int N, int K,
                              const long* strides9_host, int batch, int bias_mode, int accumulate, float alpha, void* stream) {
  if (!A_dev || !B_dev || !C_dev || !strides9_host || M < 1 || N < 1 || K < 1 || batch < 1 || bias_mode < 0 || bias_mode > 2 ||
      (bias_mode && !bias_dev))
    return fail(TM_ERR_ARG, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_gemm_f32((const float*)A_dev, (const float*)B_dev, (const float*)bias_dev, (float*)C_dev, M, N, K, strides9_host,
                                    batch, bias_mode, accumulate, alpha, st), "gemm");
}

extern "C" int tm_op_rows(int op, const void* x_dev, const void* w_dev, const void* g_dev, void* y_dev, void* dw_dev, long rows, int D,
                          void* stream) {
  if (op < 0 || op > 3 || !x_dev || !y_dev || rows < 1 || D < 1 || D > 8192) return fail(TM_ERR_ARG, "bad argument");
  if (op == 1 && D > 4096) return fail(TM_ERR_ARG, "op 1: D = %d > 4096 (its workgroup keeps 4 * D floats of dynamic LDS, 64 KiB at most)", D);
  if ((op <= 1 && !w_dev) || ((op == 1 || op == 3) && !g_dev) || (op == 1 && !dw_dev)) return fail(TM_ERR_ARG, "op %d: missing operand", op);
  DevTmp tmp;
  float* scratch = op == 1 ? tmp.zeros((size_t)((rows + 3) / 4) * D) : nullptr;
  if (tmp.err) return tmp.report();
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_rows(op, (const float*)x_dev, (const float*)w_dev, (const float*)g_dev, (float*)y_dev, (float*)dw_dev, scratch,
                                rows, D, st), "row op");
}

extern "C" int tm_op_resample(const void* x_cb8, void* y_cb8, int N, int C, int Z, int S_out, int mode, void* stream) {
  if (!x_cb8 || !y_cb8 || (mode != 1 && mode != 2) || (mode == 1 && (S_out & 1))) return fail(TM_ERR_ARG, "bad argument");
  const int S_in = mode == 1 ? S_out / 2 : S_out * 2;
  TV x = cb8_view(const_cast<void*>(x_cb8), N, C, Z, S_in, S_in), y = cb8_view(y_cb8, N, C, Z, S_out, S_out);
  PrepLaunch P = prep_start(N, Z, S_out);
  prep_src(P, x);
  P.resample = mode == 1 ? RS_UP2 : RS_DOWN2;
  prep_out(P, y);
  return finish((hipStream_t)stream, launch_prep(P, (hipStream_t)stream), "resample");
}

extern "C" int tm_op_sumsq(const void* x_dev, long n, float* out_host, void* stream) {
  if (!x_dev || n < 1 || !out_host) return fail(TM_ERR_ARG, "bad argument");
  const int nwg = (int)std::min<long>(1024, (n + 255) / 256);
  DevTmp tmp;
  float* scratch = tmp.zeros((size_t)nwg + 8);
  if (tmp.err) return tmp.report();
  hipStream_t st = (hipStream_t)stream;
  if (int rc = finish(st, launch_sumsq((const float*)x_dev, n, scratch + nwg, scratch, nwg, st), "sum of squares")) return rc;
  HIP_TRY(hipMemcpy(out_host, scratch + nwg, sizeof(float), hipMemcpyDeviceToHost));
  return TM_OK;
}

extern "C" int tm_op_adam(void* p_dev, const void* g_dev, void* m_dev, void* v_dev, long n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int step, float grad_scale, void* stream) {
  if (!p_dev || !g_dev || !m_dev || !v_dev || n < 1 || step < 1) return fail(TM_ERR_ARG, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  return finish(st, launch_adam((float*)p_dev, (const float*)g_dev, (float*)m_dev, (float*)v_dev, n, lr, beta1, beta2, eps, weight_decay,
                                step, grad_scale, st), "adam");
}

// Rank-ordered sum of W gradient slices (train_dist.GradExchange): queued on `stream`, no synchronisation, no scratch
static int rank_sum_args(int W, long n) {
  if (W < 1 || W > 64) return fail(TM_ERR_ARG, "rank sum: W = %d, must be 1 .. 64", W);
  if (n < 0) return fail(TM_ERR_ARG, "rank sum: n = %ld, must be >= 0", n);
  if ((unsigned long)n > (1UL << 60) / 64) return fail(TM_ERR_ARG, "rank sum: n = %ld is too large", n);
  return TM_OK;
}
extern "C" int tm_op_rank_sum(const void* parts_dev, void* out_dev, int W, long n, void* stream) {
  if (!parts_dev || !out_dev) return fail(TM_ERR_ARG, "rank sum: null pointer");
  if (int rc = rank_sum_args(W, n)) return rc;
  if (n == 0) return TM_OK;
  const uintptr_t p0 = (uintptr_t)parts_dev, p1 = p0 + (uintptr_t)W * (uintptr_t)n * sizeof(float);
  const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)n * sizeof(float);
  if (o0 < p1 && p0 < o1) return fail(TM_ERR_ARG, "rank sum: out overlaps parts (every slice is read after out may have been written)");
  if ((p0 | o0) & 3) return fail(TM_ERR_ARG, "rank sum: pointers must be 4-byte aligned");
  HIP_TRY(launch_rank_sum((const float*)parts_dev, (float*)out_dev, W, n, (hipStream_t)stream));
  return TM_OK;
}

// dX of Conv3d(k = 3x3x3 pad 1 | 1x1x1), stride 1: the forward MFMA conv of dY with the kernel flipped in z, y, x and
// cin <-> cout transposed (w_host [Cout][Cin][taps] as in the reference state_dict)
extern "C" int tm_op_conv_dgrad(const void* dy_cb8, const void* w_host, void* dx_cb8, int N, int Cin, int Cout, int Z, int S,
                                int ksize, void* stream) {
  if (!dy_cb8 || !w_host || !dx_cb8 || (ksize != 1 && ksize != 3)) return fail(TM_ERR_ARG, "bad argument");
  const int taps = ksize == 1 ? 1 : 27;
  const float* w = (const float*)w_host;
  std::vector<float> wt((size_t)Cin * Cout * taps);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < taps; ++t) wt[((size_t)ci * Cout + co) * taps + (taps - 1 - t)] = w[((size_t)co * Cin + ci) * taps + t];
  std::vector<float> zb(Cin, 0.f);
  return tm_op_conv_mfma(dy_cb8, wt.data(), zb.data(), dx_cb8, N, Cout, Cin, Z, S, ksize, ZM_PAD1, 0, 0, stream);
}

// dW [Cout][Cin][taps] and db [Cout] (HOST outputs) of the same convs from the forward input x and dY
extern "C" int tm_op_conv_wgrad(const void* x_cb8, const void* dy_cb8, void* dw_host, void* db_host_or_null, int N, int Cin,
                                int Cout, int Z, int S, int ksize, void* stream) {
  if (!x_cb8 || !dy_cb8 || !dw_host || (ksize != 1 && ksize != 3)) return fail(TM_ERR_ARG, "bad argument");
  if (Z < 1 || Z > 4) return fail(TM_ERR_ARG, "weight gradient: Z must be 1 .. 4 (the kernel stages up to four z planes)");
  const int taps = ksize == 1 ? 1 : 27;
  hipStream_t st = (hipStream_t)stream;
  TV x = cb8_view(const_cast<void*>(x_cb8), N, Cin, Z, S, S), dy = cb8_view(const_cast<void*>(dy_cb8), N, Cout, Z, S, S);
  DevTmp tmp;
  const size_t nw = (size_t)Cout * Cin * taps;
  float* ddw = tmp.zeros(nw);
  float* ddb = tmp.zeros((size_t)dy.Cb * 8);
  if (tmp.err) return tmp.report();
  hipError_t e = launch_conv_wgrad(x, dy, ddw, Cin, Cout, taps, st);
  if (e == hipSuccess && db_host_or_null) e = launch_chan_sum(dy, ddb, Cout, st);
  if (int rc = finish(st, e, "conv wgrad")) return rc;
  HIP_TRY(hipMemcpy(dw_host, ddw, nw * sizeof(float), hipMemcpyDeviceToHost));
  if (db_host_or_null) HIP_TRY(hipMemcpy(db_host_or_null, ddb, Cout * sizeof(float), hipMemcpyDeviceToHost));
  return TM_OK;
}

// ------------------------------------------------------------------------------------------
// resident conv ops of the training tape: weights packed on the device, gradients to device pointers.  None of them
// synchronises `stream` or touches host memory; their scratch is stream-ordered (DevTmp(stream)).
// ------------------------------------------------------------------------------------------
static int packed_form(int Cout, int Cin, int ksize, int Z, int role) {
  if (ksize != 1 && ksize != 3) return fail(TM_ERR_ARG, "ksize must be 1 or 3");
  if (Cout < 1 || Cin < 1 || Z < 1) return fail(TM_ERR_ARG, "Cout, Cin and Z must be positive");
  if (role != 0 && role != 1) return fail(TM_ERR_ARG, "role must be 0 (forward) or 1 (data gradient)");
  return TM_OK;
}
extern "C" long tm_conv_pack_floats(int Cout, int Cin, int ksize, int Z, int role) {
  if (packed_form(Cout, Cin, ksize, Z, role)) return -1;
  const int form = conv_pick_form(ksize, ZM_PAD1, Z, false, ROLE_OP);
  return (long)(role ? conv_pack_floats(form, Cin, (Cout + 7) / 8) : conv_pack_floats(form, Cout, (Cin + 7) / 8));
}
extern "C" int tm_op_conv_pack_dev(const void* w_dev, void* pack_dev, int Cout, int Cin, int ksize, int Z, int role, void* stream) {
  if (!w_dev || !pack_dev) return fail(TM_ERR_ARG, "null argument");
  if (int rc = packed_form(Cout, Cin, ksize, Z, role)) return rc;
  const int form = conv_pick_form(ksize, ZM_PAD1, Z, false, ROLE_OP);                   // of the conv that reads the pack
  HIP_TRY(launch_conv_pack((const float*)w_dev, (float*)pack_dev, Cout, Cin, form, role, (hipStream_t)stream));
  return TM_OK;
}
// y = conv(x) on a ready pack of Cout x Cin; bias_dev [Cout] or null (zero)
static int conv_packed(const void* x_cb8, const void* pack_dev, const void* bias_dev, void* y_cb8, int N, int Cin, int Cout, int Z, int S,
                       int ksize, hipStream_t st) {
  DevTmp tmp(st);
  ConvW cw = conv_w(conv_pick_form(ksize, ZM_PAD1, Z, false, ROLE_OP), Cout, (Cin + 7) / 8);
  float* b = tmp.ordered_floats((size_t)cw.ntile * 64, true);       // the epilogues read the bias zero padded to 64 couts
  if (tmp.err) return tmp.report();
  if (bias_dev) HIP_TRY(hipMemcpyAsync(b, bias_dev, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
  cw.w = (const float*)pack_dev; cw.bias = b;
  ConvLaunch L;
  L.x = cb8_view(const_cast<void*>(x_cb8), N, Cin, Z, S, S);
  L.w = cw;
  L.y = cb8_view(y_cb8, N, Cout, Z, S, S);
  L.zmode = ZM_PAD1;
  HIP_TRY(launch_conv_mfma(L, st));
  return TM_OK;
}
static int resident_geo(int N, int Cin, int Cout, int Z, int S, int ksize) {
  if (ksize != 1 && ksize != 3) return fail(TM_ERR_ARG, "ksize must be 1 or 3");
  if (N < 1 || Cin < 1 || Cout < 1 || S < 1) return fail(TM_ERR_ARG, "N, Cin, Cout and S must be positive");
  if (Z < 1 || (Z > 4 && Z != 8)) return fail(TM_ERR_ARG, "Z must be 1 .. 4 or 8 (got %d)", Z);
  return TM_OK;
}
extern "C" int tm_op_conv_mfma_packed(const void* x_cb8, const void* pack_dev, const void* bias_dev, void* y_cb8, int N, int Cin, int Cout,
                                      int Z, int S, int ksize, void* stream) {
  if (!x_cb8 || !pack_dev || !bias_dev || !y_cb8) return fail(TM_ERR_ARG, "null argument");
  if (int rc = resident_geo(N, Cin, Cout, Z, S, ksize)) return rc;
  return conv_packed(x_cb8, pack_dev, bias_dev, y_cb8, N, Cin, Cout, Z, S, ksize, (hipStream_t)stream);
}
extern "C" int tm_op_conv_dgrad_packed(const void* dy_cb8, const void* pack_dev, void* dx_cb8, int N, int Cin, int Cout, int Z, int S,
                                       int ksize, void* stream) {
  if (!dy_cb8 || !pack_dev || !dx_cb8) return fail(TM_ERR_ARG, "null argument");
  if (int rc = resident_geo(N, Cin, Cout, Z, S, ksize)) return rc;
  return conv_packed(dy_cb8, pack_dev, nullptr, dx_cb8, N, Cout, Cin, Z, S, ksize, (hipStream_t)stream);
}
extern "C" int tm_op_conv_wgrad_dev(const void* x_cb8, const void* dy_cb8, void* dw_dev, void* db_dev_or_null, int accumulate, int N,
                                    int Cin, int Cout, int Z, int S, int ksize, void* stream) {
  if (!x_cb8 || !dy_cb8 || !dw_dev) return fail(TM_ERR_ARG, "null argument");
  if (int rc = resident_geo(N, Cin, Cout, Z, S, ksize)) return rc;
  if (accumulate != 0 && accumulate != 1) return fail(TM_ERR_ARG, "accumulate must be 0 or 1");
  const int taps = ksize == 1 ? 1 : 27;
  hipStream_t st = (hipStream_t)stream;
  TV x = cb8_view(const_cast<void*>(x_cb8), N, Cin, Z, S, S), dy = cb8_view(const_cast<void*>(dy_cb8), N, Cout, Z, S, S);
  DevTmp tmp(st);
  const size_t ns = conv_wgrad_scratch_floats(N, Z, S, Cin, Cout, taps);
  float* scratch = ns ? tmp.ordered_floats(ns, false) : nullptr;
  if (tmp.err) return tmp.report();
  HIP_TRY(launch_conv_wgrad_mfma(x, dy, (float*)dw_dev, Cin, Cout, taps, accumulate, scratch, st));
  if (db_dev_or_null) HIP_TRY(launch_chan_sum(dy, (float*)db_dev_or_null, Cout, st, accumulate));
  return TM_OK;
}

// Baseline-JPEG tile scans of a resident uint8 plane (tm_export.hip); enqueues only, the bit buffers are stream-ordered scratch
extern "C" int tm_jpeg_encode_tiles(const void* plane, int H, int W, int64_t pitch, int quality, int tile0, int ntiles, void* slots,
                                    int64_t slot_bytes, int32_t* need, void* packed, int64_t* offsets, void* stream) {
  const char* fn = "tm_jpeg_encode_tiles";
  if (!plane || !slots || !need) return fail(TM_ERR_ARG, "%s: null plane / slots / need pointer", fn);
  if (!packed != !offsets) return fail(TM_ERR_ARG, "%s: packed and offsets go together (both or neither)", fn);
  if (H < 1 || W < 1) return fail(TM_ERR_ARG, "%s: H and W must be positive, got %d x %d", fn, H, W);
  if (pitch < W) return fail(TM_ERR_ARG, "%s: pitch %lld below W %d", fn, (long long)pitch, W);
  if (quality < 1 || quality > 100) return fail(TM_ERR_ARG, "%s: quality %d outside 1 .. 100", fn, quality);
  const long grid = (long)((H + 255) / 256) * ((W + 255) / 256);
  if (tile0 < 0 || ntiles < 1 || (long)tile0 + ntiles > grid)
    return fail(TM_ERR_ARG, "%s: tiles [%d, %d + %d) outside the grid of %ld", fn, tile0, tile0, ntiles, grid);
  if (slot_bytes < 1) return fail(TM_ERR_ARG, "%s: slot_bytes must be positive", fn);
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp(st);
  uint32_t* scratch = (uint32_t*)tmp.ordered_floats(jpeg_scratch_bytes(ntiles) / sizeof(float), false);
  if (tmp.err) return tmp.report();
  HIP_TRY(launch_jpeg_tiles((const uint8_t*)plane, H, W, (long)pitch, quality, tile0, ntiles, scratch, (uint8_t*)slots, (long)slot_bytes,
                            need, (uint8_t*)packed, offsets, st));
  return TM_OK;
}

// The colour composite (tm_export.hip): the checks of the source that tm_rgb_compose and tm_jpeg_encode_tiles_rgb share
static int rgb_source(const char* fn, const void* const* planes, const int64_t* pitches, int H, int W, float bright, const void* overlay,
                      int oh, int ow, int alpha, RgbSrc* src) {
  if (!planes || !pitches) return fail(TM_ERR_ARG, "%s: null planes / pitches array", fn);
  if (!planes[0] && !planes[1] && !planes[2]) return fail(TM_ERR_ARG, "%s: all three planes are null", fn);
  if (H < 1 || W < 1) return fail(TM_ERR_ARG, "%s: H and W must be positive, got %d x %d", fn, H, W);
  for (int c = 0; c < 3; ++c)
    if (planes[c] && pitches[c] < W) return fail(TM_ERR_ARG, "%s: pitch %lld of plane %d below W %d", fn, (long long)pitches[c], c, W);
  if (!(bright >= 0.f) || bright > 3.0e38f) return fail(TM_ERR_ARG, "%s: bright must be finite and not negative, got %g", fn, (double)bright);
  if (overlay) {
    if (oh < 1 || ow < 1) return fail(TM_ERR_ARG, "%s: overlay size must be positive, got %d x %d", fn, oh, ow);
    if (alpha < 0 || alpha > 255) return fail(TM_ERR_ARG, "%s: alpha %d outside 0 .. 255", fn, alpha);
    if ((long)H * oh >= (1L << 31) || (long)W * ow >= (1L << 31))
      return fail(TM_ERR_ARG, "%s: overlay %d x %d on a %d x %d level: H oh and W ow must stay below 2^31", fn, oh, ow, H, W);
  }
  for (int c = 0; c < 3; ++c) {
    src->p[c] = (const uint8_t*)planes[c];
    src->pitch[c] = planes[c] ? (long)pitches[c] : 0;
  }
  src->H = H;
  src->W = W;
  src->bright = bright;
  src->ov = (const uint8_t*)overlay;
  src->oh = overlay ? oh : 0;
  src->ow = overlay ? ow : 0;
  src->alpha = overlay ? alpha : 0;
  return TM_OK;
}
extern "C" int tm_rgb_compose(const void* const* planes, const int64_t* pitches, int H, int W, float bright, const void* overlay, int oh,
                              int ow, int alpha, void* dst, int64_t dst_pitch, void* stream) {
  const char* fn = "tm_rgb_compose";
  RgbSrc src;
  if (int rc = rgb_source(fn, planes, pitches, H, W, bright, overlay, oh, ow, alpha, &src)) return rc;
  if (!dst) return fail(TM_ERR_ARG, "%s: null destination", fn);
  if (dst_pitch < 3 * (int64_t)W) return fail(TM_ERR_ARG, "%s: destination pitch %lld below 3 W = %lld", fn, (long long)dst_pitch, 3LL * W);
  HIP_TRY(launch_rgb_compose(src, (uint8_t*)dst, (long)dst_pitch, (hipStream_t)stream));
  return TM_OK;
}
extern "C" int tm_jpeg_encode_tiles_rgb(const void* const* planes, const int64_t* pitches, int H, int W, float bright, const void* overlay,
                                        int oh, int ow, int alpha, int quality, int tile0, int ntiles, void* slots, int64_t slot_bytes,
                                        int32_t* need, void* packed, int64_t* offsets, void* stream) {
  const char* fn = "tm_jpeg_encode_tiles_rgb";
  RgbSrc src;
  if (int rc = rgb_source(fn, planes, pitches, H, W, bright, overlay, oh, ow, alpha, &src)) return rc;
  if (!slots || !need) return fail(TM_ERR_ARG, "%s: null slots / need pointer", fn);
  if (!packed != !offsets) return fail(TM_ERR_ARG, "%s: packed and offsets go together (both or neither)", fn);
  if (quality < 1 || quality > 100) return fail(TM_ERR_ARG, "%s: quality %d outside 1 .. 100", fn, quality);
  const long grid = (long)((H + 255) / 256) * ((W + 255) / 256);
  if (tile0 < 0 || ntiles < 1 || (long)tile0 + ntiles > grid)
    return fail(TM_ERR_ARG, "%s: tiles [%d, %d + %d) outside the grid of %ld", fn, tile0, tile0, ntiles, grid);
  if (slot_bytes < 1) return fail(TM_ERR_ARG, "%s: slot_bytes must be positive", fn);
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp(st);
  uint32_t* scratch = (uint32_t*)tmp.ordered_floats(jpeg_rgb_scratch_bytes(ntiles) / sizeof(float), false);
  if (tmp.err) return tmp.report();
  HIP_TRY(launch_jpeg_tiles_rgb(src, quality, tile0, ntiles, scratch, (uint8_t*)slots, (long)slot_bytes, need, (uint8_t*)packed, offsets, st));
  return TM_OK;
}

// Blosc-lz4 frames (tm_blosc.hip); enqueue only, the stream slots and length tables are stream-ordered scratch
static int blosc_args(const char* fn, size_t nbytes, int typesize, int blocksize, BloscGeo* g) {
  if (nbytes < 1) return fail(TM_ERR_ARG, "%s: nothing to compress (nbytes = 0)", fn);
  if (typesize != 1 && typesize != 2 && typesize != 4) return fail(TM_ERR_ARG, "%s: typesize %d is not 1, 2 or 4", fn, typesize);
  if (blocksize < BLOSC_ENC_MIN_BLOCK || blocksize > BLOSC_ENC_MAX_BLOCK || (blocksize & 3))
    return fail(TM_ERR_ARG, "%s: blocksize %d is not a multiple of 4 in [%d, %d]", fn, blocksize, BLOSC_ENC_MIN_BLOCK, BLOSC_ENC_MAX_BLOCK);
  if (!blosc_geometry(nbytes, typesize, blocksize, g))
    return fail(TM_ERR_ARG, "%s: %zu bytes do not fit a Blosc-1 frame (2^31 - 1 bytes with its tables)", fn, nbytes);
  return TM_OK;
}
extern "C" size_t tm_blosc_bound(size_t nbytes, int typesize, int blocksize) {
  BloscGeo g;
  return blosc_args("tm_blosc_bound", nbytes, typesize, blocksize, &g) ? 0 : g.bound;
}
static int blosc_run(const BloscSrc& src, const BloscGeo& g, int nframes, void* packed, int64_t* offsets, int64_t* total, hipStream_t st) {
  DevTmp tmp(st);
  void* scratch = tmp.ordered_floats((blosc_scratch_bytes(g, nframes) + 3) / 4, false);
  if (tmp.err) return tmp.report();
  HIP_TRY(launch_blosc_frames(src, g, nframes, scratch, (uint8_t*)packed, offsets, total, st));
  return TM_OK;
}
extern "C" int tm_blosc_compress(const void* src, size_t nbytes, int typesize, int blocksize, void* frame, size_t frame_cap,
                                 int64_t* out_bytes, void* stream) {
  const char* fn = "tm_blosc_compress";
  if (!src || !frame || !out_bytes) return fail(TM_ERR_ARG, "%s: null source / frame / out_bytes pointer", fn);
  BloscGeo g;
  if (int rc = blosc_args(fn, nbytes, typesize, blocksize, &g)) return rc;
  if (frame_cap < g.bound) return fail(TM_ERR_ARG, "%s: frame buffer of %zu bytes below the bound %zu (tm_blosc_bound)", fn, frame_cap, g.bound);
  BloscSrc s = {};
  s.base = (const uint8_t*)src; s.mode = BLOSC_SRC_BYTES;
  return blosc_run(s, g, 1, frame, nullptr, out_bytes, (hipStream_t)stream);
}
extern "C" int tm_blosc_compress_tiles(const void* canvas, int dtype, int64_t canvas_elems, int C, int TH, int TW, int64_t chan_stride,
                                       int64_t pitch, const int64_t* origins, const int64_t* origins_host, int ntiles, void* packed,
                                       int64_t packed_cap, int64_t* offsets, void* stream) {
  const char* fn = "tm_blosc_compress_tiles";
  if (!canvas || !origins || !origins_host || !packed || !offsets)
    return fail(TM_ERR_ARG, "%s: null canvas / origins (device array and its host mirror) / packed / offsets pointer", fn);
  if (dtype != TM_DTYPE_F32 && dtype != TM_DTYPE_F16) return fail(TM_ERR_ARG, "%s: dtype %d is neither TM_DTYPE_F32 nor TM_DTYPE_F16", fn, dtype);
  if ((uintptr_t)canvas & (dtype == TM_DTYPE_F32 ? 3 : 1)) return fail(TM_ERR_ARG, "%s: canvas pointer is not aligned to its element", fn);
  if (C < 1 || TH < 1 || TW < 1) return fail(TM_ERR_ARG, "%s: C, TH and TW must be positive, got %d x %d x %d", fn, C, TH, TW);
  if (ntiles < 1 || ntiles > 65535) return fail(TM_ERR_ARG, "%s: ntiles = %d outside 1 .. 65535", fn, ntiles);
  const int64_t elems = (int64_t)C * TH * TW;
  if (elems > (int64_t)1 << 29) return fail(TM_ERR_ARG, "%s: a tile of %lld elements is larger than 2^29", fn, (long long)elems);
  if (pitch < TW) return fail(TM_ERR_ARG, "%s: row pitch %lld below TW %d", fn, (long long)pitch, TW);
  const int64_t plane = (int64_t)(TH - 1) * pitch + TW;                 // elements from a channel's first to past its last
  if (chan_stride < plane) return fail(TM_ERR_ARG, "%s: channel stride %lld below the %lld elements a channel spans", fn, (long long)chan_stride, (long long)plane);
  const int64_t span = (int64_t)(C - 1) * chan_stride + plane;
  for (int k = 0; k < ntiles; ++k)
    if (origins_host[k] < 0 || origins_host[k] > canvas_elems - span)
      return fail(TM_ERR_ARG, "%s: tile %d at element %lld (+ %lld) leaves the canvas of %lld elements", fn, k, (long long)origins_host[k],
                  (long long)span, (long long)canvas_elems);
  BloscGeo g;
  if (int rc = blosc_args(fn, (size_t)elems * 2, 2, BLOSC_ENC_MAX_BLOCK, &g)) return rc;
  if (packed_cap < 0 || (size_t)packed_cap < (size_t)ntiles * g.bound)
    return fail(TM_ERR_ARG, "%s: packed buffer of %lld bytes below ntiles x bound = %d x %zu", fn, (long long)packed_cap, ntiles, g.bound);
  BloscSrc s = {};
  s.base = (const uint8_t*)canvas; s.mode = dtype == TM_DTYPE_F32 ? BLOSC_SRC_F32 : BLOSC_SRC_F16;
  s.TH = TH; s.TW = TW; s.cstride = (long)chan_stride; s.pitch = (long)pitch; s.origins = origins;
  return blosc_run(s, g, ntiles, packed, offsets, nullptr, (hipStream_t)stream);
}

// Blosc-lz4 decoder (tm_blosc.hip): the host walks the frames into a stream table (every range checked), then enqueues
extern "C" int tm_blosc_frame_info(const void* frame, size_t frame_bytes, tm_blosc_frame* out) {
  const char* fn = "tm_blosc_frame_info";
  if (!frame || !out) return fail(TM_ERR_ARG, "%s: null frame / out pointer", fn);
  BloscDecInfo in = {};
  const int rc = blosc_dec_walk(fn, 0, (const uint8_t*)frame, frame_bytes, &in, nullptr, 0, 0, nullptr);
  out->nbytes = in.nbytes; out->typesize = in.typesize; out->blocksize = in.blocksize; out->flags = in.flags;
  out->nstreams = rc == TM_OK && in.gpu ? in.nstreams : 0;
  out->longest = rc == TM_OK && in.gpu ? in.longest : 0;
  out->gpu = rc == TM_OK ? in.gpu : 0;
  return rc;
}
namespace {
struct BloscDecPlan {
  std::vector<BloscStream> tab;
  std::vector<BloscDecFrame> fr;
  size_t scratch = 0;
  int longest_lz4 = 0, max_nbytes = 0;
};
}  // namespace
// walks every frame of the host mirror; fr[k].dst and the canvas fields are left to the caller
static int blosc_dec_plan(const char* fn, const void* frames_host, const int64_t* frame_offsets, int nframes, BloscDecPlan* P) {
  if (!frames_host || !frame_offsets) return fail(TM_ERR_ARG, "%s: null host mirror of the frames / frame_offsets pointer", fn);
  if (nframes < 1 || nframes > 65535) return fail(TM_ERR_ARG, "%s: nframes = %d outside 1 .. 65535", fn, nframes);
  if (frame_offsets[0] < 0) return fail(TM_ERR_ARG, "%s: frame_offsets[0] is negative", fn);
  for (int k = 0; k < nframes; ++k)
    if (frame_offsets[k + 1] < frame_offsets[k]) return fail(TM_ERR_ARG, "%s: frame_offsets decrease at frame %d", fn, k);
  P->tab.clear(); P->fr.assign((size_t)nframes, BloscDecFrame{});
  for (int k = 0; k < nframes; ++k) {
    BloscDecInfo in = {};
    const uint8_t* f = (const uint8_t*)frames_host + frame_offsets[k];
    if (int rc = blosc_dec_walk(fn, k, f, (size_t)(frame_offsets[k + 1] - frame_offsets[k]), &in, &P->tab, frame_offsets[k], (long long)P->scratch,
                                &P->longest_lz4))
      return rc;
    if (!in.gpu)
      return fail(TM_ERR_ARG, "%s: frame %d is host only (flags 0x%02x, typesize %d, %lld bytes): bit shuffle, a codec other than lz4, a typesize "
                  "other than 1 / 2 / 4 or more than 2^30 bytes go through tm_blosc_decompress", fn, k, in.flags, in.typesize, in.nbytes);
    BloscDecFrame& d = P->fr[(size_t)k];
    const bool memcpyed = in.flags & 2;
    d.scratch = (long long)P->scratch; d.nbytes = (int)in.nbytes; d.typesize = in.typesize;
    d.blocksize = memcpyed || in.blocksize < 1 ? (in.nbytes > 0 ? (int)in.nbytes : 1) : in.blocksize;
    d.shuffled = !memcpyed && (in.flags & 1) && in.typesize > 1;
    if (d.nbytes > P->max_nbytes) P->max_nbytes = d.nbytes;
    P->scratch += ((size_t)in.nbytes + 15) & ~(size_t)15;
  }
  if (P->tab.size() > (size_t)INT32_MAX) return fail(TM_ERR_ARG, "%s: %zu streams in one call", fn, P->tab.size());
  return TM_OK;
}
static int blosc_dec_run(const char* fn, const void* frames, BloscDecPlan& P, const BloscSink& sink, int32_t* status, hipStream_t st) {
  DevTmp tmp(st);
  const size_t tab_b = (P.tab.size() * sizeof(BloscStream) + 15) & ~(size_t)15, fr_b = (P.fr.size() * sizeof(BloscDecFrame) + 15) & ~(size_t)15;
  uint8_t* dev = (uint8_t*)tmp.ordered_floats((P.scratch + tab_b + fr_b) / 4, false);   // the frames' images (16-byte multiples), the tables
  if (tmp.err) return tmp.report();
  uint8_t* tab_d = dev + P.scratch;
  uint8_t* fr_d = tab_d + tab_b;
  // pageable host memory: the runtime has taken the bytes when the call returns
  if (!P.tab.empty()) HIP_TRY(hipMemcpyAsync(tab_d, P.tab.data(), P.tab.size() * sizeof(BloscStream), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(fr_d, P.fr.data(), P.fr.size() * sizeof(BloscDecFrame), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_blosc_decode((const uint8_t*)frames, (const BloscStream*)tab_d, (int)P.tab.size(), P.longest_lz4, (const BloscDecFrame*)fr_d,
                              (int)P.fr.size(), P.max_nbytes, dev, sink, status, st));
  (void)fn;
  return TM_OK;
}
extern "C" int tm_blosc_decompress_dev(const void* frames, const void* frames_host, const int64_t* frame_offsets, int nframes, void* dst,
                                       int64_t dst_cap, const int64_t* dst_offsets, int32_t* status, void* stream) {
  const char* fn = "tm_blosc_decompress_dev";
  static thread_local BloscDecPlan P;
  P = BloscDecPlan();
  if (int rc = blosc_dec_plan(fn, frames_host, frame_offsets, nframes, &P)) return rc;
  if (!frames || !dst || !dst_offsets || !status) return fail(TM_ERR_ARG, "%s: null frames / dst / dst_offsets / status pointer", fn);
  for (int k = 0; k < nframes; ++k) {
    if (dst_offsets[k] < 0 || dst_offsets[k] > dst_cap - P.fr[(size_t)k].nbytes)
      return fail(TM_ERR_ARG, "%s: frame %d: %d bytes at offset %lld leave the destination of %lld bytes", fn, k, P.fr[(size_t)k].nbytes,
                  (long long)dst_offsets[k], (long long)dst_cap);
    P.fr[(size_t)k].dst = dst_offsets[k];
  }
  BloscSink sink = {};
  sink.base = dst; sink.mode = BLOSC_SINK_BYTES;
  return blosc_dec_run(fn, frames, P, sink, status, (hipStream_t)stream);
}
extern "C" int tm_blosc_decompress_tiles(const void* frames, const void* frames_host, const int64_t* frame_offsets, int nframes, void* canvas,
                                         int dtype, int64_t canvas_elems, int64_t chan_stride, int64_t pitch, const tm_blosc_box* boxes,
                                         int32_t* status, void* stream) {
  const char* fn = "tm_blosc_decompress_tiles";
  static thread_local BloscDecPlan P;
  P = BloscDecPlan();
  if (int rc = blosc_dec_plan(fn, frames_host, frame_offsets, nframes, &P)) return rc;
  if (!frames || !canvas || !boxes || !status) return fail(TM_ERR_ARG, "%s: null frames / canvas / boxes / status pointer", fn);
  if (dtype != TM_DTYPE_F32 && dtype != TM_DTYPE_F16) return fail(TM_ERR_ARG, "%s: dtype %d is neither TM_DTYPE_F32 nor TM_DTYPE_F16", fn, dtype);
  if ((uintptr_t)canvas & (dtype == TM_DTYPE_F32 ? 3 : 1)) return fail(TM_ERR_ARG, "%s: canvas pointer is not aligned to its element", fn);
  if (pitch < 1 || chan_stride < 1) return fail(TM_ERR_ARG, "%s: pitch and chan_stride must be positive", fn);
  for (int k = 0; k < nframes; ++k) {
    const tm_blosc_box& b = boxes[k];
    BloscDecFrame& d = P.fr[(size_t)k];
    int64_t elems = 1;
    for (int i = 0; i < 3; ++i) {
      if (b.chunk[i] < 1 || b.clip[i] < 1 || b.clip[i] > b.chunk[i])
        return fail(TM_ERR_ARG, "%s: frame %d: chunk %d x %d x %d, clip %d x %d x %d (1 <= clip <= chunk)", fn, k, b.chunk[0], b.chunk[1], b.chunk[2],
                    b.clip[0], b.clip[1], b.clip[2]);
      elems *= b.chunk[i];
      if (elems > (int64_t)1 << 29) return fail(TM_ERR_ARG, "%s: frame %d: a chunk of more than 2^29 elements", fn, k);
    }
    if (d.typesize != 2 || (int64_t)d.nbytes != 2 * elems)
      return fail(TM_ERR_ARG, "%s: frame %d holds %d bytes at typesize %d, not the %lld float16 of its chunk", fn, k, d.nbytes, d.typesize, (long long)elems);
    if (pitch < b.clip[2]) return fail(TM_ERR_ARG, "%s: frame %d: row pitch %lld below the %d columns kept", fn, k, (long long)pitch, b.clip[2]);
    const int64_t plane = (int64_t)(b.clip[1] - 1) * pitch + b.clip[2];
    if (chan_stride < plane) return fail(TM_ERR_ARG, "%s: frame %d: channel stride %lld below the %lld elements a channel spans", fn, k, (long long)chan_stride, (long long)plane);
    const int64_t span = (int64_t)(b.clip[0] - 1) * chan_stride + plane;
    if (b.origin < 0 || b.origin > canvas_elems - span)
      return fail(TM_ERR_ARG, "%s: frame %d at element %lld (+ %lld) leaves the canvas of %lld elements", fn, k, (long long)b.origin, (long long)span,
                  (long long)canvas_elems);
    d.dst = b.origin;
    for (int i = 0; i < 3; ++i) { d.chunk[i] = b.chunk[i]; d.clip[i] = b.clip[i]; }
  }
  BloscSink sink = {};
  sink.base = canvas; sink.mode = dtype == TM_DTYPE_F32 ? BLOSC_SINK_F32 : BLOSC_SINK_F16;
  sink.cstride = (long)chan_stride; sink.pitch = (long)pitch;
  return blosc_dec_run(fn, frames, P, sink, status, (hipStream_t)stream);
}

// SSIM / PSNR sums of plane pairs (tm_metrics.hip); enqueues only, the per-tile partials are stream-ordered scratch
static int pix_geometry(const char* fn, const char* what, const void* p, int dtype, int W, int64_t pitch, int64_t plane) {
  const int64_t esz = dtype == TM_PIX_F32 ? 4 : 1;
  if (pitch < (int64_t)W * esz) return fail(TM_ERR_ARG, "%s: %s pitch %lld below the row of %lld bytes", fn, what, (long long)pitch, (long long)W * esz);
  if (plane < 0) return fail(TM_ERR_ARG, "%s: negative %s plane stride", fn, what);
  if (esz == 4 && (((uintptr_t)p | (uintptr_t)pitch | (uintptr_t)plane) & 3))
    return fail(TM_ERR_ARG, "%s: float32 %s pointer, pitch and plane stride must be multiples of 4 bytes", fn, what);
  return TM_OK;
}
extern "C" int tm_ssim_planes(const void* x, const void* y, int dtype, int P, int H, int W, int64_t x_pitch, int64_t x_plane,
                              int64_t y_pitch, int64_t y_plane, const float* win_host, int n, float C1, float C2, double* out,
                              void* stream) {
  const char* fn = "tm_ssim_planes";
  if (!x || !y || !win_host || !out) return fail(TM_ERR_ARG, "%s: null x / y / window / out pointer", fn);
  if (dtype != TM_PIX_U8 && dtype != TM_PIX_F32) return fail(TM_ERR_ARG, "%s: dtype %d is neither TM_PIX_U8 nor TM_PIX_F32", fn, dtype);
  if (n < 3 || n > SSIM_MAX_TAPS || !(n & 1)) return fail(TM_ERR_ARG, "%s: window of %d taps (odd, 3 .. %d)", fn, n, SSIM_MAX_TAPS);
  if (P < 1 || P > 65535) return fail(TM_ERR_ARG, "%s: P = %d outside 1 .. 65535", fn, P);
  if (H < n || W < n) return fail(TM_ERR_ARG, "%s: plane %d x %d below the window of %d taps", fn, H, W, n);
  if ((H - n) / SSIM_TH >= 65535) return fail(TM_ERR_ARG, "%s: H = %d takes more than 65535 tile rows", fn, H);
  if (int rc = pix_geometry(fn, "x", x, dtype, W, x_pitch, x_plane)) return rc;
  if (int rc = pix_geometry(fn, "y", y, dtype, W, y_pitch, y_plane)) return rc;
  SsimTaps taps = {};
  double sum = 0.0;
  for (int t = 0; t < n; ++t) { taps.w[SSIM_TAP_PAD + t] = win_host[t]; sum += (double)win_host[t]; }
  taps.sum = (float)(sum * sum); taps.one_minus_sum = (float)(1.0 - sum * sum); taps.n = n;   // the n x n window weighs (sum)^2
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp(st);
  double* partials = (double*)tmp.ordered_floats(2 * ssim_partial_doubles(P, H, W, n), false);
  if (tmp.err) return tmp.report();
  HIP_TRY(launch_ssim_planes(x, y, dtype == TM_PIX_F32, P, H, W, (long)x_pitch, (long)x_plane, (long)y_pitch, (long)y_plane, taps, C1, C2,
                             partials, out, st));
  return TM_OK;
}

// One MS-SSIM level (tm_metrics.hip); enqueues only
extern "C" int tm_avgpool2_pad(const void* src, int dtype, int P, int H, int W, int64_t src_pitch, int64_t src_plane, void* dst,
                               int64_t dst_pitch, int64_t dst_plane, void* stream) {
  const char* fn = "tm_avgpool2_pad";
  if (!src || !dst) return fail(TM_ERR_ARG, "%s: null source / destination", fn);
  if (dtype != TM_PIX_U8 && dtype != TM_PIX_F32) return fail(TM_ERR_ARG, "%s: dtype %d is neither TM_PIX_U8 nor TM_PIX_F32", fn, dtype);
  if (P < 1 || P > 65535) return fail(TM_ERR_ARG, "%s: P = %d outside 1 .. 65535", fn, P);
  if (H < 1 || W < 1) return fail(TM_ERR_ARG, "%s: H and W must be positive, got %d x %d", fn, H, W);
  if (int rc = pix_geometry(fn, "source", src, dtype, W, src_pitch, src_plane)) return rc;
  if (int rc = pix_geometry(fn, "destination", dst, TM_PIX_F32, (W + 1) / 2, dst_pitch, dst_plane)) return rc;
  HIP_TRY(launch_avgpool2_pad(src, dtype == TM_PIX_F32, P, H, W, (long)src_pitch, (long)src_plane, dst, (long)dst_pitch, (long)dst_plane,
                              (hipStream_t)stream));
  return TM_OK;
}

// SSIM / PSNR sums of volume pairs, the 3-D window (tm_metrics.hip); enqueues only
static int vol_geometry(const char* fn, const char* what, const void* p, int dtype, int H, int W, int64_t pitch, int64_t depth, int64_t vol) {
  const int64_t esz = dtype == TM_PIX_F32 ? 4 : 1;
  if (int rc = pix_geometry(fn, what, p, dtype, W, pitch, vol)) return rc;
  const int64_t extent = (int64_t)(H - 1) * pitch + (int64_t)W * esz;
  if (depth < extent)
    return fail(TM_ERR_ARG, "%s: %s depth stride %lld below the extent of one plane, %lld bytes", fn, what, (long long)depth, (long long)extent);
  if (esz == 4 && (depth & 3)) return fail(TM_ERR_ARG, "%s: float32 %s depth stride must be a multiple of 4 bytes", fn, what);
  return TM_OK;
}
extern "C" int tm_ssim_volumes(const void* x, const void* y, int dtype, int V, int D, int H, int W, int64_t x_pitch, int64_t x_depth,
                               int64_t x_vol, int64_t y_pitch, int64_t y_depth, int64_t y_vol, const float* win_host, int n, float C1,
                               float C2, double* out, void* stream) {
  const char* fn = "tm_ssim_volumes";
  if (!x || !y || !win_host || !out) return fail(TM_ERR_ARG, "%s: null x / y / window / out pointer", fn);
  if (dtype != TM_PIX_U8 && dtype != TM_PIX_F32) return fail(TM_ERR_ARG, "%s: dtype %d is neither TM_PIX_U8 nor TM_PIX_F32", fn, dtype);
  if (n < 3 || n > SSIM3_TAPS || !(n & 1))
    return fail(TM_ERR_ARG, "%s: window of %d taps (odd, 3 .. %d: a lane keeps the depth window of every output in registers)", fn, n,
                SSIM3_TAPS);
  if (V < 1 || V > 65535) return fail(TM_ERR_ARG, "%s: V = %d outside 1 .. 65535", fn, V);
  if (D < n || H < n || W < n) return fail(TM_ERR_ARG, "%s: volume %d x %d x %d below the window of %d taps", fn, D, H, W, n);
  if ((H - n) / SSIM3_TH >= 65535) return fail(TM_ERR_ARG, "%s: H = %d takes more than 65535 tile rows", fn, H);
  if (int rc = vol_geometry(fn, "x", x, dtype, H, W, x_pitch, x_depth, x_vol)) return rc;
  if (int rc = vol_geometry(fn, "y", y, dtype, H, W, y_pitch, y_depth, y_vol)) return rc;
  if (x_pitch > ((int64_t)1 << 26) || y_pitch > ((int64_t)1 << 26))   // a tile's 26 rows are addressed with 32-bit offsets
    return fail(TM_ERR_ARG, "%s: pitch %lld above 2^26 bytes", fn, (long long)(x_pitch > y_pitch ? x_pitch : y_pitch));
  Ssim3Taps taps = {};
  double sum = 0.0;
  for (int t = 0; t < n; ++t) { taps.w[t] = win_host[t]; sum += (double)win_host[t]; }
  const double s3 = sum * sum * sum;                                 // the n x n x n window weighs (sum)^3
  taps.sum = (float)s3; taps.one_minus_sum = (float)(1.0 - s3); taps.n = n;
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp(st);
  double* partials = (double*)tmp.ordered_floats(2 * ssim3_partial_doubles(V, H, W, n), false);
  if (tmp.err) return tmp.report();
  HIP_TRY(launch_ssim_volumes(x, y, dtype == TM_PIX_F32, V, D, H, W, (long)x_pitch, (long)x_depth, (long)x_vol, (long)y_pitch, (long)y_depth,
                              (long)y_vol, taps, C1, C2, partials, out, st));
  return TM_OK;
}

// One 5-D MS-SSIM level (tm_metrics.hip); enqueues only
extern "C" int tm_avgpool2_pad3(const void* src, int dtype, int V, int D, int H, int W, int64_t src_pitch, int64_t src_depth, int64_t src_vol,
                                void* dst, int64_t dst_pitch, int64_t dst_depth, int64_t dst_vol, void* stream) {
  const char* fn = "tm_avgpool2_pad3";
  if (!src || !dst) return fail(TM_ERR_ARG, "%s: null source / destination", fn);
  if (dtype != TM_PIX_U8 && dtype != TM_PIX_F32) return fail(TM_ERR_ARG, "%s: dtype %d is neither TM_PIX_U8 nor TM_PIX_F32", fn, dtype);
  if (V < 1 || V > 65535) return fail(TM_ERR_ARG, "%s: V = %d outside 1 .. 65535", fn, V);
  if (D < 1 || H < 1 || W < 1) return fail(TM_ERR_ARG, "%s: D, H and W must be positive, got %d x %d x %d", fn, D, H, W);
  const int64_t outs = (int64_t)((D + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2);
  if (outs > ((int64_t)1 << 38)) return fail(TM_ERR_ARG, "%s: %lld outputs per volume exceed one launch (2^38)", fn, (long long)outs);
  if (int rc = vol_geometry(fn, "source", src, dtype, H, W, src_pitch, src_depth, src_vol)) return rc;
  if (int rc = vol_geometry(fn, "destination", dst, TM_PIX_F32, (H + 1) / 2, (W + 1) / 2, dst_pitch, dst_depth, dst_vol)) return rc;
  HIP_TRY(launch_avgpool2_pad3(src, dtype == TM_PIX_F32, V, D, H, W, (long)src_pitch, (long)src_depth, (long)src_vol, dst, (long)dst_pitch,
                               (long)dst_depth, (long)dst_vol, (hipStream_t)stream));
  return TM_OK;
}

// Timing hook of the conv weight gradient on random device data (uniform in [-1, 1)): engine 0 = conv_wgrad_kernel (VALU),
// 1 = conv_wgrad_mfma_kernel + its chunk reduction.  One warm-up launch, then `reps` measurements of `iters` launches between two
// events each: ms_per_launch_host[r] = milliseconds per launch of repetition r (their spread is the noise of identical calls).
__global__ void fill_f32_kernel(float* p, size_t n, unsigned seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned hsh = (unsigned)i * 2654435761u ^ (unsigned)(i >> 32) * 40503u ^ seed;
    hsh ^= hsh >> 15; hsh *= 2246822519u; hsh ^= hsh >> 13; hsh *= 3266489917u; hsh ^= hsh >> 16;
    p[i] = (float)(hsh >> 8) * (1.0f / 8388608.0f) - 1.0f;
  }
}
extern "C" int tm_op_conv_wgrad_time(int N, int Cin, int Cout, int Z, int S, int ksize, int engine, int iters, int reps,
                                     float* ms_per_launch_host, void* stream) {
  if (!ms_per_launch_host || iters < 1 || reps < 1 || (engine != 0 && engine != 1)) return fail(TM_ERR_ARG, "bad argument");
  if (int rc = resident_geo(N, Cin, Cout, Z, S, ksize)) return rc;
  if (!engine && Z > 4) return fail(TM_ERR_ARG, "engine 0 (the VALU kernel): Z must be 1 .. 4 (got %d)", Z);
  const int taps = ksize == 1 ? 1 : 27;
  hipStream_t st = (hipStream_t)stream;
  TV x = cb8_view(nullptr, N, Cin, Z, S, S), dy = cb8_view(nullptr, N, Cout, Z, S, S);
  const size_t nx = (size_t)N * x.nstride, ny = (size_t)N * dy.nstride, ns = conv_wgrad_scratch_floats(N, Z, S, Cin, Cout, taps);
  DevTmp tmp;
  x.p = tmp.alloc<float>(nx); dy.p = tmp.alloc<float>(ny);
  float* dw = tmp.alloc<float>((size_t)Cout * Cin * taps);
  float* scratch = (engine && ns) ? tmp.alloc<float>(ns) : nullptr;
  hipEvent_t e0 = tmp.event(), e1 = tmp.event();
  if (tmp.err) return tmp.report();
  hipLaunchKernelGGL(fill_f32_kernel, dim3(2048), dim3(256), 0, st, x.p, nx, 11u);
  hipLaunchKernelGGL(fill_f32_kernel, dim3(2048), dim3(256), 0, st, dy.p, ny, 23u);
  auto run = [&]() { return engine ? launch_conv_wgrad_mfma(x, dy, dw, Cin, Cout, taps, 0, scratch, st) : launch_conv_wgrad(x, dy, dw, Cin, Cout, taps, st); };
  if (int rc = finish(st, run(), "conv wgrad (timing warm-up)")) return rc;
  for (int r = 0; r < reps; ++r) {
    hipError_t e = hipEventRecord(e0, st);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = run();
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (int rc = finish(st, e, "conv wgrad (timing)")) return rc;
    HIP_TRY(hipEventElapsedTime(ms_per_launch_host + r, e0, e1));
    ms_per_launch_host[r] /= (float)iters;
  }
  return TM_OK;
}

// Timing hook of the rank sum on random device data (fill_f32_kernel): one warm-up launch, then `reps` measurements of `iters`
// launches between two events each
extern "C" int tm_op_rank_sum_time(int W, long n, int iters, int reps, float* ms_per_launch_host, void* stream) {
  if (!ms_per_launch_host || iters < 1 || reps < 1) return fail(TM_ERR_ARG, "bad argument");
  if (int rc = rank_sum_args(W, n)) return rc;
  if (n < 1) return fail(TM_ERR_ARG, "rank sum timing: n must be positive");
  hipStream_t st = (hipStream_t)stream;
  DevTmp tmp;
  float* parts = tmp.alloc<float>((size_t)W * n);
  float* out = tmp.alloc<float>((size_t)n);
  hipEvent_t e0 = tmp.event(), e1 = tmp.event();
  if (tmp.err) return tmp.report();
  hipLaunchKernelGGL(fill_f32_kernel, dim3(2048), dim3(256), 0, st, parts, (size_t)W * n, 11u);
  if (int rc = finish(st, launch_rank_sum(parts, out, W, n, st), "rank sum (timing warm-up)")) return rc;
  for (int r = 0; r < reps; ++r) {
    hipError_t e = hipEventRecord(e0, st);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_rank_sum(parts, out, W, n, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (int rc = finish(st, e, "rank sum (timing)")) return rc;
    HIP_TRY(hipEventElapsedTime(ms_per_launch_host + r, e0, e1));
    ms_per_launch_host[r] /= (float)iters;
  }
  return TM_OK;
}
