// C-ABI (include/teramind_hip.h) + host-side executor of the UNet / sampler / gene-attention
// path.  The layer graph is the reference's `ours` model (model/unet_ours.py:82-426),
// re-scheduled for inference: time embedding and every ResBlock's emb_layers computed once
// per image, concat / collage / resample never materialised on their own (they are gather
// rules of the prep kernel), skip tensors never cloned, `o == 1` decoder pass optional.
// The single-operator entry points (tm_op_*) live in tm_ops.hip.
#include "../../include/teramind_hip.h"
#include "tm_kernels.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <type_traits>
#include <vector>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace tmk;

// the message behind tm_last_error(), shared by every C-ABI unit (tm_ops.hip, tm_io.hip)
static thread_local char g_err[512] = "";
int tmk::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static const int RNA_TAIL[3] = {128, 64, 32};          // model/unet_ours.py:278-279

// ------------------------------------------------------------------------------------------
struct HostParam {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
};

struct ResW {
  std::string pfx;
  std::vector<int> seg;       // real channels of each concat source
  int cin = 0, cbi = 0, cout = 0;
  bool has_skip = false;
  bool up = false;            // ResBlock(up=True): in_layers' conv also packed as phase weights of the upsampled-input form
  ConvW c1, c2, skip, c1u;
  const float* n1 = nullptr;  // [cbi*8] virtual order
  const float* n2 = nullptr;  // [cout]
  const uint16_t *c1h = nullptr, *c2h = nullptr;   // bf16 packed 3x3x3 weights (TM_DTYPE_BF16)
  const uint16_t* c1uh = nullptr;                  // up blocks: in_layers' conv as phase weights of the upsampled-input form
  const uint16_t* skiph = nullptr;
  int emb_off = 0;
  // fp32: out_layers' norm -> modulate -> SiLU runs in c1's epilogue (conv3d_zpair<0, *, true>) wherever the launch takes the
  // 128-voxel tile.  Decided once, where c1 is packed (conv_pick_form)
  bool fuse_mid = false;
  // a decoder block of the deepest level (its launches are the smallest of the step: the interior patches at patch / 8): ROLE_DEEP
  bool dec_deep = false;
};
struct AttnW {
  std::string pfx;
  int C = 0, G = 0;
  ConvW ada, q, kv, proj, fc1, fc2;
  const float *n1 = nullptr, *n2 = nullptr, *qn = nullptr, *kn = nullptr;
  const uint16_t *adah = nullptr, *qh = nullptr, *kvh = nullptr, *projh = nullptr, *fc1h = nullptr, *fc2h = nullptr;
};
struct DirectW {
  const float* w = nullptr;   // [tap][Cin][Cop]
  const float* bias = nullptr;
  int Cin = 0, Cout = 0, kz = 1, ky = 1, kx = 1;
};
struct Op {           // one entry of a TimestepEmbedSequential
  int kind;           // 0 res, 1 attn
  int idx;            // index into res / attn
  int mode;           // RS_*
};
struct EncEntry { int lvl; bool cat; std::vector<Op> ops; };
struct DecEntry { int lvl; std::vector<Op> ops; };

struct tm_model {
  tm_config cfg;
  int z = 0, gn = 0, D = 0, L = 4;
  // the form of every fp32 conv is conv_pick_form's, fixed at pack time (tm_model_finalize) and never by N; deep8: every level's
  // plane is at least 8 x 8 (patch size 64 or 128)
  bool deep8 = false;
  int rw[4];                          // rna pyramid widths
  std::vector<std::pair<std::string, std::vector<int64_t>>> spec;
  std::map<std::string, HostParam> host;
  bool finalized = false;
  float* arena = nullptr;
  size_t arena_floats = 0;
  // graph
  std::vector<ResW> res;
  std::vector<AttnW> attn;
  std::vector<EncEntry> enc;
  std::vector<Op> mid;
  std::vector<DecEntry> dec;
  int emb_tot = 0;
  // packed pointers
  const float *te_w1 = nullptr, *te_b1 = nullptr, *te_w2 = nullptr, *te_b2 = nullptr;
  const float *emb_w = nullptr, *emb_b = nullptr;
  GeneW gene;
  ConvW downz, pyr[3];
  ConvW pyr16[3];                                    // 16-bit modes: the pyramid convs as 27-tap 16-bit convs (centre z slice)
  const uint16_t* pyrh[3] = {nullptr, nullptr, nullptr};
  DirectW stem, head, downz_d;       // downz_d: direct-conv form of down_z when the MFMA form does not apply
  bool downz_mfma = true;            // kz == 3 on a 4 x 4 (checkpoint config) or 8 x 8 gene grid
  bool gene_mfma = true;             // D == 64, G <= 232, no gene index table: fused MFMA gene-attention kernel
  const int* gene_idx = nullptr;     // device table: gene g reads slot gene_idx[g] (81-gene M2H subset) or null
  const float* out_norm = nullptr;
  // measurement hooks (tm_profile_*)
  bool prof_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
  size_t prof_used = 0;
  double prof_nominal = 0, prof_bytes = 0;
  double prof_xq_flops = 0;              // the part of prof_nominal launched in the x-quad form (13.5 of the nominal 54 taps)
  struct ProfTag { int cin, cout, S, N; double nominal; };
  std::vector<ProfTag> prof_tag;     // per counted launch (TM_PROF_LAYERS)
};

// ------------------------------------------------------------------------------------------
// graph + key enumeration (mirrors the constructor, model/unet_ours.py:134-296)
// ------------------------------------------------------------------------------------------
typedef std::vector<std::pair<std::string, std::vector<int64_t>>> Spec;
static void K(Spec& s, const std::string& k, std::vector<int64_t> shp) { s.emplace_back(k, std::move(shp)); }

static void spec_res(Spec& s, const std::string& p, int cin, int cout, int E) {
  K(s, p + ".in_layers.0.weight", {1, cin, 1, 1});
  K(s, p + ".in_layers.2.weight", {cout, cin, 3, 3, 3});
  K(s, p + ".in_layers.2.bias", {cout});
  K(s, p + ".emb_layers.1.weight", {2 * cout, E});
  K(s, p + ".emb_layers.1.bias", {2 * cout});
  K(s, p + ".out_layers.0.weight", {1, cout, 1, 1});
  K(s, p + ".out_layers.3.weight", {cout, cout, 3, 3, 3});
  K(s, p + ".out_layers.3.bias", {cout});
  if (cin != cout) {
    K(s, p + ".skip_connection.weight", {cout, cin, 1, 1, 1});
    K(s, p + ".skip_connection.bias", {cout});
  }
}
static void spec_attn(Spec& s, const std::string& p, int c, int g) {
  K(s, p + ".norm1.weight", {c});
  for (const char* n : {"q", "k", "v"}) {
    K(s, p + ".attn." + n + ".weight", {c, c});
    K(s, p + ".attn." + n + ".bias", {c});
  }
  K(s, p + ".attn.q_norm.weight", {c});
  K(s, p + ".attn.k_norm.weight", {c});
  K(s, p + ".attn.proj.weight", {c, c});
  K(s, p + ".attn.proj.bias", {c});
  K(s, p + ".norm2.weight", {c});
  K(s, p + ".mlp.fc1.weight", {4 * c, c});
  K(s, p + ".mlp.fc1.bias", {4 * c});
  K(s, p + ".mlp.fc2.weight", {c, 4 * c});
  K(s, p + ".mlp.fc2.bias", {c});
  K(s, p + ".adaLN_modulation.1.weight", {7 * c, g});
  K(s, p + ".adaLN_modulation.1.bias", {7 * c});
}

static int add_res(tm_model* m, const std::string& pfx, std::vector<int> seg, int cout) {
  ResW r;
  r.pfx = pfx; r.seg = seg; r.cout = cout;
  for (int c : seg) { r.cin += c; r.cbi += (c + 7) / 8; }
  r.has_skip = r.cin != cout;
  r.emb_off = m->emb_tot;
  m->emb_tot += 2 * cout;
  m->res.push_back(r);
  return (int)m->res.size() - 1;
}
static int add_attn(tm_model* m, const std::string& pfx, int C, int G) {
  AttnW a;
  a.pfx = pfx; a.C = C; a.G = G;
  m->attn.push_back(a);
  return (int)m->attn.size() - 1;
}

static int build_graph(tm_model* m) {
  const tm_config& c = m->cfg;
  Spec& s = m->spec;
  const int E = c.embed_ch, ch0 = c.net_ch;
  K(s, "time_embed.time_embed.0.weight", {E, ch0});
  K(s, "time_embed.time_embed.0.bias", {E});
  K(s, "time_embed.time_embed.2.weight", {E, E});
  K(s, "time_embed.time_embed.2.bias", {E});
  const int d = m->D, g = c.rna_num;
  const int kzt[17] = {0, 1, 0, 0, 3, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 9};   // MBAblocks.py:472
  const int kz = kzt[c.rna_slc];
  const std::string gp = "rna_blocks.0.0";
  for (const char* n : {"q", "v"}) {
    K(s, gp + ".attn." + n + ".weight", {d, d});
    K(s, gp + ".attn." + n + ".bias", {d});
  }
  K(s, gp + ".attn.q_norm.weight", {d});
  K(s, gp + ".attn.proj.weight", {d, d});
  K(s, gp + ".attn.proj.bias", {d});
  K(s, gp + ".norm2.weight", {d});
  K(s, gp + ".mlp.fc1.weight", {4 * d, d});
  K(s, gp + ".mlp.fc1.bias", {4 * d});
  K(s, gp + ".mlp.fc2.weight", {d, 4 * d});
  K(s, gp + ".mlp.fc2.bias", {d});
  K(s, gp + ".down_z.weight", {g, g, kz, 3, 3});
  K(s, gp + ".down_z.bias", {g});
  if (c.vis_only) return TM_OK;
  for (int rid = 1; rid < 4; ++rid) {
    const std::string p = "rna_blocks." + std::to_string(rid) + ".1";
    K(s, p + ".weight", {m->rw[rid], m->rw[rid - 1], 1, 3, 3});
    K(s, p + ".bias", {m->rw[rid]});
  }
  K(s, "input_blocks.0.0.weight", {ch0, c.n_stain, 1, 3, 3});
  K(s, "input_blocks.0.0.bias", {ch0});
  const int L = m->L;
  int ch = ch0, res = c.patch_size, k = 1;
  std::vector<std::vector<int>> enc_ch(L);
  enc_ch[0].push_back(ch);
  for (int lvl = 0; lvl < L; ++lvl) {
    const int rd = m->rw[L - 1 - lvl];
    for (int i = 0; i < c.num_res_blocks; ++i) {
      const int cout = c.ch_mult[lvl] * ch0;
      const std::string p = "input_blocks." + std::to_string(k);
      EncEntry e; e.lvl = lvl; e.cat = true;
      spec_res(s, p + ".0", ch + rd, cout, E);
      e.ops.push_back({0, add_res(m, p + ".0", {ch, rd}, cout), RS_SAME});
      ch = cout;
      if (res == c.attn_res) {
        spec_attn(s, p + ".1", ch, rd);
        e.ops.push_back({1, add_attn(m, p + ".1", ch, rd), 0});
      }
      m->enc.push_back(e);
      enc_ch[lvl].push_back(ch);
      ++k;
    }
    if (lvl != L - 1) {
      res /= 2;
      const std::string p = "input_blocks." + std::to_string(k) + ".0";
      spec_res(s, p, ch, ch, E);
      EncEntry e; e.lvl = lvl + 1; e.cat = false;
      e.ops.push_back({0, add_res(m, p, {ch}, ch), RS_DOWN2});
      m->enc.push_back(e);
      enc_ch[lvl + 1].push_back(ch);
      ++k;
    }
  }
  spec_res(s, "middle_block.0", ch + m->rw[0], ch, E);
  m->mid.push_back({0, add_res(m, "middle_block.0", {ch, m->rw[0]}, ch), RS_SAME});
  spec_attn(s, "middle_block.1", ch, m->rw[0]);
  m->mid.push_back({1, add_attn(m, "middle_block.1", ch, m->rw[0]), 0});
  spec_res(s, "middle_block.2", ch, ch, E);
  m->mid.push_back({0, add_res(m, "middle_block.2", {ch}, ch), RS_SAME});
  k = 0;
  for (int lvl = L - 1; lvl >= 0; --lvl) {
    const int rd = m->rw[L - 1 - lvl];
    for (int i = 0; i < c.num_res_blocks + 1; ++i) {
      const int skip = enc_ch[lvl].back();
      enc_ch[lvl].pop_back();
      const int cout = c.ch_mult[lvl] * ch0;
      const std::string p = "output_blocks." + std::to_string(k);
      DecEntry e; e.lvl = lvl;
      spec_res(s, p + ".0", ch + skip + rd, cout, E);
      e.ops.push_back({0, add_res(m, p + ".0", {ch, skip, rd}, cout), RS_SAME});
      m->res.back().dec_deep = lvl == L - 1;
      ch = cout;
      int nxt = 1;
      if (res == c.attn_res) {
        spec_attn(s, p + ".1", ch, rd);
        e.ops.push_back({1, add_attn(m, p + ".1", ch, rd), 0});
        nxt = 2;
      }
      if (lvl && i == c.num_res_blocks) {
        res *= 2;
        const std::string pu = p + "." + std::to_string(nxt);
        spec_res(s, pu, ch, ch, E);
        e.ops.push_back({0, add_res(m, pu, {ch}, ch), RS_UP2});
        m->res.back().up = true;
      }
      m->dec.push_back(e);
      ++k;
    }
  }
  K(s, "out.0.weight", {1, ch, 1, 1});
  K(s, "out.2.weight", {c.n_stain, ch0, 1, 3, 3});
  K(s, "out.2.bias", {c.n_stain});
  return TM_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" int tm_version(void) { return TM_ABI_VERSION; }

extern "C" int tm_gene_tile_dense(const int32_t* crd, const void* dat, int64_t nnz, int gblk, int shift_h, int shift_w,
                                  int gsz, int chan_in, int zpad_ch, void* out, void* stream) {
  if (!out || nnz < 0 || (nnz > 0 && (!crd || !dat))) return fail(TM_ERR_ARG, "null / negative argument");
  if (gblk < 1 || gsz < 1 || chan_in < 1 || zpad_ch < 0) return fail(TM_ERR_ARG, "bad gene-tile geometry");
  HIP_TRY(launch_gene_tile_scatter(crd, (const float*)dat, (long)nnz, gblk, shift_h, shift_w, gsz, chan_in, zpad_ch,
                                   (float*)out, (hipStream_t)stream));
  return TM_OK;
}

extern "C" int tm_blosc_decompress(const void* src, size_t src_bytes, void* dst, size_t dst_cap, size_t* out_bytes) {
  return blosc_decompress(src, src_bytes, dst, dst_cap, out_bytes);
}
extern "C" const char* tm_last_error(void) { return g_err; }

extern "C" int tm_model_create(const tm_config* cfg, tm_model** out) {
  if (!cfg || !out) return fail(TM_ERR_ARG, "null argument");
  if (cfg->dtype != TM_DTYPE_F32 && !is_h16(cfg->dtype)) return fail(TM_ERR_ARG, "dtype must be TM_DTYPE_F32, TM_DTYPE_BF16 or TM_DTYPE_F16");
  if (cfg->patch_size != 32 && cfg->patch_size != 64 && cfg->patch_size != 128)
    return fail(TM_ERR_ARG, "patch_size must be 32, 64 or 128 (config_parm.py:47-55), got %d", cfg->patch_size);
  if (cfg->rna_slc != 1 && cfg->rna_slc != 4 && cfg->rna_slc != 8 && cfg->rna_slc != 16)
    return fail(TM_ERR_ARG, "rna_slc must be 1, 4, 8 or 16 (train.py:24-26), got %d", cfg->rna_slc);
  if (cfg->n_stain < 1 || cfg->n_stain > 2 || cfg->rna_num < 1 || cfg->rna_num > 512)
    return fail(TM_ERR_ARG, "n_stain/rna_num out of range");
  if ((cfg->patch_size / 16) * (cfg->patch_size / 16) * cfg->rna_slc > 512)
    return fail(TM_ERR_ARG, "gene-token width gn^2 * rna_slc = %d > 512 is not implemented (patch_size 128 with rna_slc 16)",
                (cfg->patch_size / 16) * (cfg->patch_size / 16) * cfg->rna_slc);
  if (cfg->rna_num == 81 && cfg->rna_slc != 1)
    return fail(TM_ERR_ARG, "the 81-gene human-brain subset requires rna_slc = 1 (model/unet_ours.py:313-316)");
  if (is_h16(cfg->dtype) && cfg->patch_size == 32)
    return fail(TM_ERR_ARG, "TM_DTYPE_BF16 / TM_DTYPE_F16 need patch_size 64 or 128 (no 4 x 4 tile form of the 16-bit conv)");
  if (cfg->net_ch % 64 || cfg->embed_ch % 64 || cfg->embed_ch > 1024)
    return fail(TM_ERR_ARG, "net_ch must be a multiple of 64, embed_ch a multiple of 64 <= 1024");
  tm_model* m = new tm_model();
  m->cfg = *cfg;
  m->z = (cfg->rna_slc + 1) / 2;
  m->deep8 = (cfg->patch_size >> 3) >= 8;                          // the deepest of the four levels: patch / 8
  m->gn = cfg->patch_size / 16;
  m->D = m->gn * m->gn * cfg->rna_slc;
  m->gene_mfma = gene_mfma_rule(m->D, cfg->rna_num, cfg->rna_num == 81);
  m->downz_mfma = cfg->rna_slc == 4 && (m->gn == 4 || m->gn == 8);   // kz == 3 on a grid the MFMA tile forms cover
  m->rw[0] = cfg->rna_num;
  for (int i = 0; i < 3; ++i) m->rw[i + 1] = RNA_TAIL[i];
  int rc = build_graph(m);
  if (rc != TM_OK) { delete m; return rc; }
  for (auto& kv : m->spec) {
    HostParam hp; hp.shape = kv.second;
    m->host[kv.first] = hp;
  }
  *out = m;
  return TM_OK;
}

extern "C" int tm_model_num_params(const tm_model* m) { return m ? (int)m->spec.size() : 0; }
extern "C" const char* tm_model_param_key(const tm_model* m, int i) {
  if (!m || i < 0 || i >= (int)m->spec.size()) return nullptr;
  return m->spec[i].first.c_str();
}

extern "C" int tm_model_load_param(tm_model* m, const char* ref_key, const void* host_ptr, const int64_t* shape,
                                   int ndim, int dtype) {
  if (!m || !ref_key || !host_ptr || !shape) return fail(TM_ERR_ARG, "null argument");
  if (m->finalized) return fail(TM_ERR_STATE, "model already finalized");
  if (dtype != TM_DTYPE_F32) return fail(TM_ERR_ARG, "only fp32 parameters accepted");
  auto it = m->host.find(ref_key);
  if (it == m->host.end()) return fail(TM_ERR_KEY, "unexpected key '%s'", ref_key);
  HostParam& hp = it->second;
  if ((int)hp.shape.size() != ndim) return fail(TM_ERR_KEY, "key '%s': rank %d, expected %d", ref_key, ndim, (int)hp.shape.size());
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (hp.shape[i] != shape[i]) return fail(TM_ERR_KEY, "key '%s': dim %d is %lld, expected %lld", ref_key, i,
                                             (long long)shape[i], (long long)hp.shape[i]);
    n *= (size_t)shape[i];
  }
  hp.data.assign((const float*)host_ptr, (const float*)host_ptr + n);
  hp.loaded = true;
  return TM_OK;
}

// ---- arena packing -------------------------------------------------------------------------
struct Packer {
  std::vector<float> buf;
  size_t reserve(size_t n) {                 // 64-byte aligned sub-allocations
    size_t off = (buf.size() + 15) / 16 * 16;
    buf.resize(off + n, 0.f);
    return off;
  }
};
struct Fix { const float** slot; size_t off; };
struct FixH { const uint16_t** slot; size_t off; };   // offsets in floats into the same arena

static const std::vector<float>& P(tm_model* m, const std::string& k) { return m->host[k].data; }

// bias zero padded to the cout tiles
static void pack_bias(Packer& pk, std::vector<Fix>& fx, ConvW& cw, const std::vector<float>& b) {
  const size_t boff = pk.reserve((size_t)cw.ntile * 64);
  for (int i = 0; i < cw.Cout; ++i) pk.buf[boff + i] = b[i];
  fx.push_back({&cw.bias, boff});
}
// real channels and padded channel blocks of a concat: every segment is padded to a multiple of 8 ("virtual" cin order)
struct SegSum { int cin = 0, cbi = 0; };
static SegSum seg_sum(const std::vector<int>& seg) {
  SegSum t;
  for (int c : seg) { t.cin += c; t.cbi += (c + 7) / 8; }
  return t;
}
// fp32 conv weights of `wkey` ([Cout][Cin][27], or [9] / [1] for the 1x3x3 and 1x1x1 convs) in `form`, with the bias
static void pack_conv(tm_model* m, Packer& pk, std::vector<Fix>& fx, ConvW& cw, const std::string& wkey,
                      const std::string& bkey, int Cout, const std::vector<int>& seg, int form) {
  const SegSum t = seg_sum(seg);
  // CF_INPLANE of a 3x3x3 pad-1 conv: applied to ONE plane (z_size 1, rna_slc 1) it only ever multiplies its kz = 1 slice
  // with data -- pack those 9 taps and run the in-plane kernel
  std::vector<float> centre;
  const float* wsrc = P(m, wkey).data();
  if (form == CF_INPLANE && P(m, wkey).size() == (size_t)Cout * t.cin * 27) {
    centre.resize((size_t)Cout * t.cin * 9);
    for (size_t i = 0; i < (size_t)Cout * t.cin; ++i)
      for (int k = 0; k < 9; ++k) centre[i * 9 + k] = wsrc[i * 27 + 9 + k];
    wsrc = centre.data();
  }
  cw = conv_w(form, Cout, t.cbi);
  size_t off = pk.reserve(conv_pack_floats(form, Cout, t.cbi));
  conv_pack_host(form, wsrc, Cout, seg.data(), (int)seg.size(), pk.buf.data() + off);
  fx.push_back({&cw.w, off});
  pack_bias(pk, fx, cw, P(m, bkey));
}
// 3x3x3 conv for the bf16 path: bf16 packed weights (tm_conv_bf16.hip layout) + the fp32 bias
static void pack_conv_h(tm_model* m, Packer& pk, std::vector<Fix>& fx, std::vector<FixH>& fxh, ConvW& cw,
                        const uint16_t** wslot, const std::string& wkey, const std::string& bkey, int Cout,
                        const std::vector<int>& seg, bool inplane = false) {
  const SegSum t = seg_sum(seg);
  // inplane: a Conv3d(k = (1,3,3), pad (0,1,1)) run by the 3x3x3 kernel -- its 9 taps sit in the centre z slice, the z - 1
  // and z + 1 slices are zero
  std::vector<float> w27;
  if (inplane) {
    const std::vector<float>& w9 = P(m, wkey);
    w27.assign((size_t)Cout * t.cin * 27, 0.f);
    for (size_t i = 0; i < (size_t)Cout * t.cin; ++i)
      for (int k = 0; k < 9; ++k) w27[i * 27 + 9 + k] = w9[i * 9 + k];
  }
  cw = conv_w(CF_PLANES3, Cout, t.cbi);                // geometry and bias only: the 16-bit pack lives in *wslot
  const size_t elems = conv_bf16_pack_elems(Cout, t.cbi);
  size_t off = pk.reserve((elems + 1) / 2);
  (m->cfg.dtype == TM_DTYPE_F16 ? conv_f16_pack_host : conv_bf16_pack_host)(inplane ? w27.data() : P(m, wkey).data(), Cout, seg.data(),
                                                                            (int)seg.size(), (uint16_t*)(pk.buf.data() + off));
  fxh.push_back({wslot, off});
  pack_bias(pk, fx, cw, P(m, bkey));
}
// rows of several [rows_i][Cin] matrices (Linears, or a 1x1x1 conv over the concat `seg`) stacked into one conv1 weight, with the
// stacked bias.  wslot == nullptr: the fp32 pack behind cw.w; otherwise the 16-bit pack behind *wslot, cw carrying the geometry
// and the bias only.
static void pack_linear_stack(tm_model* m, Packer& pk, std::vector<Fix>& fx, std::vector<FixH>& fxh, ConvW& cw,
                              const uint16_t** wslot, const std::vector<std::string>& pfx, int rows_each,
                              const std::vector<int>& seg) {
  const SegSum t = seg_sum(seg);
  const int Cout = rows_each * (int)pfx.size();
  std::vector<float> w((size_t)Cout * t.cin), b(Cout);
  for (size_t i = 0; i < pfx.size(); ++i) {
    const std::vector<float>& wi = P(m, pfx[i] + ".weight");
    const std::vector<float>& bi = P(m, pfx[i] + ".bias");
    memcpy(w.data() + i * (size_t)rows_each * t.cin, wi.data(), (size_t)rows_each * t.cin * sizeof(float));
    memcpy(b.data() + i * rows_each, bi.data(), rows_each * sizeof(float));
  }
  cw = conv_w(CF_1X1, Cout, t.cbi);
  if (wslot) {
    const size_t off = pk.reserve((conv1_bf16_pack_elems(Cout, t.cbi) + 1) / 2);
    (m->cfg.dtype == TM_DTYPE_F16 ? conv1_f16_pack_host : conv1_bf16_pack_host)(w.data(), Cout, seg.data(), (int)seg.size(),
                                                                                (uint16_t*)(pk.buf.data() + off));
    fxh.push_back({wslot, off});
  } else {
    const size_t off = pk.reserve(conv_pack_floats(CF_1X1, Cout, t.cbi));
    conv_pack_host(CF_1X1, w.data(), Cout, seg.data(), (int)seg.size(), pk.buf.data() + off);
    fx.push_back({&cw.w, off});
  }
  pack_bias(pk, fx, cw, b);
}
static void pack_vec(Packer& pk, std::vector<Fix>& fx, const float** slot, const std::vector<float>& v,
                     const std::vector<int>& seg) {
  size_t off = pk.reserve((size_t)seg_sum(seg).cbi * 8);
  vec_pack_host(v.data(), seg.data(), (int)seg.size(), pk.buf.data() + off);
  fx.push_back({slot, off});
}
static void pack_raw(Packer& pk, std::vector<Fix>& fx, const float** slot, const std::vector<float>& v) {
  size_t off = pk.reserve(v.size());
  memcpy(pk.buf.data() + off, v.data(), v.size() * sizeof(float));
  fx.push_back({slot, off});
}
static void pack_transposed(Packer& pk, std::vector<Fix>& fx, const float** slot, const std::vector<float>& w,
                            int rows, int cols) {           // [rows][cols] -> [cols][rows]
  size_t off = pk.reserve((size_t)rows * cols);
  transpose_host(w.data(), rows, cols, pk.buf.data() + off);
  fx.push_back({slot, off});
}
static void pack_direct(tm_model* m, Packer& pk, std::vector<Fix>& fx, DirectW& dw, const std::string& pfx, int Cout,
                        int Cin, int kz, int ky, int kx) {
  dw.Cin = Cin; dw.Cout = Cout; dw.kz = kz; dw.ky = ky; dw.kx = kx;
  const int taps = kz * ky * kx, Cop = (Cout + 7) / 8 * 8;
  const std::vector<float>& w = P(m, pfx + ".weight");
  size_t off = pk.reserve((size_t)taps * Cin * Cop);
  direct_pack_host(w.data(), Cout, Cin, taps, pk.buf.data() + off);
  fx.push_back({&dw.w, off});
  pack_raw(pk, fx, &dw.bias, P(m, pfx + ".bias"));
}

extern "C" int tm_model_finalize(tm_model* m) {
  if (!m) return fail(TM_ERR_ARG, "null model");
  if (m->finalized) return fail(TM_ERR_STATE, "already finalized");
  for (auto& kv : m->spec)
    if (!m->host[kv.first].loaded) return fail(TM_ERR_KEY, "missing key '%s' (strict load)", kv.first.c_str());
  const tm_config& c = m->cfg;
  Packer pk;
  std::vector<Fix> fx;
  std::vector<FixH> fxh;
  const bool bf16 = is_h16(c.dtype);            // 16-bit operand mode (bf16 or fp16): same packing layout
  pack_raw(pk, fx, &m->te_w1, P(m, "time_embed.time_embed.0.weight"));
  pack_raw(pk, fx, &m->te_b1, P(m, "time_embed.time_embed.0.bias"));
  pack_raw(pk, fx, &m->te_w2, P(m, "time_embed.time_embed.2.weight"));
  pack_raw(pk, fx, &m->te_b2, P(m, "time_embed.time_embed.2.bias"));
  {
    const std::string g = "rna_blocks.0.0";
    const int d = m->D;
    pack_transposed(pk, fx, &m->gene.wq_t, P(m, g + ".attn.q.weight"), d, d);
    pack_raw(pk, fx, &m->gene.bq, P(m, g + ".attn.q.bias"));
    pack_transposed(pk, fx, &m->gene.wv_t, P(m, g + ".attn.v.weight"), d, d);
    pack_raw(pk, fx, &m->gene.bv, P(m, g + ".attn.v.bias"));
    pack_raw(pk, fx, &m->gene.qnorm, P(m, g + ".attn.q_norm.weight"));
    pack_transposed(pk, fx, &m->gene.wp_t, P(m, g + ".attn.proj.weight"), d, d);
    pack_raw(pk, fx, &m->gene.bp, P(m, g + ".attn.proj.bias"));
    pack_raw(pk, fx, &m->gene.norm2, P(m, g + ".norm2.weight"));
    pack_transposed(pk, fx, &m->gene.w1_t, P(m, g + ".mlp.fc1.weight"), 4 * d, d);
    pack_raw(pk, fx, &m->gene.b1, P(m, g + ".mlp.fc1.bias"));
    pack_transposed(pk, fx, &m->gene.w2_t, P(m, g + ".mlp.fc2.weight"), d, 4 * d);
    pack_raw(pk, fx, &m->gene.b2, P(m, g + ".mlp.fc2.bias"));
    if (m->downz_mfma) pack_conv(m, pk, fx, m->downz, g + ".down_z.weight", g + ".down_z.bias", c.rna_num, {c.rna_num},
                                 conv_pick_form(3, ZM_VALID, m->z + 2, m->deep8, ROLE_OP));
    else {
      static const int kzt[17] = {0, 1, 0, 0, 3, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 9};            // MBAblocks.py:472
      pack_direct(m, pk, fx, m->downz_d, g + ".down_z", c.rna_num, c.rna_num, kzt[c.rna_slc], 3, 3);
    }
    if (c.rna_num == 81) {                      // human-brain generalisation: the 81 shared genes (utils/__init__.py:49-57)
      static const int M2H[81] = {1, 4, 5, 11, 21, 22, 23, 24, 25, 27, 35, 38, 40, 55, 56, 57, 61, 67, 69, 70, 75, 84, 90, 91, 96,
                                  108, 111, 113, 118, 130, 134, 137, 139, 145, 152, 155, 158, 165, 170, 171, 179, 180, 189, 191,
                                  206, 215, 223, 229, 230, 235, 241, 243, 253, 288, 297, 301, 309, 329, 337, 344, 346, 370, 372,
                                  378, 380, 395, 410, 436, 441, 442, 443, 458, 465, 467, 472, 478, 487, 492, 493, 494, 496};
      size_t off = pk.reserve(81);
      memcpy(pk.buf.data() + off, M2H, sizeof(M2H));
      fx.push_back({(const float**)&m->gene_idx, off});
    }
  }
  if (!c.vis_only) {
    for (int rid = 1; rid < 4 && !is_h16(c.dtype); ++rid)
      pack_conv(m, pk, fx, m->pyr[rid - 1], "rna_blocks." + std::to_string(rid) + ".1.weight",
                "rna_blocks." + std::to_string(rid) + ".1.bias", m->rw[rid], {m->rw[rid - 1]},
                conv_pick_form(3, ZM_INPLANE, m->z, m->deep8, ROLE_OP));
    if (is_h16(c.dtype))
      for (int rid = 1; rid < 4; ++rid)
        pack_conv_h(m, pk, fx, fxh, m->pyr16[rid - 1], &m->pyrh[rid - 1], "rna_blocks." + std::to_string(rid) + ".1.weight",
                    "rna_blocks." + std::to_string(rid) + ".1.bias", m->rw[rid], {m->rw[rid - 1]}, true);
    pack_direct(m, pk, fx, m->stem, "input_blocks.0.0", c.net_ch, c.n_stain, 1, 3, 3);
    pack_direct(m, pk, fx, m->head, "out.2", c.n_stain, c.net_ch, 1, 3, 3);
    pack_raw(pk, fx, &m->out_norm, P(m, "out.0.weight"));
    // all emb_layers as one [emb_tot][E] matrix
    {
      const int E = c.embed_ch;
      size_t woff = pk.reserve((size_t)m->emb_tot * E), boff = pk.reserve(m->emb_tot);
      for (ResW& r : m->res) {
        const std::vector<float>& w = P(m, r.pfx + ".emb_layers.1.weight");
        const std::vector<float>& b = P(m, r.pfx + ".emb_layers.1.bias");
        memcpy(pk.buf.data() + woff + (size_t)r.emb_off * E, w.data(), w.size() * sizeof(float));
        memcpy(pk.buf.data() + boff + r.emb_off, b.data(), b.size() * sizeof(float));
      }
      fx.push_back({&m->emb_w, woff});
      fx.push_back({&m->emb_b, boff});
    }
    for (ResW& r : m->res) {
      if (bf16) {
        pack_conv_h(m, pk, fx, fxh, r.c1, &r.c1h, r.pfx + ".in_layers.2.weight", r.pfx + ".in_layers.2.bias", r.cout, r.seg);
        pack_conv_h(m, pk, fx, fxh, r.c2, &r.c2h, r.pfx + ".out_layers.3.weight", r.pfx + ".out_layers.3.bias", r.cout, {r.cout});
        if (r.up && m->z == 2 && r.cout % 128 == 0) {          // phase weights of the upsampled-input form (bias: c1's)
          const size_t off = pk.reserve((conv_bf16_pack_ups_elems(r.cout, r.cbi) + 1) / 2);
          (c.dtype == TM_DTYPE_F16 ? conv_f16_pack_ups_host : conv_bf16_pack_ups_host)(
              P(m, r.pfx + ".in_layers.2.weight").data(), r.cout, r.seg.data(), (int)r.seg.size(), (uint16_t*)(pk.buf.data() + off));
          fxh.push_back({&r.c1uh, off});
        }
      } else {
        const int role = ROLE_RES | (r.dec_deep ? ROLE_DEEP : 0);
        pack_conv(m, pk, fx, r.c1, r.pfx + ".in_layers.2.weight", r.pfx + ".in_layers.2.bias", r.cout, r.seg,
                  conv_pick_form(3, ZM_PAD1, m->z, m->deep8, role | (r.cout == 64 ? ROLE_C1_64 : 0), &r.fuse_mid));
        if (r.up && m->z == 2)                               // phase weights of the upsampled-input form + their own copy of the bias
          pack_conv(m, pk, fx, r.c1u, r.pfx + ".in_layers.2.weight", r.pfx + ".in_layers.2.bias", r.cout, r.seg,
                    conv_pick_form(3, ZM_UPS, m->z, m->deep8, role));
        pack_conv(m, pk, fx, r.c2, r.pfx + ".out_layers.3.weight", r.pfx + ".out_layers.3.bias", r.cout, {r.cout},
                  conv_pick_form(3, ZM_PAD1, m->z, m->deep8, role));
      }
      if (r.has_skip)
        pack_linear_stack(m, pk, fx, fxh, r.skip, bf16 ? &r.skiph : nullptr, {r.pfx + ".skip_connection"}, r.cout, r.seg);
      pack_vec(pk, fx, &r.n1, P(m, r.pfx + ".in_layers.0.weight"), r.seg);
      pack_raw(pk, fx, &r.n2, P(m, r.pfx + ".out_layers.0.weight"));
    }
    for (AttnW& a : m->attn) {
      auto slot = [&](const uint16_t** h) { return bf16 ? h : nullptr; };
      pack_linear_stack(m, pk, fx, fxh, a.ada, slot(&a.adah), {a.pfx + ".adaLN_modulation.1"}, 7 * a.C, {a.G});
      pack_linear_stack(m, pk, fx, fxh, a.q, slot(&a.qh), {a.pfx + ".attn.q"}, a.C, {a.C});
      pack_linear_stack(m, pk, fx, fxh, a.kv, slot(&a.kvh), {a.pfx + ".attn.k", a.pfx + ".attn.v"}, a.C, {a.C});
      pack_linear_stack(m, pk, fx, fxh, a.proj, slot(&a.projh), {a.pfx + ".attn.proj"}, a.C, {a.C});
      pack_linear_stack(m, pk, fx, fxh, a.fc1, slot(&a.fc1h), {a.pfx + ".mlp.fc1"}, 4 * a.C, {a.C});
      pack_linear_stack(m, pk, fx, fxh, a.fc2, slot(&a.fc2h), {a.pfx + ".mlp.fc2"}, a.C, {4 * a.C});
      pack_raw(pk, fx, &a.n1, P(m, a.pfx + ".norm1.weight"));
      pack_raw(pk, fx, &a.n2, P(m, a.pfx + ".norm2.weight"));
      pack_raw(pk, fx, &a.qn, P(m, a.pfx + ".attn.q_norm.weight"));
      pack_raw(pk, fx, &a.kn, P(m, a.pfx + ".attn.k_norm.weight"));
    }
  }
  m->arena_floats = (pk.buf.size() + 15) / 16 * 16;
  pk.buf.resize(m->arena_floats, 0.f);
  HIP_TRY(hipMalloc((void**)&m->arena, m->arena_floats * sizeof(float)));
  HIP_TRY(hipMemcpy(m->arena, pk.buf.data(), m->arena_floats * sizeof(float), hipMemcpyHostToDevice));
  for (Fix& f : fx) *f.slot = m->arena + f.off;
  for (FixH& f : fxh) *f.slot = (const uint16_t*)(m->arena + f.off);
  if (bf16) HIP_TRY(c.dtype == TM_DTYPE_F16 ? init_f16_device() : init_bf16_device());
  m->host.clear();
  m->finalized = true;
  return TM_OK;
}

extern "C" size_t tm_model_arena_bytes(const tm_model* m) { return m ? m->arena_floats * sizeof(float) : 0; }
extern "C" void* tm_model_arena_ptr(tm_model* m) { return m ? (void*)m->arena : nullptr; }

extern "C" int tm_profile_enable(tm_model* m, int on) {
  if (!m) return fail(TM_ERR_ARG, "null model");
  m->prof_on = on != 0;
  return TM_OK;
}
extern "C" int tm_profile_collect(tm_model* m, tm_prof_stats* out) {
  if (!m || !out) return fail(TM_ERR_ARG, "null argument");
  memset(out, 0, sizeof(*out));
  if (m->prof_used) HIP_TRY(hipEventSynchronize(m->prof_ev[m->prof_used - 1].second));
  // TM_PROF_LAYERS=<file>: one line per counted launch (diagnosis: which layers sit furthest below the kernel's average)
  static const char* layer_log = getenv("TM_PROF_LAYERS");
  FILE* lf = (layer_log && m->prof_tag.size() == m->prof_used) ? fopen(layer_log, "a") : nullptr;
  for (size_t i = 0; i < m->prof_used; ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m->prof_ev[i].first, m->prof_ev[i].second));
    out->total_ms += ms;
    if (lf) fprintf(lf, "%zu cin %d cout %d S %d N %d nominal_gflop %.3f ms %.4f\n", i, m->prof_tag[i].cin, m->prof_tag[i].cout,
                    m->prof_tag[i].S, m->prof_tag[i].N, m->prof_tag[i].nominal * 1e-9, ms);
  }
  if (lf) fclose(lf);
  m->prof_tag.clear();
  out->launches = m->prof_used;
  out->nominal_flops = m->prof_nominal;
  // Z == 2: the pair form issues 27 taps per plane PAIR (27 of the nominal 54), the z-skip form 18 of 27 per plane; Z == 1: the
  // centre slice only (9); Z >= 3: all 27 (zero planes staged)
  // (the 16-bit conv never stages z-padding planes: (3Z - 2) / 3Z of the taps for any Z)
  // per layer: a launch in the x-quad form issues 54 tap-products per EIGHT outputs, 13.5 of the nominal 54
  out->executed_flops = (m->prof_nominal - m->prof_xq_flops) *
                            (is_h16(m->cfg.dtype) ? (3.0 * m->z - 2.0) / (3.0 * m->z)
                                                  : (m->z == 2 ? (conv_pick_form(3, ZM_PAD1, 2, false, ROLE_RES) == CF_PAIR ? 27.0 / 54.0 : 18.0 / 27.0)
                                                               : (m->z == 1 ? 9.0 / 27.0 : 1.0))) +
                        m->prof_xq_flops * (13.5 / 54.0);
  out->alg_bytes = m->prof_bytes;
  m->prof_used = 0; m->prof_nominal = 0; m->prof_bytes = 0; m->prof_xq_flops = 0;
  return TM_OK;
}

extern "C" int tm_model_destroy(tm_model* m) {
  if (!m) return TM_OK;
  for (auto& e : m->prof_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (m->arena) (void)hipFree(m->arena);
  delete m;
  return TM_OK;
}

// ------------------------------------------------------------------------------------------
// executor
// ------------------------------------------------------------------------------------------
struct Ctx {
  tm_model* m = nullptr;
  char* base = nullptr;
  size_t cap = 0, top = 0, peak = 0;
  bool dry = false;
  hipStream_t s = nullptr;
  int b = 0, p1 = 0, p2 = 0, Ne = 0, Nd = 0;
  hipError_t err = hipSuccess;
  const float* ss = nullptr;      // [b][emb_tot]

  // buf: the workspace or pyramid buffer the tensors are carved from; nullptr: a dry run (sizes and layout only)
  void init(tm_model* m_, int b_, int p1_, int p2_, void* buf, size_t bytes, hipStream_t s_) {
    m = m_; s = s_;
    b = b_; p1 = p1_; p2 = p2_; Ne = b * p1 * p2; Nd = b * (p1 - 1) * (p2 - 1);
    if (buf) {
      base = (char*)(((uintptr_t)buf + 255) / 256 * 256);
      cap = bytes - (size_t)(base - (char*)buf);
    } else dry = true;
  }
  bool h16() const { return is_h16(m->cfg.dtype); }
  float* alloc_f(size_t nfloats) {
    size_t off = (top + 255) / 256 * 256;
    top = off + nfloats * sizeof(float);
    if (top > peak) peak = top;
    if (dry) return (float*)(uintptr_t)256;     // never dereferenced
    if (top > cap) { if (err == hipSuccess) err = hipErrorOutOfMemory; return (float*)base; }
    return (float*)(base + off);
  }
  TV tensor(int N, int C, int Z, int S) {
    TV t = cb8_view(nullptr, N, C, Z, S, S);
    t.p = alloc_f((size_t)N * t.nstride);
    return t;
  }
  TVH tensor_h(int N, int Cb_even, int Z, int S) {           // bf16 CB8 (conv27_bf16 input)
    TVH t = as_h(cb8_view(nullptr, N, Cb_even * 8, Z, S, S));
    t.p = (uint16_t*)alloc_f(((size_t)N * t.nstride + 1) / 2);
    return t;
  }
  // Activation-stream tensor (block outputs, skips, RNA pyramid levels): fp32 CB8 in TM_DTYPE_F32; in the 16-bit modes
  // the SAME geometry with 16-bit elements (the TV's `p` then points at uint16_t data and `nstride` counts elements).
  TV tensor_s(int N, int C, int Z, int S) {
    TV t = cb8_view(nullptr, N, C, Z, S, S);
    t.p = alloc_f(h16() ? ((size_t)N * t.nstride + 1) / 2 : (size_t)N * t.nstride);
    return t;
  }
  void check(hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; }
  // A block-input / glue pass (launch_prep) of N output patches of Z x S x S, with what the context knows; per_image: output
  // patches per image (the row of a per-image modulation)
  PrepLaunch prep(int N, int Z, int S, int per_image = 1) const {
    PrepLaunch P = prep_start(N, Z, S);
    P.p1 = p1; P.p2 = p2; P.per_image = per_image; P.h_f16 = m->cfg.dtype == TM_DTYPE_F16;
    return P;
  }
  // a stream tensor (tensor_s) as a source of P: fp32, or 16-bit in the 16-bit modes
  void stream_src(PrepLaunch& P, const TV& t, bool collage = false) const {
    if (h16()) prep_src(P, as_h(t), collage);
    else prep_src(P, t, collage);
  }
  void run(const PrepLaunch& P) { if (!dry) check(launch_prep(P, s)); }
};
struct Src { TV t; bool collage; };


// Debug taps: with TM_DEBUG_DIR set, every block output is written (NCDHW fp32, raw) to
// $TM_DEBUG_DIR/<name>.bin after a stream sync.  Test/diagnostic aid only.
static const char* debug_dir() {
  static const char* d = getenv("TM_DEBUG_DIR");
  return (d && *d) ? d : nullptr;
}
static void dump_tv(Ctx& cx, const std::string& name, const TV& t_in) {
  if (cx.dry || !debug_dir()) return;
  TV t = t_in;
  const size_t n = (size_t)t.N * t.C * t.Z * t.H * t.W;
  float* dev = nullptr;
  float* f32copy = nullptr;
  if (hipMalloc((void**)&dev, n * sizeof(float)) != hipSuccess) return;
  if (is_h16(cx.m->cfg.dtype)) {              // 16-bit stream tensor -> fp32 CB8 copy (prep kernel, no norm / act)
    if (hipMalloc((void**)&f32copy, (size_t)t.N * t.nstride * sizeof(float)) != hipSuccess) { (void)hipFree(dev); return; }
    PrepLaunch P = cx.prep(t.N, t.Z, t.H);
    prep_src(P, as_h(t));
    t.p = f32copy;
    prep_out(P, t);
    if (launch_prep(P, cx.s) != hipSuccess) { (void)hipFree(dev); (void)hipFree(f32copy); return; }
  }
  std::vector<float> host(n);
  if (launch_from_cb8(t, dev, cx.s) == hipSuccess && hipStreamSynchronize(cx.s) == hipSuccess &&
      hipMemcpy(host.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess) {
    const std::string path = std::string(debug_dir()) + "/" + name + ".bin";
    if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(host.data(), sizeof(float), n, f); fclose(f); }
  }
  (void)hipFree(dev);
  if (f32copy) (void)hipFree(f32copy);
}

// ---- conv launches: the caller fills the launch struct by name, the runners add the dry-run rule, the error latch and the books ----
static ConvLaunch conv(const TV& x, const ConvW& w, const TV& y) {
  ConvLaunch L;
  L.x = x; L.w = w; L.y = y;
  return L;
}
// cw: the geometry and the bias of the 16-bit pack `w`.  y: fp32 output, or with out_h the geometry of the 16-bit one
static ConvLaunchH conv_h(const TVH& x, const uint16_t* w, const ConvW& cw, const TV& y) {
  ConvLaunchH L;
  L.x = x; L.w = w; L.bias = cw.bias; L.Cout = cw.Cout; L.y = y;
  return L;
}
static void out_h(ConvLaunchH& L, const TVH& o) { L.y_h = o.p; L.yh_nstride = o.nstride; }   // write 16-bit o instead of L.y
// The fused mid-section of ResBlock w (out_layers' norm -> modulate -> SiLU) in the epilogue of its first conv, which then writes
// a2, the second conv's input, instead of L.y
template <class Launch, class A2>
static void fuse_mid_section(Launch& L, const Ctx& cx, const ResW& w, int per_image, const A2& a2) {
  L.fuse_norm = 1; L.a2 = a2; L.norm_w = w.n2; L.per_image = per_image;
  L.mod_scale = cx.ss + w.emb_off; L.mod_shift = cx.ss + w.emb_off + w.cout; L.mod_stride = cx.m->emb_tot;
  if constexpr (std::is_same<Launch, ConvLaunch>::value) L.inv_c = 1.0f / (float)w.cout;   // the 16-bit kernel knows its Cout
}

// What one counted 3x3x3 launch adds to the books of tm_profile_collect
struct ConvBook { int cin, cout, S, N; double vox, bytes; bool xquad; };
// The profiling bracket of the 3x3x3 launchers: ensure an event pair, record, launch, record, book.  book == nullptr or
// profiling off: the launch alone.
template <class LaunchFn>
static void launch_booked(Ctx& cx, const ConvBook* book, LaunchFn launch) {
  tm_model* m = cx.m;
  if (!book || !m->prof_on) { cx.check(launch()); return; }
  if (m->prof_used == m->prof_ev.size()) {
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i)
      if (hipEventCreate(&ev[i]) != hipSuccess) {
        if (i) (void)hipEventDestroy(ev[0]);
        cx.check(hipErrorOutOfMemory);
        return;
      }
    m->prof_ev.emplace_back(ev[0], ev[1]);
  }
  cx.check(hipEventRecord(m->prof_ev[m->prof_used].first, cx.s));
  cx.check(launch());
  cx.check(hipEventRecord(m->prof_ev[m->prof_used].second, cx.s));
  m->prof_used++;
  const double nominal = 2.0 * book->cin * book->cout * 27.0 * book->vox;
  m->prof_nominal += nominal;
  if (book->xquad) m->prof_xq_flops += nominal;
  m->prof_tag.push_back({book->cin, book->cout, book->S, book->N, nominal});
  m->prof_bytes += book->bytes;
}

// Split K of an x-quad conv (xquad_ksplit, a function of the shapes alone: the dry pass carves what the real pass carves): the
// partial sums come from the context and live until the block's mark.  The factor belongs to the layer, as its form does, and
// never follows the patch count: another factor is another order of the sum, and one image alone, a tile alone and the same
// image or tile inside a larger call must agree bit for bit (tests/test_gpu_fullsize.py, tests/test_gpu_sweep.py).  So the
// decoder blocks of the deepest level (`deep`), whose launches at the benchmark's 32 patches are the ones xquad_ksplit splits,
// take its factor for that launch, 2, at every patch count -- also where the launch would fill the chip unsplit and the rule
// itself says 1 (the 400 patches of a tile) -- and every other layer stays unsplit
static void split_k(Ctx& cx, ConvLaunch& L, bool deep) {
  if (!deep || L.w.form != CF_XQUAD || L.res_half) return;
  L.xquad_ksplit = xquad_split_on() && L.w.Cbi / 2 >= XQUAD_SPLIT_FLOOR ? 2 : 1;
  if (L.xquad_ksplit > 1) L.part = cx.alloc_f(xquad_part_floats(L.xquad_ksplit, L.y));
}

// fp32 conv (launch_conv_mfma: every form; a split x-quad launch is the conv and its reduction, both inside the profiling
// bracket).  count_cin: the real input channels of a ResBlock 3x3x3 conv, which is counted; 0:
// not counted (1x1 convs and Linears, the pyramid convs, down_z, the upsampled-input form)
static void run_conv(Ctx& cx, const ConvLaunch& L, int count_cin = 0) {
  if (cx.dry) return;
  const double vox = (double)L.x.N * L.x.Z * L.x.H * L.x.W;
  const ConvBook book = {count_cin, L.w.Cout, L.x.H, L.x.N, vox,
                         4.0 * (vox * L.x.Cb * 8 + (double)L.w.ntile * L.w.Cbi * L.w.taps * 512 + vox * L.y.Cb * 8), L.w.form == CF_XQUAD};
  launch_booked(cx, count_cin ? &book : nullptr, [&] { return launch_conv_mfma(L, cx.s); });
}
// 16-bit 3x3x3 conv; cw: the ConvW behind L.w (pack size).  count_cin as above (0: the in-plane pyramid convs, 9 real taps, and
// the upsampled-input form)
static void run_conv27_h(Ctx& cx, const ConvLaunchH& L, const ConvW& cw, int count_cin) {
  if (cx.dry) return;
  const double vox = (double)L.x.N * L.x.Z * L.x.H * L.x.W;
  const ConvBook book = {count_cin, cw.Cout, L.x.H, L.x.N, vox,
                         2.0 * vox * L.x.Cb * 8 + 2.0 * (double)conv_bf16_pack_elems(cw.Cout, cw.Cbi) +
                             ((L.y_h || L.fuse_norm) ? 2.0 : 4.0) * vox * L.y.Cb * 8 + (L.res_h ? 2.0 * vox * L.y.Cb * 8 : 0.0),
                         false};
  launch_booked(cx, count_cin ? &book : nullptr,
                [&] { return cx.m->cfg.dtype == TM_DTYPE_F16 ? launch_conv27_f16(L, cx.s) : launch_conv27_bf16(L, cx.s); });
}
// 16-bit 1x1 conv / Linear
static void run_conv1_h(Ctx& cx, const ConvLaunchH& L) {
  if (cx.dry) return;
  cx.check(cx.m->cfg.dtype == TM_DTYPE_F16 ? launch_conv1_f16(L, cx.s) : launch_conv1_bf16(L, cx.s));
}
// x = th.cat(sources, 1) (+ to_collage) read in place by the 16-bit 1x1 conv; L.x then carries the geometry only
static void concat_sources(ConvLaunchH& L, const Ctx& cx, const std::vector<Src>& src) {
  L.nsrc = (int)src.size();
  for (int i = 0; i < L.nsrc; ++i) { L.xs[i] = as_h(src[i].t); L.xs_collage[i] = src[i].collage ? 1 : 0; }
  L.p1 = cx.p1; L.p2 = cx.p2;
}

// The block-input pass of ResBlock w: th.cat of the sources (+ to_collage), resampled by `mode`, in_layers' norm and SiLU; the
// caller adds the outputs
static PrepLaunch block_input(const Ctx& cx, const ResW& w, const std::vector<Src>& src, int N, int Z, int S, int per_image, int mode) {
  PrepLaunch P = cx.prep(N, Z, S, per_image);
  for (const Src& sv : src) cx.stream_src(P, sv.t, sv.collage);
  P.resample = mode; P.act = 1;
  prep_norm(P, w.n1, w.cin);
  return P;
}
// The mid-section pass of ResBlock w where it is not fused into the first conv: out_layers' norm, the per-image modulation and
// SiLU from H1; the caller adds the output (the second conv's operand)
static PrepLaunch mid_section(const Ctx& cx, const ResW& w, const TV& H1, int per_image) {
  PrepLaunch P = cx.prep(H1.N, H1.Z, H1.H, per_image);
  cx.stream_src(P, H1);
  P.act = 1;
  prep_norm(P, w.n2, w.cout);
  prep_mod_image(P, cx.ss, w.emb_off, w.cout, cx.m->emb_tot);
  return P;
}

// ResBlock._forward (model/MBAblocks.py:237-299) in the 16-bit modes: every tensor that crosses a block boundary (sources,
// output, the resampled / concatenated x that feeds the skip conv or the residual add) is a 16-bit CB8 stream tensor --
// as under the reference's fp16 autocast, where every conv output and the residual sum are half tensors
// (diffusion/base.py:377).  Norm statistics, modulation, SiLU and all accumulation stay fp32.
static TV res_block_h16(Ctx& cx, const ResW& w, const std::vector<Src>& src, int N, int per_image, int S_out, int mode) {
  tm_model* m = cx.m;
  const int Z = m->z;
  TV out = cx.tensor_s(N, w.cout, Z, S_out);
  const size_t mark = cx.top;
  const int cbe = pair_cb(w.cbi);
  const TV geom = cb8_view(nullptr, N, w.cout, Z, S_out, S_out);      // of the first conv's output where it goes to A2 directly
  const TVH outh = as_h(out);
  if (mode == RS_UP2 && w.c1uh && src.size() == 1 && !src[0].collage && !w.has_skip && !(S_out & (S_out - 1)) && S_out >= 16) {
    // ResBlock(up=True) (MBAblocks.py:254-261,297) without upsampling anything: norm + SiLU on the low-resolution x, the first
    // conv in its upsampled-input form (per-phase 2 x 2 in-plane weights: 8 instead of 18 taps), the second conv's epilogue
    // reads the residual Upsample(x) at (z, y >> 1, x >> 1) of x itself (see the fp32 twin in res_block)
    const int S_in = S_out / 2;
    TVH Al = cx.tensor_h(N, cbe, Z, S_in);
    PrepLaunch P = block_input(cx, w, src, N, Z, S_in, per_image, RS_SAME);
    prep_out_h(P, Al, w.cbi);
    cx.run(P);
    TVH A2u = cx.tensor_h(N, pair_cb(w.cout / 8), Z, S_out);
    ConvLaunchH L1 = conv_h(Al, w.c1uh, w.c1, geom);
    L1.ups = 1;
    if (w.cout == 128) {
      fuse_mid_section(L1, cx, w, per_image, A2u);
      run_conv27_h(cx, L1, w.c1, 0);
    } else {
      TV H1 = cx.tensor_s(N, w.cout, Z, S_out);
      L1.y = H1;
      out_h(L1, as_h(H1));
      run_conv27_h(cx, L1, w.c1, 0);
      PrepLaunch Q = mid_section(cx, w, H1, per_image);
      prep_out_h(Q, A2u, w.cout / 8);
      cx.run(Q);
    }
    const TVH xh = as_h(src[0].t);
    ConvLaunchH L2 = conv_h(A2u, w.c2h, w.c2, out);
    out_h(L2, outh);
    L2.res_h = &xh; L2.res_half = 1;
    run_conv27_h(cx, L2, w.c2, w.cout);
    cx.top = mark;
    return out;
  }
  TVH Ah = cx.tensor_h(N, cbe, Z, S_out), rawh;
  // The concatenated / re-tiled x (MBAblocks.py:252-258,297) is only materialised where it is the RESIDUAL of a block
  // without skip conv (the up / down blocks: resampled x); the skip conv reads the sources in place (conv1's concat input)
  const bool need_raw = !w.has_skip && (mode != RS_SAME || src.size() > 1 || src[0].collage);
  if (w.has_skip && mode != RS_SAME) { cx.check(hipErrorInvalidValue); return out; }    // never in this model family
  if (need_raw) rawh = cx.tensor_h(N, cbe, Z, S_out);
  PrepLaunch P = block_input(cx, w, src, N, Z, S_out, per_image, mode);
  prep_out_h(P, Ah, w.cbi);
  if (need_raw) prep_raw_h(P, rawh);
  cx.run(P);
  TVH A2h = cx.tensor_h(N, pair_cb(w.cout / 8), Z, S_out);
  ConvLaunchH L1 = conv_h(Ah, w.c1h, w.c1, geom);
  if (w.cout == 64 || w.cout == 128) {
    // Cout in {64, 128}: one workgroup holds every cout of its voxels, so out_layers' norm -> modulate -> SiLU runs in the
    // first conv's epilogue and writes the second conv's 16-bit input directly
    fuse_mid_section(L1, cx, w, per_image, A2h);
    run_conv27_h(cx, L1, w.c1, w.cin);
  } else {
    // Cout > 128 (several cout tiles per voxel): the conv output goes through a 16-bit tensor like every other conv
    // output of the 16-bit modes -- under the reference's autocast in_layers' Conv3d returns fp16 and out_layers'
    // LlamaRMSNorm takes its statistics from those half values (MBAblocks.py:21-43 casts the half input up)
    TV H1 = cx.tensor_s(N, w.cout, Z, S_out);
    L1.y = H1;
    out_h(L1, as_h(H1));
    run_conv27_h(cx, L1, w.c1, w.cin);
    PrepLaunch Q = mid_section(cx, w, H1, per_image);
    prep_out_h(Q, A2h, w.cout / 8);
    cx.run(Q);
  }
  TVH resh = as_h(src[0].t);                           // the residual: a single plain source as it stands,
  if (w.has_skip) {
    ConvLaunchH Ls = conv_h(Ah, w.skiph, w.skip, out); // (geometry + padded block count of the virtual concat)
    Ls.x.p = nullptr;
    concat_sources(Ls, cx, src);
    out_h(Ls, outh);
    run_conv1_h(cx, Ls);
    resh = outh;                                       // the skip conv's output, in place,
  } else if (need_raw) {
    resh = as_h(geom);                                 // or rawh (channels < cout only)
    resh.p = rawh.p; resh.nstride = rawh.nstride;
  }
  ConvLaunchH L2 = conv_h(A2h, w.c2h, w.c2, out);
  out_h(L2, outh);
  L2.res_h = &resh;
  run_conv27_h(cx, L2, w.c2, w.cout);
  cx.top = mark;
  return out;
}

// ResBlock._forward (model/MBAblocks.py:237-299)
static TV res_block(Ctx& cx, const ResW& w, const std::vector<Src>& src, int N, int per_image, int S_out, int mode,
                    TV* out_opt) {
  tm_model* m = cx.m;
  if (cx.h16()) return res_block_h16(cx, w, src, N, per_image, S_out, mode);
  const int Z = m->z;
  TV out = out_opt ? *out_opt : cx.tensor(N, w.cout, Z, S_out);
  const size_t mark = cx.top;
  if (mode == RS_UP2 && w.c1u.w && src.size() == 1 && !src[0].collage && !w.has_skip && !(S_out & (S_out - 1))) {
    // ResBlock(up=True) (MBAblocks.py:254-261,297): h = Upsample(x) feeds in_layers, x = Upsample(x) is the residual.  Nothing
    // is upsampled here: norm and SiLU act per voxel, so they run on the low-resolution x (a quarter of the bytes); the first
    // conv is the upsampled-input form (per-phase 2 x 2 in-plane weights: conv3d_zpair_ups, 12 tap-products per plane pair, or
    // with TM_CONV_ZPAIR=0 the z-skip form of conv3d_mfma, 8 instead of 18 taps per plane); the second
    // conv's epilogue reads the residual at (z, y >> 1, x >> 1) of x itself.
    const int S_in = S_out / 2;
    TV A = cx.tensor(N, w.cbi * 8, Z, S_in);
    PrepLaunch P = block_input(cx, w, src, N, Z, S_in, per_image, RS_SAME);
    prep_out(P, A);
    cx.run(P);
    TV A2 = cx.tensor(N, w.cout, Z, S_out), H1 = cx.tensor(N, w.cout, Z, S_out);
    ConvLaunch L1 = conv(A, w.c1u, H1);
    L1.zmode = ZM_UPS;
    run_conv(cx, L1);
    PrepLaunch Q = mid_section(cx, w, H1, per_image);
    prep_out(Q, A2);
    cx.run(Q);
    ConvLaunch L2 = conv(A2, w.c2, out);
    L2.res = &src[0].t; L2.res_half = 1;
    run_conv(cx, L2, w.cout);
    cx.top = mark;
    return out;
  }
  int cin_pad = w.cbi * 8;
  TV A = cx.tensor(N, cin_pad, Z, S_out), raw;
  // the residual / skip-conv input is the CONCATENATED (and resampled) x, MBAblocks.py:252-258,297:
  // it equals a stored tensor only for a single plain source
  const bool need_raw = w.has_skip || mode != RS_SAME || src.size() > 1 || src[0].collage;
  if (need_raw) raw = cx.tensor(N, cin_pad, Z, S_out);
  PrepLaunch P = block_input(cx, w, src, N, Z, S_out, per_image, mode);
  prep_out(P, A);
  if (need_raw) prep_raw(P, raw);
  cx.run(P);
  TV A2 = cx.tensor(N, w.cout, Z, S_out);
  ConvLaunch L1 = conv(A, w.c1, A2);
  // 64 output channels in the pair form's 128-voxel tile: a wave holds every channel of its voxels, so out_layers' norm ->
  // modulate -> SiLU runs in c1's epilogue and H1 is never written (nor allocated: the dry pass takes the same branch)
  if (w.fuse_mid && Z == 2 && conv_tile(CF_PAIR, (long)N * Z * S_out * S_out, 1, S_out, 0) == 2) {
    fuse_mid_section(L1, cx, w, per_image, A2);
    run_conv(cx, L1, w.cin);
  } else {
    TV H1 = cx.tensor(N, w.cout, Z, S_out);
    L1.y = H1;
    split_k(cx, L1, w.dec_deep);
    run_conv(cx, L1, w.cin);
    PrepLaunch Q = mid_section(cx, w, H1, per_image);
    prep_out(Q, A2);
    cx.run(Q);
  }
  if (w.has_skip) run_conv(cx, conv(raw, w.skip, out));
  ConvLaunch L2 = conv(A2, w.c2, out);
  L2.res = w.has_skip ? &out : (need_raw ? &raw : &src[0].t);
  split_k(cx, L2, w.dec_deep);
  run_conv(cx, L2, w.cout);
  cx.top = mark;
  return out;
}

// The conditioning side of an AttnBlock: SiLU(cond), mod = the 7C adaLN tensor Linear(SiLU(cond)) (shift / scale / gate of
// both halves and the cross-cond chunk) and kv = Linear(cross-cond chunk).  cond is an RNA pyramid level, so none of it
// depends on x or t: a caller that keeps the pyramid over the steps of a reverse loop keeps these too (attn_cond_stage).
struct AttnGeom { bool half = false, mfma_core = false; int Sc = 0; };
struct AttnCond {
  TV mod, kv;                 // fp32 mode; 16-bit modes: kv of the generic fp32 attention core
  TVH mod_h, kv_h;            // 16-bit modes (kv_h: the MFMA attention cores)
};

static AttnGeom attn_geom(const tm_model* m, const AttnW& w, int Z, int S) {
  // The conditioning side at HALF resolution.  cond is an RNA pyramid level, and every level leaves its stage through a
  // nearest x2 Upsample (unet_ours.py:290-295, MBAblocks.py:472-479): it -- and with it SiLU(cond), the 7C adaLN modulation
  // Linear(SiLU(cond)) (MBAblocks.py:463-466,487), the cross-cond chunk, k and v (no positional term, :551-556) -- is
  // constant over aligned 2 x 2 voxel blocks, also after to_collage (a shift by S/2, even).  So these tensors are computed
  // once per block of four voxels ([.., Z, S/2, S/2]: a quarter of the Linear work and of the bytes of the largest tensor
  // of the block) and their consumers read entry (z, y >> 1, x >> 1).  Same numbers, bit for bit (TM_ATTN_HALF=0: the
  // full-resolution form, for A/B timing and the equality test).
  static const bool no_half = getenv("TM_ATTN_HALF") && atoi(getenv("TM_ATTN_HALF")) == 0;
  const int C = w.C, Tw = Z * (S / 2) * (S / 2);
  AttnGeom g;
  if (is_h16(m->cfg.dtype)) {
    g.mfma_core = Tw == 128 || Tw == 64 || Tw == 32 || ((Tw == 256 || Tw == 512) && C <= 256);
    g.half = !no_half && (Tw == 128 || Tw == 64 || Tw == 32) && S >= 4 && !(S & (S - 1));
  } else {
    // fp32: where the attention core has the k / v half-resolution read (T = 128 MFMA and T = 32 kernels, C a multiple of 128)
    g.half = !no_half && S >= 4 && !(S & (S - 1)) && C % 128 == 0 && ((Tw == 128 && C <= 512) || Tw == 32);
  }
  g.Sc = g.half ? S / 2 : S;
  return g;
}

// the block's mod and kv, allocated (nothing else: inside a pyramid buffer these are the persistent part)
static AttnCond attn_cond_alloc(Ctx& cx, const AttnW& w, int N, int Z, int S) {
  const AttnGeom g = attn_geom(cx.m, w, Z, S);
  const int C = w.C, cb = C / 8;
  AttnCond A;
  if (is_h16(cx.m->cfg.dtype)) {
    A.mod_h = cx.tensor_h(N, 7 * cb, Z, g.Sc);
    if (g.mfma_core) A.kv_h = cx.tensor_h(N, 2 * cb, Z, g.Sc);
    else A.kv = cx.tensor(N, 2 * C, Z, S);
  } else {
    A.mod = cx.tensor(N, 7 * C, Z, g.Sc);
    A.kv = cx.tensor(N, 2 * C, Z, g.Sc);
  }
  return A;
}

// computes them from cond; cond_act (fp32): SiLU(cond) where the pyramid has it and the cond is not re-tiled.  Scratch is released.
static void attn_cond_run(Ctx& cx, const AttnW& w, const AttnCond& A, int N, int Z, int S, const Src& cond, int per_image,
                          const TV* cond_act) {
  const size_t mark = cx.top;
  const AttnGeom g = attn_geom(cx.m, w, Z, S);
  const int C = w.C, cb = C / 8, Sc = g.Sc;
  // SiLU(cond), through the collage remap and at half resolution where the geometry says so
  PrepLaunch P = cx.prep(N, Z, Sc, per_image);
  cx.stream_src(P, cond.t, cond.collage);
  P.resample = g.half ? RS_PICK2 : RS_SAME; P.act = 1;
  if (cx.h16()) {
    // bf16 operands for every Linear (fp32 accumulate).  Activations that only feed a Linear, and the 7C modulation tensor
    // (shift/scale/gate/cross-cond chunks), are produced directly in bf16: the cross-cond chunk is the kv Linear's input as
    // it stands.
    TVH cact = cx.tensor_h(N, pair_cb((w.G + 7) / 8), Z, Sc);
    prep_out_h(P, cact, cond.t.Cb);
    cx.run(P);
    ConvLaunchH La = conv_h(cact, w.adah, w.ada, cb8_view(nullptr, N, 7 * C, Z, Sc, Sc));
    out_h(La, A.mod_h);
    run_conv1_h(cx, La);
    ConvLaunchH Lk = conv_h(A.mod_h.blocks(3 * cb, cb), w.kvh, w.kv, A.kv);
    if (g.mfma_core) {                                   // k, v leave their Linear as 16-bit (the attention core's MFMA operands)
      Lk.y = cb8_view(nullptr, N, 2 * C, Z, Sc, Sc);
      out_h(Lk, A.kv_h);
    }
    run_conv1_h(cx, Lk);
    cx.top = mark;
    return;
  }
  TV cact = (cond_act && !g.half) ? *cond_act : cx.tensor(N, (w.G + 7) / 8 * 8, Z, Sc);
  if (g.half || !cond_act) {
    prep_out(P, cact);
    cx.run(P);
  }
  run_conv(cx, conv(cact, w.ada, A.mod));
  run_conv(cx, conv(A.mod.blocks(3 * cb, cb), w.kv, A.kv));
  cx.top = mark;
}

// AttnBlock._forward with cond (model/MBAblocks.py:484-489); x updated in place.  pre: the conditioning side computed
// before (attn_cond_stage) for this block at this geometry; otherwise it is computed here, in the workspace.
static void attn_block(Ctx& cx, const AttnW& w, TV x, const Src& cond, int per_image, const TV* cond_act = nullptr,
                       const AttnCond* pre = nullptr) {
  const size_t mark = cx.top;
  const int N = x.N, Z = x.Z, S = x.H, C = w.C, cb = C / 8;
  const AttnGeom g = attn_geom(cx.m, w, Z, S);
  const bool half = g.half;
  AttnCond loc;
  if (!pre) {
    loc = attn_cond_alloc(cx, w, N, Z, S);
    attn_cond_run(cx, w, loc, N, Z, S, cond, per_image, cond_act);
    pre = &loc;
  }
  if (cx.h16()) {
    const bool f16 = cx.m->cfg.dtype == TM_DTYPE_F16;
    // The residual stream x, q/k/v and the softmax stay fp32; the Linears take 16-bit operands (see attn_cond_run).
    const TVH mod = pre->mod_h;
    // chunk order (MBAblocks.py:487): shift_msa, scale_msa, gate_msa, crss_cnd, shift_mlp, scale_mlp, gate_mlp
    TVH sh_a = mod.blocks(0 * cb, cb), sc_a = mod.blocks(1 * cb, cb), g_a = mod.blocks(2 * cb, cb);
    TVH sh_m = mod.blocks(4 * cb, cb), sc_m = mod.blocks(5 * cb, cb), g_m = mod.blocks(6 * cb, cb);
    TVH xa = cx.tensor_h(N, cb, Z, S), oh = cx.tensor_h(N, cb, Z, S);
    auto modulate = [&](const float* nw, const TVH& sc, const TVH& sh) {      // xa <- norm(x) (1 + scale) + shift
      PrepLaunch P = cx.prep(N, Z, S, per_image);
      prep_src(P, as_h(x));
      prep_norm(P, nw, C);
      prep_mod_voxel(P, sc, sh, half);
      prep_out_h(P, xa, x.Cb);
      cx.run(P);
    };
    modulate(w.n1, sc_a, sh_a);
    if (g.mfma_core) {
      // q leaves its Linear as 16-bit like k, v (the attention core's MFMA operands); softmax and accumulation are fp32
      TVH q = cx.tensor_h(N, cb, Z, S);
      const TVH kv = pre->kv_h;
      ConvLaunchH Lq = conv_h(xa, w.qh, w.q, cb8_view(nullptr, N, C, Z, S, S));
      out_h(Lq, q);
      run_conv1_h(cx, Lq);
      if (!cx.dry) cx.check((f16 ? launch_window_attn_f16 : launch_window_attn_bf16)(q, kv.blocks(0, cb), kv.blocks(cb, cb), w.qn, w.kn, oh, cx.s));
    } else {
      // other window sizes (z_size 1 / 4 / 8, patch_size 128): fp32 q / k / v into the generic fp32 attention core, its
      // output rounded to the 16-bit type for proj
      TV q = cx.tensor(N, C, Z, S), o = cx.tensor(N, C, Z, S);
      const TV kv = pre->kv;
      run_conv1_h(cx, conv_h(xa, w.qh, w.q, q));
      if (!cx.dry) cx.check(launch_window_attn(q, kv.blocks(0, cb), kv.blocks(cb, cb), w.qn, w.kn, o, cx.s));
      PrepLaunch P = cx.prep(N, Z, S, per_image);
      prep_src(P, o);
      prep_out_h(P, oh, o.Cb);
      cx.run(P);
    }
    // x <- x + gate * Linear(.): the 16-bit stream tensor is updated in place (each element is read and written by one lane)
    const TVH xh = as_h(x);
    auto gated = [&](const TVH& in, const uint16_t* wh, const ConvW& cw, const TVH& gate) {
      ConvLaunchH L = conv_h(in, wh, cw, x);
      out_h(L, xh);
      L.res_h = &xh; L.gate_h = &gate; L.gate_half = half ? 1 : 0;
      run_conv1_h(cx, L);
    };
    gated(oh, w.projh, w.proj, g_a);
    modulate(w.n2, sc_m, sh_m);
    TVH h1 = cx.tensor_h(N, 4 * cb, Z, S);
    ConvLaunchH L1 = conv_h(xa, w.fc1h, w.fc1, cb8_view(nullptr, N, 4 * C, Z, S, S));
    L1.flags = EPI_GELU;
    out_h(L1, h1);
    run_conv1_h(cx, L1);
    gated(h1, w.fc2h, w.fc2, g_m);
    cx.top = mark;
    return;
  }
  // fp32: the same structure
  const TV mod = pre->mod, kv = pre->kv;
  // chunk order (MBAblocks.py:487): shift_msa, scale_msa, gate_msa, crss_cnd, shift_mlp, scale_mlp, gate_mlp
  TV sh_a = mod.blocks(0 * cb, cb), sc_a = mod.blocks(1 * cb, cb), g_a = mod.blocks(2 * cb, cb);
  TV sh_m = mod.blocks(4 * cb, cb), sc_m = mod.blocks(5 * cb, cb), g_m = mod.blocks(6 * cb, cb);
  TV xa = cx.tensor(N, C, Z, S);
  auto modulate = [&](const float* nw, const TV& sc, const TV& sh) {          // xa <- norm(x) (1 + scale) + shift
    PrepLaunch P = cx.prep(N, Z, S, per_image);
    prep_src(P, x);
    prep_norm(P, nw, C);
    prep_mod_voxel(P, sc, sh, half);
    prep_out(P, xa);
    cx.run(P);
  };
  auto gated = [&](const TV& in, const ConvW& cw, const TV& gate) {          // x <- x + gate * Linear(in)
    ConvLaunch L = conv(in, cw, x);
    L.res = &x; L.gate = &gate; L.gate_half = half ? 1 : 0;
    run_conv(cx, L);
  };
  modulate(w.n1, sc_a, sh_a);
  TV q = cx.tensor(N, C, Z, S), o = cx.tensor(N, C, Z, S);
  run_conv(cx, conv(xa, w.q, q));
  if (!cx.dry) cx.check(launch_window_attn(q, kv.blocks(0, cb), kv.blocks(cb, cb), w.qn, w.kn, o, cx.s));
  gated(o, w.proj, g_a);
  modulate(w.n2, sc_m, sh_m);
  TV h1 = cx.tensor(N, 4 * C, Z, S);
  ConvLaunch L1 = conv(xa, w.fc1, h1);
  L1.flags = EPI_GELU;
  run_conv(cx, L1);
  gated(h1, w.fc2, g_m);
  cx.top = mark;
}

static void run_direct(Ctx& cx, const DirectW& w, const float* x, Acc5 ax, float* y, Acc5 ay, int N, int Zin, int Zout,
                       int S, int pz, int silu_in, int up2) {
  if (cx.dry) return;
  DirectLaunch L;
  L.x = x; L.ax = ax; L.y = y; L.ay = ay; L.w = w.w; L.bias = w.bias;
  L.N = N; L.Cin = w.Cin; L.Cout = w.Cout; L.Zin = Zin; L.Zout = Zout; L.S = S;
  L.kz = w.kz; L.ky = w.ky; L.kx = w.kx; L.pz = pz; L.py = 1; L.px = 1;
  L.silu_in = silu_in; L.up2_out = up2;
  cx.check(launch_conv_direct(L, cx.s));
}

// The RNA conditioning of a call (get_rna, model/unet_ours.py:298-323): four pyramid levels (stream tensors: fp32, or 16-bit
// in the 16-bit modes) and, in fp32 mode, SiLU(level) of the first three (pyramid conv input and adaLN input of the
// non-re-tiled AttnBlocks).  It depends on the genes only, not on t or x: a sampler that runs many steps on the same genes
// (mode A, LitModel.gen_sample) computes it once (tm_rna_pyramid) and hands it to every step (tm_unet_forward_rna).
// ac: the conditioning side of the AttnBlocks of the encoder, the middle and the collage decoder, by index into
// tm_model::attn (attn_cond_stage); empty where the caller computes it inside each block.
struct RnaOut { TV rl[4]; TV rs[3]; std::vector<AttnCond> ac; };

// Allocates the persistent outputs FIRST (so that their layout inside a caller-provided pyramid buffer is a pure function
// of (b, p1, p2)), computes them, and releases the scratch.  rna == nullptr: layout only.
// l0_in: level 0 (gene attention -> down_z -> Upsample, the part that reads the gene counts) was computed before
// (tm_rna_level0) and is taken from that buffer -- a tile sweep recomputes the conditioning of the SAME genes at every diffusion
// step (test_brn.py:232-255), and level 0 is both its costly part and small enough to keep (59 KB per patch).
// l0_out: compute level 0 only, into that buffer.
static void rna_stage(Ctx& cx, const float* rna, RnaOut& R, const void* l0_in = nullptr, void* l0_out = nullptr) {
  tm_model* m = cx.m;
  const tm_config& c = m->cfg;
  const int Z = m->z, Ne = cx.Ne;
  const bool h16 = cx.h16(), run = !cx.dry && (rna != nullptr || l0_in != nullptr);
  const bool head = l0_in == nullptr;                            // gene attention + down_z run in this call
  int S = m->gn * 2;
  for (int i = 0; i < 4; ++i) { R.rl[i] = cx.tensor_s(Ne, m->rw[i], Z, S); S *= 2; }
  if (l0_in) R.rl[0].p = (float*)const_cast<void*>(l0_in);
  if (l0_out) R.rl[0].p = (float*)l0_out;
  S = m->gn * 2;
  if (!h16) for (int i = 0; i < 3; ++i) { R.rs[i] = cx.tensor(Ne, m->rw[i], Z, S); S *= 2; }
  const size_t rna_mark = cx.top;
  TV tok = cx.tensor(Ne, c.rna_num, c.rna_slc, m->gn);           // gene-attention output, CB8 [Ne][Gb][zs][gn][gn][8]
  if (run && head) {
    cx.check(hipMemsetAsync(tok.p, 0, (size_t)Ne * tok.nstride * sizeof(float), cx.s));      // pad gene slots
    if (m->gene_mfma)
      cx.check(launch_gene_attn(rna, Ne, m->gn, c.rna_slc, c.rna_num, m->gene, tok.p, nullptr, 0, c.rna_slc, cx.s));
  }
  if (!m->gene_mfma) {
    const size_t mark = cx.top;
    float* gws = cx.alloc_f((size_t)Ne * gene_generic_split(Ne) * gene_generic_ws_floats(c.rna_num, m->D));
    if (run && head)
      cx.check(launch_gene_attn_generic(rna, Ne, m->gn, c.rna_slc, c.rna_num, m->D, m->gene, m->gene_idx, tok.p, nullptr, 0,
                                        c.rna_slc, gws, cx.s));
    cx.top = mark;                                               // scratch only (the stream orders its reuse)
  }
  const bool was_dry = cx.dry;
  cx.dry = !run;
  auto down_z = [&](const TV& y) {                               // down_z + Upsample into fp32 y
    if (m->downz_mfma) {
      ConvLaunch L = conv(tok, m->downz, y);
      L.flags = EPI_UP2; L.zmode = ZM_VALID;
      run_conv(cx, L);
    } else {
      // generic (kz, gn): direct conv straight from / to the CB8 tensors, nearest x2 fused into the store
      const Acc5 ax = acc_cb8(tok), ay = acc_cb8(y);
      if (run) cx.check(hipMemsetAsync(y.p, 0, (size_t)Ne * y.nstride * sizeof(float), cx.s));           // pad channels
      run_direct(cx, m->downz_d, tok.p, ax, y.p, ay, Ne, c.rna_slc, Z, m->gn, 0, 0, 1);
    }
  };
  if (h16) {
    // 16-bit modes: gene attention and down_z stay fp32 (they read the fp32 gene counts; < 0.3 % of the FLOPs), level 0
    // enters the 16-bit stream behind down_z, and the three SiLU -> Conv3d(1,3,3) -> Upsample stages
    // (model/unet_ours.py:290-295) run as 16-bit convs like every other conv under the reference's autocast: the in-plane
    // conv is the 3x3x3 kernel on weights whose z - 1 / z + 1 slices are zero, its output leaves at the conv's resolution
    // and ONE pass of the block-input kernel writes both the x2 level (raw copy) and SiLU of it (the next conv's input).
    int S0 = m->gn * 2;
    TV rl0 = cx.tensor(Ne, m->rw[0], Z, S0);
    if (head) {
      down_z(rl0);
      PrepLaunch P = cx.prep(Ne, Z, S0);                           // fp32 level 0 -> the 16-bit stream tensor
      prep_src(P, rl0);
      prep_out_h(P, as_h(R.rl[0]), rl0.Cb);
      cx.run(P);
    }
    if (l0_out) { cx.dry = was_dry; cx.top = rna_mark; return; }
    auto silu_pair = [&](const TV& lvl, int Sl, const TVH& dst) {  // SiLU(level), pair-padded: the next conv's input
      PrepLaunch Q = cx.prep(Ne, Z, Sl);
      prep_src(Q, as_h(lvl));
      Q.act = 1;
      prep_out_h(Q, dst, lvl.Cb);
      cx.run(Q);
    };
    TVH act = cx.tensor_h(Ne, pair_cb(rl0.Cb), Z, S0);
    silu_pair(R.rl[0], S0, act);
    int S = S0;
    for (int i = 1; i < 4; ++i) {
      TV y = cx.tensor_s(Ne, m->rw[i], Z, S);                      // conv output at the conv's resolution (16-bit)
      ConvLaunchH L = conv_h(act, m->pyrh[i - 1], m->pyr16[i - 1], y);
      out_h(L, as_h(y));
      run_conv27_h(cx, L, m->pyr16[i - 1], 0);
      S *= 2;
      TVH nxt;
      if (i < 3) nxt = cx.tensor_h(Ne, pair_cb(R.rl[i].Cb), Z, S);
      PrepLaunch U = cx.prep(Ne, Z, S);                            // Upsample: level i (raw) and SiLU(level i)
      prep_src(U, as_h(y));
      U.resample = RS_UP2;
      if (i < 3 && nxt.Cb == R.rl[i].Cb) {
        U.act = 1;
        prep_out_h(U, nxt, y.Cb);
        prep_raw_h(U, as_h(R.rl[i]));
        cx.run(U);
      } else {
        prep_out_h(U, as_h(R.rl[i]), y.Cb);
        cx.run(U);
        if (i < 3) silu_pair(R.rl[i], S, nxt);                     // odd block count: the pair-padded SiLU copy on its own
      }
      act = nxt;
    }
    cx.dry = was_dry;
    cx.top = rna_mark;
    return;
  }
  TV* rl = R.rl;
  TV* rs = R.rs;
  if (head) down_z(rl[0]);
  if (l0_out) { cx.dry = was_dry; cx.top = rna_mark; return; }
  for (int i = 1; i < 4; ++i) {
    PrepLaunch P = cx.prep(Ne, Z, rl[i - 1].H);
    prep_src(P, rl[i - 1]);
    P.act = 1;
    prep_out(P, rs[i - 1]);
    cx.run(P);
    ConvLaunch L = conv(rs[i - 1], m->pyr[i - 1], rl[i]);          // SiLU -> conv -> Upsample
    L.flags = EPI_UP2; L.zmode = ZM_INPLANE;
    run_conv(cx, L);
  }
  cx.dry = was_dry;
  cx.top = rna_mark;                                              // tok / fp32 scratch are dead (the stream orders reuse)
}

// The step-invariant part of the AttnBlocks behind the levels of a pyramid buffer: mod and kv (attn_cond_alloc) of every
// AttnBlock of the encoder, the middle and the `pred` decoder, each with the geometry it has there (encoder / middle: Ne
// patches of the encoder grid; decoder: Nd patches, cond through the collage remap).  Called with cx.top behind the levels
// (rna_stage has released its scratch): all persistent tensors first, so that the layout is a pure function of
// (b, p1, p2), then one block after the other with its scratch.  run == false: layout only.  The `pred2` decoder pass is
// not covered (another geometry of the same blocks, and not on the sampler's path): it computes its own in-step.
static void attn_cond_stage(Ctx& cx, RnaOut& R, bool run) {
  tm_model* m = cx.m;
  const int Z = m->z, L = m->L, ps = m->cfg.patch_size;
  const int ne_img = cx.p1 * cx.p2, nd_img = (cx.p1 - 1) * (cx.p2 - 1);
  const bool h16 = is_h16(m->cfg.dtype);
  struct Site { int idx, lvl; bool col; };
  std::vector<Site> sites;
  for (const EncEntry& e : m->enc)
    for (const Op& op : e.ops) if (op.kind == 1) sites.push_back({op.idx, e.lvl, false});
  sites.push_back({m->mid[1].idx, L - 1, false});
  for (const DecEntry& e : m->dec)
    for (const Op& op : e.ops) if (op.kind == 1) sites.push_back({op.idx, e.lvl, true});
  R.ac.assign(m->attn.size(), AttnCond());
  for (const Site& st : sites) R.ac[st.idx] = attn_cond_alloc(cx, m->attn[st.idx], st.col ? cx.Nd : cx.Ne, Z, ps >> st.lvl);
  const size_t mark = cx.top;
  const bool was_dry = cx.dry;
  cx.dry = was_dry || !run;
  for (const Site& st : sites) {
    const int ri = L - 1 - st.lvl;
    attn_cond_run(cx, m->attn[st.idx], R.ac[st.idx], st.col ? cx.Nd : cx.Ne, Z, ps >> st.lvl, {R.rl[ri], st.col},
                  st.col ? nd_img : ne_img, (!st.col && !h16 && ri < 3) ? &R.rs[ri] : nullptr);
  }
  cx.dry = was_dry;
  cx.top = mark;
}

// rna != nullptr: compute the conditioning inside this call's workspace; otherwise R_in (tm_rna_pyramid) is used
static int forward_impl(Ctx& cx, const float* x, const int64_t* t, const float* rna, const RnaOut* R_in, float* pred,
                        float* pred2, const void* l0_in = nullptr) {
  tm_model* m = cx.m;
  const tm_config& c = m->cfg;
  const int Z = m->z, L = m->L, ps = c.patch_size, Ne = cx.Ne, Nd = cx.Nd, b = cx.b;
  const int ne_img = cx.p1 * cx.p2, nd_img = (cx.p1 - 1) * (cx.p2 - 1);
  const bool h16 = is_h16(c.dtype);
  // ---- time embedding + all emb_layers ----
  float* te = cx.alloc_f((size_t)2 * b * c.embed_ch);       // te, then SiLU(te)
  float* te_act = te + (size_t)b * c.embed_ch;
  float* ss = cx.alloc_f((size_t)b * m->emb_tot);
  cx.ss = ss;
  if (!cx.dry) {
    cx.check(launch_time_embed(t, b, c.net_ch, c.embed_ch, m->te_w1, m->te_b1, m->te_w2, m->te_b2, te, te_act, cx.s));
    cx.check(launch_emb_all(te_act, b, c.embed_ch, m->emb_w, m->emb_b, m->emb_tot, ss, cx.s));
  }
  // ---- RNA pyramid ----
  RnaOut Rloc;
  if (!R_in) { rna_stage(cx, rna, Rloc, l0_in); R_in = &Rloc; }
  TV rl[4], rs[3];
  for (int i = 0; i < 4; ++i) rl[i] = R_in->rl[i];
  for (int i = 0; i < 3; ++i) rs[i] = R_in->rs[i];
  auto pre = [&](int idx) -> const AttnCond* { return R_in->ac.empty() ? nullptr : &R_in->ac[idx]; };
  for (int i = 0; i < 4; ++i) { TV v = rl[i]; v.C = m->rw[i]; dump_tv(cx, "rna." + std::to_string(i), v); }
  // ---- stem ----
  std::vector<std::vector<TV>> skips(L);
  TV h = cx.tensor_s(Ne, c.net_ch, Z, ps);
  if (!cx.dry) cx.check(launch_stem(x, h, m->stem.w, m->stem.bias, c.n_stain, cx.s, h16 ? (uint16_t*)h.p : nullptr, h.nstride,
                                    c.dtype == TM_DTYPE_F16));
  skips[0].push_back(h);
  dump_tv(cx, "stem", h);
  // ---- encoder ----
  for (const EncEntry& e : m->enc) {
    const TV& cond = rl[L - 1 - e.lvl];
    const int So = ps >> e.lvl;
    std::vector<Src> src;
    src.push_back({h, false});
    if (e.cat) src.push_back({cond, false});
    for (const Op& op : e.ops) {
      if (op.kind == 0) h = res_block(cx, m->res[op.idx], src, Ne, ne_img, So, op.mode, nullptr);
      else attn_block(cx, m->attn[op.idx], h, {cond, false}, ne_img, (L - 1 - e.lvl) < 3 ? &rs[L - 1 - e.lvl] : nullptr, pre(op.idx));
    }
    skips[e.lvl].push_back(h);
    const Op& last = e.ops.back();
    dump_tv(cx, last.kind == 0 ? m->res[last.idx].pfx : m->attn[last.idx].pfx, h);
  }
  // ---- middle ----
  {
    std::vector<Src> src = {{h, false}, {rl[0], false}};
    const int So = ps >> (L - 1);
    h = res_block(cx, m->res[m->mid[0].idx], src, Ne, ne_img, So, RS_SAME, nullptr);
    attn_block(cx, m->attn[m->mid[1].idx], h, {rl[0], false}, ne_img, &rs[0], pre(m->mid[1].idx));
    std::vector<Src> src2 = {{h, false}};
    h = res_block(cx, m->res[m->mid[2].idx], src2, Ne, ne_img, So, RS_SAME, nullptr);
    dump_tv(cx, "middle_block", h);
  }
  // ---- decoder(s) ----
  auto decode = [&](bool col, float* outp) {
    const size_t mark = cx.top;
    const int N = col ? Nd : Ne, per = col ? nd_img : ne_img;
    std::vector<std::vector<TV>> st = skips;
    TV hd = h;
    bool hd_col = col;                 // only the middle output still lives on the encoder grid
    for (const DecEntry& e : m->dec) {
      const int So = ps >> e.lvl;
      Src cond = {rl[L - 1 - e.lvl], col};
      std::vector<Src> src = {{hd, hd_col}, {st[e.lvl].back(), col}, cond};
      st[e.lvl].pop_back();
      for (const Op& op : e.ops) {
        if (op.kind == 0) {
          if (op.mode == RS_SAME) hd = res_block(cx, m->res[op.idx], src, N, per, So, RS_SAME, nullptr);
          else { std::vector<Src> s1 = {{hd, false}}; hd = res_block(cx, m->res[op.idx], s1, N, per, So * 2, RS_UP2, nullptr); }
        } else attn_block(cx, m->attn[op.idx], hd, cond, per, nullptr, col ? pre(op.idx) : nullptr);
      }
      hd_col = false;
      if (col) { const std::string& p0 = m->res[e.ops[0].idx].pfx; dump_tv(cx, p0.substr(0, p0.size() - 2), hd); }
    }
    // head: RMSNorm -> SiLU -> Conv3d(1,3,3) -> 'b s z h w -> b (s z) h w'  (unet_ours.py:271-275,423-424)
    // (16-bit modes: the normalised, activated tensor is a 16-bit tensor like every other conv input)
    TV A = cx.tensor_s(N, c.net_ch, Z, ps);
    PrepLaunch P = cx.prep(N, Z, ps, per);
    cx.stream_src(P, hd);
    prep_norm(P, m->out_norm, c.net_ch);
    P.act = 1;
    if (h16) prep_out_h(P, as_h(A), A.Cb);
    else prep_out(P, A);
    cx.run(P);
    if (!cx.dry) cx.check(launch_head(A, outp, m->head.w, m->head.bias, c.n_stain, cx.s, h16 ? (c.dtype == TM_DTYPE_F16 ? 2 : 1) : 0));
    cx.top = mark;
  };
  decode(true, pred);
  if (pred2) decode(false, pred2);
  return TM_OK;
}

static int check_fwd_args(const tm_model* m, int b, int p1, int p2) {
  if (!m) return fail(TM_ERR_ARG, "null model");
  if (!m->finalized) return fail(TM_ERR_STATE, "tm_model_finalize has not been called");
  if (m->cfg.vis_only) return fail(TM_ERR_STATE, "attention-map model has no UNet forward");
  if (b < 1 || p1 < 2 || p2 < 2) return fail(TM_ERR_ARG, "need b >= 1 and p1, p2 >= 2 (got %d, %d, %d)", b, p1, p2);
  return TM_OK;
}

extern "C" size_t tm_workspace_bytes(const tm_model* m, int b, int p1, int p2, int want_pred2) {
  if (check_fwd_args(m, b, p1, p2) != TM_OK) return 0;
  Ctx cx;
  cx.init(const_cast<tm_model*>(m), b, p1, p2, nullptr, 0, nullptr);
  forward_impl(cx, nullptr, nullptr, nullptr, nullptr, (float*)256, want_pred2 ? (float*)256 : nullptr);
  return cx.peak + 256;
}
// tm_workspace_bytes is an upper bound for every forward entry point (it includes the RNA scratch)
static int check_workspace(const tm_model* m, int b, int p1, int p2, bool want_pred2, size_t workspace_bytes) {
  const size_t need = tm_workspace_bytes(m, b, p1, p2, want_pred2);
  if (workspace_bytes < need) return fail(TM_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, need);
  return TM_OK;
}
// the shared tail of the entry points: the first launch error of the call, if any
static int fwd_status(const Ctx& cx) {
  if (cx.err != hipSuccess) return fail(TM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(cx.err));
  return TM_OK;
}

extern "C" int tm_unet_forward(tm_model* m, const void* x, const int64_t* t, const void* rna_dense, int b, int p1,
                               int p2, void* pred, void* pred2_or_null, void* workspace, size_t workspace_bytes,
                               void* stream) {
  int rc = check_fwd_args(m, b, p1, p2);
  if (rc != TM_OK) return rc;
  if (!x || !t || !rna_dense || !pred || !workspace) return fail(TM_ERR_ARG, "null tensor argument");
  if ((rc = check_workspace(m, b, p1, p2, pred2_or_null != nullptr, workspace_bytes)) != TM_OK) return rc;
  Ctx cx;
  cx.init(m, b, p1, p2, workspace, workspace_bytes, (hipStream_t)stream);
  forward_impl(cx, (const float*)x, t, (const float*)rna_dense, nullptr, (float*)pred, (float*)pred2_or_null);
  return fwd_status(cx);
}

// ---- RNA conditioning computed once for many steps (mode A: the genes do not change over the reverse loop) ----
extern "C" size_t tm_rna_pyramid_bytes(const tm_model* m, int b, int p1, int p2) {
  if (check_fwd_args(m, b, p1, p2) != TM_OK) return 0;
  Ctx cx;
  cx.init(const_cast<tm_model*>(m), b, p1, p2, nullptr, 0, nullptr);
  RnaOut R;
  rna_stage(cx, nullptr, R);
  attn_cond_stage(cx, R, false);
  return cx.peak + 512;
}
extern "C" int tm_rna_pyramid(tm_model* m, const void* rna_dense, int b, int p1, int p2, void* pyramid, size_t pyramid_bytes,
                              void* stream) {
  int rc = check_fwd_args(m, b, p1, p2);
  if (rc != TM_OK) return rc;
  if (!rna_dense || !pyramid) return fail(TM_ERR_ARG, "null tensor argument");
  const size_t need = tm_rna_pyramid_bytes(m, b, p1, p2);
  if (pyramid_bytes < need) return fail(TM_ERR_WORKSPACE, "pyramid buffer %zu B < required %zu B", pyramid_bytes, need);
  Ctx cx;
  cx.init(m, b, p1, p2, pyramid, pyramid_bytes, (hipStream_t)stream);
  RnaOut R;
  rna_stage(cx, (const float*)rna_dense, R);
  attn_cond_stage(cx, R, true);
  return fwd_status(cx);
}
// ---- level 0 of the RNA conditioning on its own (the sweep's per-window cache) ----
extern "C" size_t tm_rna_level0_bytes(const tm_model* m, int b, int p1, int p2) {
  if (check_fwd_args(m, b, p1, p2) != TM_OK) return 0;
  const TV t = cb8_view(nullptr, b * p1 * p2, m->rw[0], m->z, m->gn * 2, m->gn * 2);
  return (size_t)t.N * t.nstride * (is_h16(m->cfg.dtype) ? 2 : 4);
}
// the level-0 buffer of a call: aligned for the kernels' 16-byte accesses and large enough for (b, p1, p2)
static int check_level0(const tm_model* m, int b, int p1, int p2, const void* level0, size_t level0_bytes) {
  if (((uintptr_t)level0 & 15) != 0) return fail(TM_ERR_ARG, "level0 buffer must be 16-byte aligned");
  if (level0_bytes < tm_rna_level0_bytes(m, b, p1, p2)) return fail(TM_ERR_WORKSPACE, "level-0 buffer too small for (b, p1, p2)");
  return TM_OK;
}
extern "C" int tm_rna_level0(tm_model* m, const void* rna_dense, int b, int p1, int p2, void* level0, size_t level0_bytes,
                             void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_fwd_args(m, b, p1, p2);
  if (rc != TM_OK) return rc;
  if (!rna_dense || !level0 || !workspace) return fail(TM_ERR_ARG, "null tensor argument");
  if ((rc = check_level0(m, b, p1, p2, level0, level0_bytes)) != TM_OK) return rc;
  if ((rc = check_workspace(m, b, p1, p2, false, workspace_bytes)) != TM_OK) return rc;
  Ctx cx;
  cx.init(m, b, p1, p2, workspace, workspace_bytes, (hipStream_t)stream);
  RnaOut R;
  rna_stage(cx, (const float*)rna_dense, R, nullptr, level0);
  return fwd_status(cx);
}
extern "C" int tm_unet_forward_level0(tm_model* m, const void* x, const int64_t* t, const void* level0, size_t level0_bytes,
                                      int b, int p1, int p2, void* pred, void* pred2_or_null, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  int rc = check_fwd_args(m, b, p1, p2);
  if (rc != TM_OK) return rc;
  if (!x || !t || !level0 || !pred || !workspace) return fail(TM_ERR_ARG, "null tensor argument");
  if ((rc = check_level0(m, b, p1, p2, level0, level0_bytes)) != TM_OK) return rc;
  if ((rc = check_workspace(m, b, p1, p2, pred2_or_null != nullptr, workspace_bytes)) != TM_OK) return rc;
  Ctx cx;
  cx.init(m, b, p1, p2, workspace, workspace_bytes, (hipStream_t)stream);
  forward_impl(cx, (const float*)x, t, nullptr, nullptr, (float*)pred, (float*)pred2_or_null, level0);
  return fwd_status(cx);
}
extern "C" int tm_unet_forward_rna(tm_model* m, const void* x, const int64_t* t, const void* pyramid, size_t pyramid_bytes,
                                   int b, int p1, int p2, void* pred, void* pred2_or_null, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  int rc = check_fwd_args(m, b, p1, p2);
  if (rc != TM_OK) return rc;
  if (!x || !t || !pyramid || !pred || !workspace) return fail(TM_ERR_ARG, "null tensor argument");
  if (pyramid_bytes < tm_rna_pyramid_bytes(m, b, p1, p2)) return fail(TM_ERR_WORKSPACE, "pyramid buffer too small for (b, p1, p2)");
  if ((rc = check_workspace(m, b, p1, p2, pred2_or_null != nullptr, workspace_bytes)) != TM_OK) return rc;
  // the layout of the persistent tensors inside the pyramid buffer is a pure function of (b, p1, p2): replay it
  Ctx px;
  px.init(m, b, p1, p2, const_cast<void*>(pyramid), pyramid_bytes, (hipStream_t)stream);
  RnaOut R;
  rna_stage(px, nullptr, R);
  attn_cond_stage(px, R, false);
  Ctx cx;
  cx.init(m, b, p1, p2, workspace, workspace_bytes, (hipStream_t)stream);
  forward_impl(cx, (const float*)x, t, nullptr, &R, (float*)pred, (float*)pred2_or_null);
  return fwd_status(cx);
}

// ------------------------------------------------------------------------------------------
extern "C" int tm_sampler_step(const tm_step_coefs* c, const void* x_patches, const void* eps, const void* noise,
                               void* x_prev_img, int b, int P1, int P2, int C, int ps, int mode, void* stream) {
  if (!c || !x_patches || !eps || !x_prev_img) return fail(TM_ERR_ARG, "null argument");
  if (b < 1 || P1 < 1 || P2 < 1 || C < 1 || ps < 2 || (ps & 1)) return fail(TM_ERR_ARG, "bad geometry");
  if (mode != TM_SAMPLE_DDPM && mode != TM_SAMPLE_DDIM) return fail(TM_ERR_ARG, "mode must be DDPM or DDIM");
  StepCoefs k = {c->sqrt_recip_alphas_cumprod, c->sqrt_recipm1_alphas_cumprod, c->posterior_mean_coef1,
                 c->posterior_mean_coef2, c->sigma, c->sqrt_alpha_bar_prev, c->sqrt_one_minus_alpha_bar_prev};
  HIP_TRY(launch_sampler_step(k, (const float*)x_patches, (const float*)eps, (const float*)noise, (float*)x_prev_img,
                              b, P1, P2, C, ps, mode, (hipStream_t)stream));
  return TM_OK;
}

extern "C" int tm_pad_patchify(const void* img, void* patches, int b, int C, int P1, int P2, int ps, float pad,
                               void* stream) {
  if (!img || !patches || b < 1 || P1 < 1 || P2 < 1 || C < 1 || ps < 2 || (ps & 1)) return fail(TM_ERR_ARG, "bad argument");
  HIP_TRY(launch_pad_patchify((const float*)img, (float*)patches, b, C, P1, P2, ps, pad, (hipStream_t)stream));
  return TM_OK;
}

extern "C" size_t tm_gene_attn_workspace_bytes(const tm_model* m, int B) {
  if (!m || B < 1 || m->gene_mfma) return 256;
  return 256 + (size_t)B * gene_generic_split(B) * gene_generic_ws_floats(m->cfg.rna_num, m->D) * sizeof(float);
}

extern "C" int tm_gene_attn(tm_model* m, const void* rna_dense, int B, void* attn_out, void* rna_mid, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!m || !rna_dense || !attn_out || B < 1) return fail(TM_ERR_ARG, "bad argument");
  if (!m->finalized) return fail(TM_ERR_STATE, "tm_model_finalize has not been called");
  const tm_config& c = m->cfg;
  const int G = c.rna_num, zs = c.rna_slc;
  if (zs != 4) return fail(TM_ERR_ARG, "the attention-map read-out is defined for rna_slc = 4 (three slice pairs, model/unet_attn.py:162-172)");
  if (workspace_bytes < tm_gene_attn_workspace_bytes(m, B) || (!m->gene_mfma && !workspace))
    return fail(TM_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, tm_gene_attn_workspace_bytes(m, B));
  float* ao = (float*)attn_out;
  hipStream_t s = (hipStream_t)stream;
  // three slice-pair masks then the unmasked map (model/unet_attn.py:162-172)
  for (int i = 0; i < 4; ++i) {
    const int lo = (i < 3) ? i : 0, hi = (i < 3) ? i + 2 : zs;
    if (m->gene_mfma)
      HIP_TRY(launch_gene_attn((const float*)rna_dense, B, m->gn, zs, G, m->gene, nullptr, ao + (size_t)i * B * G * G, lo, hi, s));
    else
      HIP_TRY(launch_gene_attn_generic((const float*)rna_dense, B, m->gn, zs, G, m->D, m->gene, m->gene_idx, nullptr,
                                       ao + (size_t)i * B * G * G, lo, hi, (float*)workspace, s));
  }
  if (rna_mid) HIP_TRY(launch_rna_mid((const float*)rna_dense, B, m->gn, zs, G, (float*)rna_mid, s));
  return TM_OK;
}

extern "C" size_t tm_gene_attn_readout_workspace_bytes(const tm_model* m, int B, int K) {
  if (!m || B < 1 || m->gene_mfma) return 256;
  return 256 + gene_readout_ws_floats(B, m->cfg.rna_num, m->D) * sizeof(float);
}

int tmk::gene_readout_args(int zs, const int* glst, int K, int G) {
  if (zs != 4) return fail(TM_ERR_ARG, "the attention-map read-out is defined for rna_slc = 4 (three slice pairs, model/unet_attn.py:162-172)");
  if (K < 1 || K > 8) return fail(TM_ERR_ARG, "read-out gene list length K = %d outside [1, 8]", K);
  for (int k = 0; k < K; ++k) {
    if (glst[k] < 0 || glst[k] >= G) return fail(TM_ERR_ARG, "read-out gene index glst[%d] = %d outside [0, %d)", k, glst[k], G);
    for (int j = 0; j < k; ++j)
      if (glst[j] == glst[k]) return fail(TM_ERR_ARG, "read-out gene index %d is repeated (glst[%d] and glst[%d])", glst[k], j, k);
  }
  return TM_OK;
}

extern "C" int tm_gene_attn_readout(tm_model* m, const void* rna_dense, int B, const int* glst, int K, void* out, void* sub,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!m || !rna_dense || !glst || !out || B < 1) return fail(TM_ERR_ARG, "bad argument");
  if (!m->finalized) return fail(TM_ERR_STATE, "tm_model_finalize has not been called");
  const tm_config& c = m->cfg;
  const int G = c.rna_num, zs = c.rna_slc;
  if (int rc = gene_readout_args(zs, glst, K, G)) return rc;
  const size_t need = tm_gene_attn_readout_workspace_bytes(m, B, K);
  if (workspace_bytes < need || (!m->gene_mfma && !workspace)) return fail(TM_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, need);
  const float* rna = (const float*)rna_dense;
  hipStream_t s = (hipStream_t)stream;
  if (m->gene_mfma)
    HIP_TRY(launch_gene_readout(rna, B, m->gn, zs, G, m->gene, glst, K, (float*)out, (float*)sub, s));
  else
    HIP_TRY(launch_gene_readout_chunks(rna, B, m->gn, zs, G, m->D, m->gene, m->gene_idx, glst, K, (float*)out, (float*)sub,
                                       (float*)workspace, s));
  return TM_OK;
}
