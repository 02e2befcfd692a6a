// The forms of the fp32 MFMA conv (ConvForm, tm_kernels.h): which form a layer runs in, and the host packers of each.  Host only.
#include "tm_conv_frag.h"
#include "tm_kernels.h"

#include <stdlib.h>
#include <string.h>

#include <vector>

namespace tmk {

int conv_form_taps(int form) {
  switch (form) {
    case CF_1X1: return 1;
    case CF_INPLANE: return 9;
    case CF_ZSKIP_UPS: case CF_PAIR_UPS: return 12;
    case CF_XQUAD: return 54;
    default: return 27;
  }
}
static bool form_ups(int form) { return form == CF_ZSKIP_UPS || form == CF_PAIR_UPS; }
size_t conv_pack_floats(int form, int Cout, int Cbi) {
  return (size_t)(form_ups(form) ? 4 : 1) * ((Cout + 63) / 64) * Cbi * conv_form_taps(form) * 512;
}
ConvW conv_w(int form, int Cout, int Cbi) {
  ConvW cw;
  cw.form = form; cw.Cout = Cout; cw.Cbi = Cbi; cw.taps = conv_form_taps(form); cw.ntile = (Cout + 63) / 64;
  return cw;
}

static bool switch_on(const char* name) {        // an A/B switch: on unless the variable is set to 0
  const char* v = getenv(name);
  return !(v && atoi(v) == 0);
}
bool xquad_split_on() {
  static const bool on = switch_on("TM_CONV_XQUAD_SPLIT");
  return on;
}
int conv_pick_form(int ksize, int zmode, int Z, bool deep8, int role, bool* fuse_mid) {
  static const bool zpair_on = switch_on("TM_CONV_ZPAIR"), fuse_on = switch_on("TM_CONV_FUSE_MID"),
                    xquad_on = switch_on("TM_CONV_XQUAD");
  if (fuse_mid) *fuse_mid = false;
  if (ksize == 1) return CF_1X1;
  if (zmode == ZM_INPLANE) return CF_INPLANE;
  if (zmode == ZM_VALID) return CF_PLANES3;
  const bool pair = Z == 2 && zpair_on;
  if (zmode == ZM_UPS) return ((role & ROLE_OP_PAIR_UPS) || ((role & ROLE_RES) && pair)) ? CF_PAIR_UPS : CF_ZSKIP_UPS;
  if (Z != 2) return (Z == 1 && (role & ROLE_RES)) ? CF_INPLANE : CF_PLANES3;
  if ((role & ROLE_OP_XQUAD) && xquad_on) return CF_XQUAD;
  if (!pair) return CF_ZSKIP;
  // a ResBlock conv on planes of at least 8 x 8 runs in the x-quad form (F(4,3) along x, half the pair form's MFMAs);
  // TM_CONV_XQUAD=0 leaves it on the pair form.  The decoder blocks of the deepest level have too few workgroups for the chip
  // unless their K loop is split (xquad_ksplit): with TM_CONV_XQUAD_SPLIT=0 they stay on the pair form.  c1 of a 64-channel
  // block: the pair form fuses the mid norm into its epilogue; an x-quad workgroup holds 32 of the 64 channels and leaves the
  // norm to the separate pass
  const bool xq = (role & ROLE_RES) && !((role & ROLE_DEEP) && !xquad_split_on()) && deep8 && xquad_on;
  if (fuse_mid) *fuse_mid = (role & ROLE_C1_64) && fuse_on && !xq;
  return xq ? CF_XQUAD : CF_PAIR;
}

// ---- packers ----
static void seg_counts(const int* seg_c, int nseg, int& Cin, int& Cbi) {
  Cin = Cbi = 0;
  for (int s = 0; s < nseg; ++s) { Cin += seg_c[s]; Cbi += (seg_c[s] + 7) / 8; }
}
// w [Cout][Cin][taps] -> [n_tile][cblk][tap][64 cout][8 cin], pad slots zero.  HALVES (the forms that reach LDS by LDS-DMA: the
// pack is the LDS image): a tap is [2 k-halves][64 cout][4 cin] instead (conv_w_off, tm_conv_frag.h): the same floats permuted
static void pack_taps(const float* w, int Cout, const int* seg_c, int nseg, int taps, float* out, bool halves = false) {
  int Cin, Cbi;
  seg_counts(seg_c, nseg, Cin, Cbi);
  memset(out, 0, (size_t)((Cout + 63) / 64) * Cbi * taps * 512 * sizeof(float));
  int ci0 = 0, cb0 = 0;
  for (int s = 0; s < nseg; ++s) {
    for (int c = 0; c < seg_c[s]; ++c) {
      const int ci = ci0 + c;
      const int cb = cb0 + c / 8, c8 = c % 8;
      for (int co = 0; co < Cout; ++co) {
        const int nt = co / 64, col = co % 64;
        const float* src = w + ((size_t)co * Cin + ci) * taps;
        float* dst = out + (((size_t)nt * Cbi + cb) * taps) * 512 + (halves ? conv_w_off(col, c8) : col * 8 + c8);
        for (int t = 0; t < taps; ++t) dst[(size_t)t * 512] = src[t];
      }
    }
    ci0 += seg_c[s];
    cb0 += (seg_c[s] + 7) / 8;
  }
}

// The three weight transforms, each over n = Cout * Cin filters and all in fp32.
// Phase sums of the upsampled-input conv: for output phase (py, px) the 3 x 3 in-plane taps collapse onto a 2 x 2 window of the
// low-resolution input -- rows: py = 0: {ky 0} | {ky 1, 2}; py = 1: {ky 0, 1} | {ky 2}; columns alike.  [n][27] -> [n][kz][wy][wx]
static std::vector<float> phase_sums(const float* w, size_t n, int py, int px) {
  static const int G0[2][2][2] = {{{0, 0}, {1, 2}}, {{0, 1}, {2, 2}}};       // [phase bit][window pos] -> tap range [lo, hi]
  std::vector<float> o(n * 12);
  for (size_t i = 0; i < n; ++i)
    for (int kz = 0; kz < 3; ++kz)
      for (int wy = 0; wy < 2; ++wy)
        for (int wx = 0; wx < 2; ++wx) {
          float acc = 0.f;
          for (int ky = G0[py][wy][0]; ky <= G0[py][wy][1]; ++ky)
            for (int kx = G0[px][wx][0]; kx <= G0[px][wx][1]; ++kx) acc += w[i * 27 + kz * 9 + ky * 3 + kx];
          o[i * 12 + kz * 4 + wy * 2 + wx] = acc;
        }
  return o;
}
// z difference of the pair forms: the kz slices V0, V1, V2 of k in-plane taps each -> V1, V2 - V1, V0 - V1, the order the
// kernels consume the three products in.  [n][3][k] -> [n][3][k]
static std::vector<float> z_diff(const float* w, size_t n, int k) {
  std::vector<float> o(n * 3 * k);
  for (size_t i = 0; i < n; ++i)
    for (int t = 0; t < k; ++t) {
      const float w0 = w[i * 3 * k + t], w1 = w[i * 3 * k + k + t], w2 = w[i * 3 * k + 2 * k + t];
      o[i * 3 * k + t] = w1;
      o[i * 3 * k + k + t] = w2 - w1;
      o[i * 3 * k + 2 * k + t] = w0 - w1;
    }
  return o;
}
// F(4,3) filter transform of the three kx taps of every (product, ky) row: U0 = g0 / 4, U1 = -((g0 + g1) + g2) / 6,
// U2 = -((g0 - g1) + g2) / 6, U3 = (g0 / 24 + g1 / 12) + g2 / 6, U4 = (g0 / 24 - g1 / 12) + g2 / 6, U5 = g2.  Divisions, not
// rounded reciprocals: weights that are multiples of 24 transform exactly.  [n][9 rows][3] -> [n][9 rows][6]
static std::vector<float> f43_rows(const float* w, size_t n) {
  std::vector<float> o(n * 54);
  for (size_t r = 0; r < n * 9; ++r) {
    const float* g = w + r * 3;
    float* u = o.data() + r * 6;
    u[0] = g[0] / 4.f;
    u[1] = -((g[0] + g[1]) + g[2]) / 6.f;
    u[2] = -((g[0] - g[1]) + g[2]) / 6.f;
    u[3] = (g[0] / 24.f + g[1] / 12.f) + g[2] / 6.f;
    u[4] = (g[0] / 24.f - g[1] / 12.f) + g[2] / 6.f;
    u[5] = g[2];
  }
  return o;
}
// The x-quad pack: a workgroup of conv3d_xquad owns 32 couts, so the tiles are of 32 couts and a tap is [2 k-halves][32 cout][4 cin],
// one contiguous 1 KiB LDS-DMA piece: w [Cout][Cin][54] -> [ceil(Cout / 64) * 2 tiles][cblk][54 taps][256], pad slots zero
static void pack_taps32(const float* w, int Cout, const int* seg_c, int nseg, float* out) {
  int Cin, Cbi;
  seg_counts(seg_c, nseg, Cin, Cbi);
  memset(out, 0, conv_pack_floats(CF_XQUAD, Cout, Cbi) * sizeof(float));
  int ci0 = 0, cb0 = 0;
  for (int s = 0; s < nseg; ++s) {
    for (int c = 0; c < seg_c[s]; ++c) {
      const int ci = ci0 + c, cb = cb0 + c / 8, c8 = c % 8;
      for (int co = 0; co < Cout; ++co) {
        const float* src = w + ((size_t)co * Cin + ci) * 54;
        float* dst = out + (((size_t)(co / 32) * Cbi + cb) * 54) * 256 + conv_frag_off(co % 32, c8 >> 2, 32) + (c8 & 3);
        for (int t = 0; t < 54; ++t) dst[(size_t)t * 256] = src[t];
      }
    }
    ci0 += seg_c[s];
    cb0 += (seg_c[s] + 7) / 8;
  }
}

void conv_pack_host(int form, const float* w, int Cout, const int* seg_c, int nseg, float* out) {
  int Cin, Cbi;
  seg_counts(seg_c, nseg, Cin, Cbi);
  const size_t n = (size_t)Cout * Cin;
  if (form == CF_XQUAD) {
    pack_taps32(f43_rows(z_diff(w, n, 9).data(), n).data(), Cout, seg_c, nseg, out);
  } else if (form == CF_PAIR) {
    pack_taps(z_diff(w, n, 9).data(), Cout, seg_c, nseg, 27, out, true);
  } else if (form_ups(form)) {               // [phase = 2 py + px][the 12-tap pack of that phase's weights]
    const size_t per = conv_pack_floats(form, Cout, Cbi) / 4;
    for (int ph = 0; ph < 4; ++ph) {
      std::vector<float> v = phase_sums(w, n, ph >> 1, ph & 1);
      if (form == CF_PAIR_UPS) v = z_diff(v.data(), n, 4);
      pack_taps(v.data(), Cout, seg_c, nseg, 12, out + ph * per, form == CF_PAIR_UPS);
    }
  } else {
    pack_taps(w, Cout, seg_c, nseg, conv_form_taps(form), out);
  }
}

void vec_pack_host(const float* v, const int* seg_c, int nseg, float* out) {
  int ci0 = 0, cb0 = 0;
  for (int s = 0; s < nseg; ++s) {
    const int nb = (seg_c[s] + 7) / 8;
    for (int c = 0; c < nb * 8; ++c) out[cb0 * 8 + c] = (c < seg_c[s]) ? v[ci0 + c] : 0.f;
    ci0 += seg_c[s];
    cb0 += nb;
  }
}

void transpose_host(const float* w, int rows, int cols, float* out) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) out[(size_t)c * rows + r] = w[(size_t)r * cols + c];
}

void direct_pack_host(const float* w, int Cout, int Cin, int taps, float* out) {
  const int Cop = (Cout + 7) / 8 * 8;
  for (size_t i = 0; i < (size_t)taps * Cin * Cop; ++i) out[i] = 0.f;
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < taps; ++t) out[((size_t)t * Cin + ci) * Cop + co] = w[((size_t)co * Cin + ci) * taps + t];
}

}  // namespace tmk
