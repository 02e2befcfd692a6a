// Stand-alone host check of the conv weight packers (no GPU): every form is packed for the segment lists (5, 16, 3) and (8) at
// Cout 37 and 128 into buffers of exactly conv_pack_floats() floats -- built with -fsanitize=address,undefined a write past the
// end aborts.  The forms that reach LDS by LDS-DMA (CF_PAIR, CF_PAIR_UPS) must hold, tap for tap, the [64 cout][8 cin]
// image permuted into [2 k-halves][64 cout][4 cin] (tm_conv_frag.h); CF_XQUAD holds tiles of 32 couts, a tap being
// [2 k-halves][32 cout][4 cin], and is checked against the F(4,3) filter transform evaluated here.  Pad slots (couts past Cout,
// channels past a segment) must be zero.
//   F="-O1 -g -std=c++17 -x hip --cuda-host-only -fsanitize=address,undefined"
//   hipcc $F -Itera-mind_amd/csrc -Iinclude tools/conv_pack_check.cpp tera-mind_amd/csrc/tm_conv_pack.cpp -o conv_pack_check \
//     && ./conv_pack_check
// With -DTM_PARENT_PACK and a second copy of the packer, from the parent commit and compiled with -Dtmk=tmk_parent against its own
// headers, every form must also be byte-identical to ITS pack.  The forms are passed by this commit's numbers, so the parent's
// ConvForm must number them alike (the sed line: the parent of the commit that removed CF_XPAIR had it in front of CF_XQUAD):
//   mkdir -p P/a/b P/include && git show HEAD~1:include/teramind_hip.h > P/include/teramind_hip.h
//   for f in tm_conv_pack.cpp tm_kernels.h tm_conv_frag.h; do git show HEAD~1:tera-mind_amd/csrc/$f > P/a/b/$f; done
//   sed -i '/^  CF_XPAIR,/{h;d};/^  CF_XQUAD,/G' P/a/b/tm_kernels.h
//   hipcc $F -Dtmk=tmk_parent -c P/a/b/tm_conv_pack.cpp -o P/parent_pack.o
//   hipcc $F -Itera-mind_amd/csrc -Iinclude -DTM_PARENT_PACK -c tools/conv_pack_check.cpp -o P/check.o
//   hipcc $F -Itera-mind_amd/csrc -Iinclude -c tera-mind_amd/csrc/tm_conv_pack.cpp -o P/pack.o
//   hipcc -fsanitize=address,undefined P/check.o P/pack.o P/parent_pack.o -o P/check_parent && P/check_parent
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tm_conv_frag.h"
#include "tm_kernels.h"

#ifdef TM_PARENT_PACK
namespace tmk_parent {
void conv_pack_host(int form, const float* w, int Cout, const int* seg_c, int nseg, float* out);
size_t conv_pack_floats(int form, int Cout, int Cbi);
}
#endif

using namespace tmk;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main() {
  const int segs[2][3] = {{5, 16, 3}, {8, 0, 0}}, nsegs[2] = {3, 1}, couts[2] = {37, 128};
  const int forms[] = {CF_1X1, CF_INPLANE, CF_PLANES3, CF_ZSKIP, CF_ZSKIP_UPS, CF_PAIR, CF_PAIR_UPS, CF_XQUAD};
  const char* names[] = {"CF_1X1", "CF_INPLANE", "CF_PLANES3", "CF_ZSKIP", "CF_ZSKIP_UPS", "CF_PAIR", "CF_PAIR_UPS", "CF_XQUAD"};
  unsigned long long lcg = 88172645463325252ull;
  for (int si = 0; si < 2; ++si)
    for (int ci = 0; ci < 2; ++ci)
      for (int fi = 0; fi < 8; ++fi) {
        const int form = forms[fi], Cout = couts[ci], nseg = nsegs[si];
        int Cin = 0, Cbi = 0;
        for (int s = 0; s < nseg; ++s) { Cin += segs[si][s]; Cbi += (segs[si][s] + 7) / 8; }
        const int wtaps = form == CF_1X1 ? 1 : form == CF_INPLANE ? 9 : 27;              // taps of the reference filter
        std::vector<float> w((size_t)Cout * Cin * wtaps);
        for (float& v : w) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; v = (float)((int)(lcg >> 40) % 2001 - 1000) / 64.f + 0.015625f; }
        const size_t n = conv_pack_floats(form, Cout, Cbi);
        std::vector<float> pk(n, -7.f);
        conv_pack_host(form, w.data(), Cout, segs[si], nseg, pk.data());
        auto same_as_parent = [&] {
#ifdef TM_PARENT_PACK
          CHECK(tmk_parent::conv_pack_floats(form, Cout, Cbi) == n, "%s pack size changed", names[fi]);
          std::vector<float> old(n, -9.f);
          tmk_parent::conv_pack_host(form, w.data(), Cout, segs[si], nseg, old.data());
          CHECK(memcmp(old.data(), pk.data(), n * sizeof(float)) == 0, "%s bytes changed", names[fi]);
#endif
        };
        const bool halves = form == CF_PAIR || form == CF_PAIR_UPS;
        if (form == CF_XQUAD) {                                    // every slot: the transformed tap of its (cout, cin), or a zero pad
          size_t pads = 0, nonzero = 0, wrong = 0;
          const int n32 = (Cout + 63) / 64 * 2;
          CHECK(n == (size_t)n32 * Cbi * 54 * 256, "CF_XQUAD pack size");
          for (int nt = 0; nt < n32; ++nt) {
            int cb = 0, ci0 = 0;
            for (int s = 0; s < nseg; ci0 += segs[si][s], ++s)
              for (int b = 0; b < (segs[si][s] + 7) / 8; ++b, ++cb)
                for (int col = 0; col < 32; ++col)
                  for (int c8 = 0; c8 < 8; ++c8) {
                    const int co = nt * 32 + col, c = b * 8 + c8;
                    const bool pad = co >= Cout || c >= segs[si][s];
                    for (int r = 0; r < 9; ++r) {                  // r = product * 3 + ky
                      float u[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                      if (!pad) {
                        const float* f = &w[((size_t)co * Cin + ci0 + c) * 27];
                        const int pr = r / 3, ky = r % 3;
                        float g[3];
                        for (int kx = 0; kx < 3; ++kx) {
                          const float w0 = f[ky * 3 + kx], w1 = f[9 + ky * 3 + kx], w2 = f[18 + ky * 3 + kx];
                          g[kx] = pr == 0 ? w1 : pr == 1 ? w2 - w1 : w0 - w1;
                        }
                        u[0] = g[0] / 4.f; u[1] = -((g[0] + g[1]) + g[2]) / 6.f; u[2] = -((g[0] - g[1]) + g[2]) / 6.f;
                        u[3] = (g[0] / 24.f + g[1] / 12.f) + g[2] / 6.f; u[4] = (g[0] / 24.f - g[1] / 12.f) + g[2] / 6.f; u[5] = g[2];
                      }
                      for (int q = 0; q < 6; ++q) {
                        const float v = pk[(((size_t)nt * Cbi + cb) * 54 + r * 6 + q) * 256 + conv_frag_off(col, c8 >> 2, 32) + (c8 & 3)];
                        if (pad) { ++pads; unsigned b32; memcpy(&b32, &v, 4); CHECK(b32 == 0u, "CF_XQUAD pad slot not zero"); }
                        else { nonzero += v != 0.f; wrong += memcmp(&v, &u[q], 4) != 0; }
                      }
                    }
                  }
          }
          CHECK(wrong == 0, "CF_XQUAD: %zu slots are not the F(4,3) transform of their filter row", wrong);
          same_as_parent();
          printf("%-12s segs %-8s Cout %3d: %8zu floats, %7zu pad slots zero, %7zu real non-zero\n", names[fi], si ? "(8)" : "(5,16,3)",
                 Cout, n, pads, nonzero);
          continue;
        }
        const int taps = conv_form_taps(form), ntile = (Cout + 63) / 64, groups = (int)(n / ((size_t)ntile * Cbi * taps * 512));
        // pad slots: cout past Cout or channel past its segment
        size_t nonzero = 0, pads = 0;
        for (int g = 0; g < groups; ++g)
          for (int nt = 0; nt < ntile; ++nt) {
            int cb = 0;
            for (int s = 0; s < nseg; ++s)
              for (int b = 0; b < (segs[si][s] + 7) / 8; ++b, ++cb)
                for (int t = 0; t < taps; ++t)
                  for (int col = 0; col < 64; ++col)
                    for (int c8 = 0; c8 < 8; ++c8) {
                      const float v = pk[((((size_t)g * ntile + nt) * Cbi + cb) * taps + t) * 512 + (halves ? conv_w_off(col, c8) : col * 8 + c8)];
                      if (nt * 64 + col >= Cout || b * 8 + c8 >= segs[si][s]) { ++pads; unsigned u; memcpy(&u, &v, 4); CHECK(u == 0u, "%s pad slot not zero", names[fi]); }
                      else nonzero += v != 0.f;
                    }
          }
        same_as_parent();
        printf("%-12s segs %-8s Cout %3d: %8zu floats, %7zu pad slots zero, %7zu real non-zero\n", names[fi],
               si ? "(8)" : "(5,16,3)", Cout, n, pads, nonzero);
      }
  printf(fails ? "FAILED: %d checks\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
