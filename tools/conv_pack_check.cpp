// Stand-alone host check of the conv weight packers (no GPU): every form is packed for the segment lists (5, 16, 3) and (8) at
// Cout 37 and 128 into buffers of exactly conv_pack_floats() floats -- built with -fsanitize=address,undefined a write past the
// end aborts.  The forms that reach LDS by LDS-DMA (CF_PAIR, CF_PAIR_UPS, CF_XPAIR) must hold, tap for tap, the [64 cout][8 cin]
// image permuted into [2 k-halves][64 cout][4 cin] (tm_conv_frag.h).  With -DTM_PARENT_PACK and a second copy of the packer,
// from the build before the images changed and compiled with -Dtmk=tmk_parent, that is checked against ITS bytes, float for
// float and as multisets of bit patterns, and every other form must be byte-identical; without it the run checks sizes, pad
// slots and the sanitizers' silence.  Pad slots (couts past Cout, channels past a segment) must be zero.
//   hipcc -O1 -g -std=c++17 -x hip --cuda-host-only -fsanitize=address,undefined -Itera-mind_amd/csrc -Iinclude \
//         tools/conv_pack_check.cpp tera-mind_amd/csrc/tm_conv_pack.cpp -o conv_pack_check && ./conv_pack_check
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
  const int forms[] = {CF_1X1, CF_INPLANE, CF_PLANES3, CF_ZSKIP, CF_ZSKIP_UPS, CF_PAIR, CF_PAIR_UPS, CF_XPAIR};
  const char* names[] = {"CF_1X1", "CF_INPLANE", "CF_PLANES3", "CF_ZSKIP", "CF_ZSKIP_UPS", "CF_PAIR", "CF_PAIR_UPS", "CF_XPAIR"};
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
        const bool halves = form == CF_PAIR || form == CF_PAIR_UPS || form == CF_XPAIR;
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
        size_t moved = 0;
#ifdef TM_PARENT_PACK
        CHECK(tmk_parent::conv_pack_floats(form, Cout, Cbi) == n, "%s pack size changed", names[fi]);
        std::vector<float> old(n, -9.f);
        tmk_parent::conv_pack_host(form, w.data(), Cout, segs[si], nseg, old.data());
        if (!halves) CHECK(memcmp(old.data(), pk.data(), n * sizeof(float)) == 0, "%s bytes changed", names[fi]);
        else {
          for (size_t blk = 0; blk < n / 512; ++blk)
            for (int col = 0; col < 64; ++col)
              for (int c8 = 0; c8 < 8; ++c8) {
                const size_t a = blk * 512 + col * 8 + c8, b = blk * 512 + conv_w_off(col, c8);
                CHECK(memcmp(&old[a], &pk[b], 4) == 0, "%s block %zu cout %d cin %d: not the parent's float", names[fi], blk, col, c8);
                moved += a != b;
              }
          std::vector<float> x(old), y(pk);                       // and as multisets of bit patterns
          auto bits = [](float f) { unsigned u; memcpy(&u, &f, 4); return u; };
          std::sort(x.begin(), x.end(), [&](float p, float q) { return bits(p) < bits(q); });
          std::sort(y.begin(), y.end(), [&](float p, float q) { return bits(p) < bits(q); });
          CHECK(memcmp(x.data(), y.data(), n * sizeof(float)) == 0, "%s is not a permutation of the parent's pack", names[fi]);
        }
#endif
        printf("%-12s segs %-8s Cout %3d: %8zu floats, %7zu pad slots zero, %7zu real non-zero, %7zu floats moved\n", names[fi],
               si ? "(8)" : "(5,16,3)", Cout, n, pads, nonzero, moved);
      }
  printf(fails ? "FAILED: %d checks\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
