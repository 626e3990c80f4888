// hoist_emu.cpp — TEST INFRASTRUCTURE: the per-workgroup invariants of the N = 4096 STFT kernel on the CPU, through the helpers the
// kernel instantiates (melonix_amd/csrc/stft_core.h): the row-side pick with its in-band tests taken once (row_band_mask and the
// mask form of row_pick_key) against the form that tests kmin / kmax per key, and pass 3 with thread 0's selected twiddles
// made once (pass3_wp0) against the per-call selects.
// This is not a product path and is never loaded by melonix_amd.
#include <cstdint>
#include <cstring>

#include "../../melonix_amd/csrc/stft_core.h"

using namespace mx;

namespace {

float from_bits(uint32_t u) { return __builtin_bit_cast(float, u); }

// four magnitudes of a lane: ties everywhere, ties in pairs, rising, falling, zeros (silence), NaN payloads of either sign in
// every position, infinities, denormals
const uint32_t kPatterns[][4] = {
    {0x3f800000u, 0x3f800000u, 0x3f800000u, 0x3f800000u}, {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x3f800000u, 0x3f800000u, 0x40000000u, 0x40000000u}, {0x40000000u, 0x3f800000u, 0x3f800000u, 0x40000000u},
    {0x3dcccccdu, 0x3e4ccccdu, 0x3e99999au, 0x3ecccccdu}, {0x3ecccccdu, 0x3e99999au, 0x3e4ccccdu, 0x3dcccccdu},
    {0x7fc00000u, 0x3f800000u, 0x3f800000u, 0x3f800000u}, {0x3f800000u, 0x7fc00000u, 0x3f800000u, 0x3f800000u},
    {0x3f800000u, 0x3f800000u, 0x7fc00000u, 0x3f800000u}, {0x3f800000u, 0x3f800000u, 0x3f800000u, 0x7fc00000u},
    {0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u}, {0x7fc00001u, 0x7fc00000u, 0xffc00000u, 0x7f800001u},
    {0xffc00000u, 0x7fc00000u, 0x7fc00000u, 0xffc00000u}, {0x7f800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u},
    {0x00000001u, 0x00000001u, 0x00000000u, 0x00000002u}, {0x80000000u, 0x00000000u, 0x80000000u, 0x00000000u},
};

}  // namespace

// Every band 0 <= kmin, kmax <= 255 (empty ones included) x wave 0's 64 lanes x the patterns above: the number of (band, lane,
// pattern) triples whose masked key differs from the kmin / kmax key, or whose mask bit j is not "bin 4 lane + j in band".
extern "C" long emu_hoist_pick_mismatches(long *checked) {
  long bad = 0, n = 0;
  for (int kmin = 0; kmin < 256; ++kmin)
    for (int kmax = 0; kmax < 256; ++kmax)
      for (int lane = 0; lane < 64; ++lane) {
        const int b0 = 4 * lane;
        const unsigned mask = row_band_mask(b0, kmin, kmax);
        for (int j = 0; j < 4; ++j) bad += (((mask >> j) & 1u) != 0) != (b0 + j >= kmin && b0 + j <= kmax);
        bad += (mask >> 4) != 0;
        for (const auto &p : kPatterns) {
          const float m0 = from_bits(p[0]), m1 = from_bits(p[1]), m2 = from_bits(p[2]), m3 = from_bits(p[3]);
          const unsigned long long want = row_pick_key(b0, m0, m1, m2, m3, kmin, kmax);
          const unsigned long long got = row_pick_key(b0, m0, m1, m2, m3, mask);
          const unsigned long long got_b = row_pick_key(b0, m0, m1, m2, m3, (mask & 1u) != 0, (mask & 2u) != 0,
                                                        (mask & 4u) != 0, (mask & 8u) != 0);
          bad += (want != got) + (want != got_b);
          ++n;
        }
      }
  if (checked) *checked = n;
  return bad;
}

// Pass 3 of the N = 4096 plan for thread t on the 16 points v (32 floats) and the 7 twiddles w (14 floats), with the first KH
// selected twiddles made once: out_ref <- the per-call selects, out_new <- the hoisted ones (32 floats each).
template <int KH>
static void pass3_both(int t, const float *v, const float *w, float *out_ref, float *out_new) {
  using P = Plan<4096, 16>;
  cpx a[P::E], b[P::E], tw[P::R3 - 1], wph[KH > 0 ? KH : 1];
  for (int i = 0; i < P::E; ++i) a[i] = b[i] = mk(v[2 * i], v[2 * i + 1]);
  for (int r = 0; r < P::R3 - 1; ++r) tw[r] = mk(w[2 * r], w[2 * r + 1]);
  pass3_reg<P, true>(t, a, tw);
  pass3_wp0<P, KH>(t, tw, wph);
  pass3_reg<P, true, KH>(t, b, tw, wph);
  std::memcpy(out_ref, a, sizeof a);
  std::memcpy(out_new, b, sizeof b);
}
extern "C" int emu_hoist_pass3(int kh, int t, const float *v, const float *w, float *out_ref, float *out_new) {
  switch (kh) {
    case 0: pass3_both<0>(t, v, w, out_ref, out_new); return 0;
    case 1: pass3_both<1>(t, v, w, out_ref, out_new); return 0;
    case 2: pass3_both<2>(t, v, w, out_ref, out_new); return 0;
    case 3: pass3_both<3>(t, v, w, out_ref, out_new); return 0;
    case 4: pass3_both<4>(t, v, w, out_ref, out_new); return 0;
    case 5: pass3_both<5>(t, v, w, out_ref, out_new); return 0;
    case 6: pass3_both<6>(t, v, w, out_ref, out_new); return 0;
    case 7: pass3_both<7>(t, v, w, out_ref, out_new); return 0;
  }
  return -1;
}
