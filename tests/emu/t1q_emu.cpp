// t1q_emu.cpp — TEST INFRASTRUCTURE: the q-major T1 image and the one-reduction row-side pick of the N = 4096 STFT kernel on the
// CPU, through the helpers the kernel instantiates (melonix_amd/csrc/stft_core.h): store_t1q / load_t1q_tw2 / fetch_tw2_tail
// against store_t1 / load_t1_tw2, row_pick_lane_max / row_pick_first against max(row_pick_key) over the wavefront.
// This is not a product path and is never loaded by melonix_amd.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../melonix_amd/csrc/stft_core.h"

using namespace mx;

namespace {

using P = Plan<4096, 16>;
constexpr int kImg = t1q_size<P>();  // 2080 points

float from_bits(uint32_t u) { return __builtin_bit_cast(float, u); }
uint32_t to_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

std::vector<cpx> tw2_table() {  // tw2[(r-1)*R1 + k] = exp(-2*pi*i*r*k/(R1*R2))
  std::vector<cpx> tw(P::TW2);
  for (int r = 1; r < P::R2; ++r)
    for (int k = 0; k < P::R1; ++k) {
      const double a = -2.0 * M_PI * (double)(r * k) / (double)(P::R1 * P::R2);
      tw[(r - 1) * P::R1 + k] = mk((float)std::cos(a), (float)std::sin(a));
    }
  return tw;
}

// four magnitudes of a lane: ties everywhere, zeros (silence), ties in pairs, rising, falling, NaN payloads of either sign in
// every position, infinities, the largest finite value, denormals, negative zero
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
constexpr int kNP = (int)(sizeof kPatterns / sizeof kPatterns[0]);
// what the other 63 lanes hold while one lane holds a pattern: silence, the value most patterns tie with, a NaN everywhere
const uint32_t kBackgrounds[] = {0x00000000u, 0x3f800000u, 0x7fc00000u};
constexpr int kNB = (int)(sizeof kBackgrounds / sizeof kBackgrounds[0]);

// A wavefront of wave 0 for one band: lane l holds the magnitudes bits[l][0..3] of bins 4 l .. 4 l + 3.  Per lane it keeps what the
// kernel's lanes hold — the in-band tests and row_pick_lane_max — and, for the reference, the lane's row_pick_key; set() changes
// one lane.
struct Wave {
  int kmin, kmax;
  uint32_t bits[64][4], m[64];
  unsigned mask[64];
  unsigned long long key[64];
  uint64_t rany;
  void band(int k0, int k1) {
    kmin = k0, kmax = k1, rany = 0;
    for (int l = 0; l < 64; ++l) {
      mask[l] = row_band_mask(4 * l, kmin, kmax);
      rany |= (uint64_t)(mask[l] != 0) << l;
    }
  }
  void set(int l, const uint32_t (&b)[4]) {
    std::memcpy(bits[l], b, sizeof b);
    const float f0 = from_bits(b[0]), f1 = from_bits(b[1]), f2 = from_bits(b[2]), f3 = from_bits(b[3]);
    m[l] = row_pick_lane_max(f0, f1, f2, f3, (mask[l] & 1u) != 0, (mask[l] & 2u) != 0, (mask[l] & 4u) != 0, (mask[l] & 8u) != 0);
    key[l] = row_pick_key(4 * l, f0, f1, f2, f3, kmin, kmax);
  }
  // the record by the one-reduction rule: what the kernel does with a DPP reduction, a ballot, a find-first-set and lane reads
  void pick_new(int &bin, uint32_t &mag) const {
    uint32_t mhi = 0;
    for (int l = 0; l < 64; ++l) mhi = m[l] > mhi ? m[l] : mhi;
    int L = 0;  // ctz(ballot(m == mhi) & rany): the lowest lane that reaches the maximum and holds an in-band bin
    while (L < 63 && !(m[L] == mhi && ((rany >> L) & 1u))) ++L;
    bin = 4 * L + row_pick_first(mhi, bits[L][0], bits[L][1], bits[L][2], bits[L][3], (mask[L] & 1u) != 0, (mask[L] & 2u) != 0,
                                 (mask[L] & 4u) != 0, (mask[L] & 8u) != 0);
    mag = mhi;
  }
  // ... and by the keys: the record of max(row_pick_key) over the lanes
  void pick_ref(int &bin, uint32_t &mag) const {
    unsigned long long best = 0ull;
    for (int l = 0; l < 64; ++l) best = key[l] > best ? key[l] : best;
    bin = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
    mag = (uint32_t)(best >> 32);
  }
};

}  // namespace

// The layout, through the store and read forms themselves.  Returns the number of violations of:
//   (a) (j, q) -> t1q_index(j, q) is injective into [0, 2080);
//   (b) store_t1q of thread t puts its output q at t1q_index(t, q), for every t and q;
//   (c) load_t1q_tw2 of thread t reads, as its input r, the point (j = (t >> 4) + 8 r, q = t & 15), for every t and r — and its
//       twiddles are tw2[(r - 1)*16 + (t & 15)], rows 14 and 15 coming from fetch_tw2_tail's registers (the LDS table holds 13);
//   (d) every 32-lane group of a ds_read_b64 (lanes 0-31, 32-63 of a wave, one r) touches 32 different 8-byte slots mod 32;
//   (e) every 16-lane group of a ds_write_b64 (one q) touches 16 different 8-byte slots mod 16, i.e. 32 banks once each.
extern "C" long emu_t1q_layout_violations(long *checked) {
  long bad = 0, n = 0;
  std::vector<int> seen(kImg, 0);
  for (int j = 0; j < P::T; ++j)
    for (int q = 0; q < P::R1; ++q) {
      const int i = t1q_index(j, q);
      bad += (i < 0 || i >= kImg);
      if (i >= 0 && i < kImg) bad += seen[i]++ != 0;
      ++n;
    }
  // (b): every thread writes the pair (j, q) as its value; where it lands is where the store form put it
  std::vector<cpx> img(kImg, mk(-1.0f, -1.0f));
  int where[P::T][P::R1];  // point index of thread t's q-th store
  for (int t = 0; t < P::T; ++t) {
    cpx v[P::E];
    for (int q = 0; q < P::R1; ++q) v[q] = mk((float)t, (float)q);
    store_t1q<P>(t, v, img.data());
  }
  for (int t = 0; t < P::T; ++t)
    for (int q = 0; q < P::R1; ++q) {
      const cpx z = img[t1q_index(t, q)];
      bad += !(z.x == (float)t && z.y == (float)q);
      where[t][q] = t1q_index(t, q);
      ++n;
    }
  // (c): read the (j, q) pairs back; an image of point indices tells the addresses the read form touches
  const std::vector<cpx> tw = tw2_table();
  std::vector<cpx> ltw(tw.begin(), tw.begin() + kT1qTwRows * P::R1);  // the 13 rows the LDS keeps
  std::vector<cpx> idx(kImg);
  for (int i = 0; i < kImg; ++i) idx[i] = mk((float)i, 0.0f);
  int from[P::T][P::R2];  // point index of thread t's r-th read
  for (int t = 0; t < P::T; ++t) {
    cpx v[P::E], w[P::R2 - 1], wt[P::R2 - 1 - kT1qTwRows];
    fetch_tw2_tail<P>(t, tw.data(), wt);
    load_t1q_tw2<P>(t, v, img.data(), ltw.data(), wt, w);
    for (int r = 0; r < P::R2; ++r) {
      bad += !(v[r].x == (float)((t >> 4) + 8 * r) && v[r].y == (float)(t & 15));
      ++n;
    }
    for (int r = 1; r < P::R2; ++r) {
      const cpx e = tw[(r - 1) * P::R1 + (t & 15)];
      bad += !(to_bits(w[r - 1].x) == to_bits(e.x) && to_bits(w[r - 1].y) == to_bits(e.y));
      ++n;
    }
    load_t1q_tw2<P>(t, v, idx.data(), ltw.data(), wt, w);
    for (int r = 0; r < P::R2; ++r) from[t][r] = (int)v[r].x;
  }
  // (d), (e): the bank rules on the addresses just observed (8-byte points: slot = point index)
  for (int g = 0; g < P::T / 32; ++g)
    for (int r = 0; r < P::R2; ++r) {
      unsigned used = 0;
      for (int l = 0; l < 32; ++l) used |= 1u << (from[32 * g + l][r] & 31);
      bad += used != 0xffffffffu;
      ++n;
    }
  for (int g = 0; g < P::T / 16; ++g)
    for (int q = 0; q < P::R1; ++q) {
      unsigned used = 0;
      for (int l = 0; l < 16; ++l) used |= 1u << (where[16 * g + l][q] & 15);
      bad += used != 0xffffu;
      ++n;
    }
  if (checked) *checked = n;
  return bad;
}

// One frame of the N = 4096 plan, Y[t][e] = frame[2*(t + 128 e)], frame[2*(t + 128 e) + 1], through pass 1, the first
// transposition and pass 2, once by the XOR image and the 15-row table and once by the q-major image with rows 14 and 15 of the
// table in "registers": out_xor, out_q <- v[] of every thread after pass 2 (128 * 16 * 2 floats each).
extern "C" void emu_t1q_frame(const float *frame, float *out_xor, float *out_q) {
  const std::vector<cpx> tw = tw2_table();
  std::vector<cpx> ltw(tw.begin(), tw.begin() + kT1qTwRows * P::R1);
  std::vector<cpx> img_x(t1_size<P>()), img_q(kImg, mk(0.0f, 0.0f));
  std::vector<cpx> v1(P::T * P::E);
  for (int t = 0; t < P::T; ++t) {
    cpx Y[P::E], v[P::E];
    for (int e = 0; e < P::E; ++e) Y[e] = mk(frame[2 * (t + P::T * e)], frame[2 * (t + P::T * e) + 1]);
    pass1<P>(Y, v);
    store_t1<P>(t, v, img_x.data());
    store_t1q<P>(t, v, img_q.data());
  }
  for (int t = 0; t < P::T; ++t) {
    cpx v[P::E], w[P::R2 - 1], wt[P::R2 - 1 - kT1qTwRows];
    load_t1_tw2<P>(t, v, img_x.data(), tw.data(), w);
    pass2_reg<P>(v, w);
    std::memcpy(out_xor + 2 * P::E * t, v, sizeof v);
    fetch_tw2_tail<P>(t, tw.data(), wt);
    load_t1q_tw2<P>(t, v, img_q.data(), ltw.data(), wt, w);
    pass2_reg<P>(v, w);
    std::memcpy(out_q + 2 * P::E * t, v, sizeof v);
  }
}

// Every band 0 <= kmin <= kmax <= 255 x every lane of wave 0 x a pattern in that lane x a background in the other 63 lanes, and
// every pattern in all 64 lanes at once (ties across lanes): the number of wavefronts whose one-reduction record differs from the
// record of max(row_pick_key).  The lanes that hold the band's ends and their neighbours on either side take every pattern (their
// in-band tests differ from bin to bin); a lane inside the band takes kInside (ties, silence, rising, a NaN in one place, NaN
// payloads of either sign), a lane outside it the two with the largest bit patterns (what would win if a mask let it through).
extern "C" long emu_t1q_pick_mismatches(long *checked) {
  long bad = 0, n = 0;
  static Wave w;
  constexpr int kInside[] = {0, 1, 4, 6, 11, 12}, kFar[] = {11, 12};
  for (int kmin = 0; kmin < 256; ++kmin)
    for (int kmax = kmin; kmax < 256; ++kmax) {
      w.band(kmin, kmax);
      auto one = [&]() {
        int b0, b1;
        uint32_t m0, m1;
        w.pick_new(b0, m0);
        w.pick_ref(b1, m1);
        bad += (b0 != b1) + (m0 != m1);
        ++n;
      };
      for (int p = 0; p < kNP; ++p) {
        for (int l = 0; l < 64; ++l) w.set(l, kPatterns[p]);
        one();
      }
      const int la = kmin / 4, lb = kmax / 4;
      for (int g = 0; g < kNB; ++g) {
        const uint32_t bg[4] = {kBackgrounds[g], kBackgrounds[g], kBackgrounds[g], kBackgrounds[g]};
        for (int l = 0; l < 64; ++l) w.set(l, bg);
        for (int l = 0; l < 64; ++l) {
          if ((l >= la - 1 && l <= la + 1) || (l >= lb - 1 && l <= lb + 1)) {
            for (int p = 0; p < kNP; ++p) {
              w.set(l, kPatterns[p]);
              one();
            }
          } else if (l > la && l < lb) {
            for (int p : kInside) {
              w.set(l, kPatterns[p]);
              one();
            }
          } else {
            for (int p : kFar) {
              w.set(l, kPatterns[p]);
              one();
            }
          }
          w.set(l, bg);
        }
      }
    }
  if (checked) *checked = n;
  return bad;
}
