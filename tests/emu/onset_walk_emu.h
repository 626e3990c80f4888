// onset_walk_emu.h — what onset_emu.cpp and sibilant_emu.cpp share: the 1024-point transform of melonix_amd/csrc/onset_core.h run
// lane by lane on the CPU, a loop over the 64 lanes where the kernels (melonix_amd/csrc/onset_walk.h) have a barrier.  The heads
// and tails of the two walkers stay in their files.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../melonix_amd/csrc/onset_core.h"

namespace emu {

using namespace mx::onset;

// the context's table (W1024^j, j < 1024, rounded from binary64) and what every lane keeps of it for the whole walk
struct Walk {
  std::vector<float2> tw, img;
  std::vector<LaneConsts> lc;
  const float *wav;
  long n;
  Walk(const float *wav_, long n_) : tw(1024), img(kImage), lc(kLanes), wav(wav_), n(n_) {
    for (int j = 0; j < 1024; ++j) {
      const double ang = -2.0 * M_PI * (double)j / 1024.0;
      tw[(size_t)j].x = (float)std::cos(ang);
      tw[(size_t)j].y = (float)std::sin(ang);
    }
    for (int l = 0; l < kLanes; ++l) lane_consts(l, tw.data(), lc[(size_t)l]);
  }
  // zeros outside the file: the mx_audio pad
  float sample(long i) const { return i >= 0 && i < n ? wav[i] : 0.f; }
  // Frame h at `hop` through the transform: leaves v[l] = lane l's Z[l + 64 r] and Z in the image in bin order, ready for the
  // split.  head(l, x) sees lane l's raw sample pairs before pass 1 takes them.
  template <class Head>
  void frame(long h, int hop, float2 (&v)[kLanes][8], Head &&head) {
    for (int l = 0; l < kLanes; ++l) {
      float2 x[8];
      for (int r = 0; r < 8; ++r) {
        const long i = h * hop - 512 + 128 * r + 2 * l;
        x[r].x = sample(i);
        x[r].y = sample(i + 1);
      }
      head(l, x);
      pass1(l, lc[(size_t)l], x, img.data());
    }
    for (int l = 0; l < kLanes; ++l) pass2(l, lc[(size_t)l], img.data(), v[l]);
    for (int l = 0; l < kLanes; ++l) store2(l, v[l], img.data());
    for (int l = 0; l < kLanes; ++l) pass3(l, img.data(), v[l]);
    for (int l = 0; l < kLanes; ++l) store3(l, v[l], img.data());
  }
};

}  // namespace emu
