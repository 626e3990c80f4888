// onset_emu.cpp — the onset-strength kernel's per-lane functions (melonix_amd/csrc/onset_core.h) run lane by lane on the CPU,
// in the walker's order: a run of consecutive frames, the head frames first, the transform of onset_walk_emu.h, the wavefront's
// sum in the kernel's exchange order.  tests/test_onset_host.py compares it with the binary64 definition: what the GPU adds is
// the device's log1pf / sqrtf.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared onset_emu.cpp -o libonset_emu.so
#include "onset_walk_emu.h"

using namespace mx::onset;

extern "C" void emu_onset_flux(const float *wav, long n, int hop, long first_frame, long count, int lag, int kmin, int kmax,
                               float compress, int run, float *flux) {
  emu::Walk walk(wav, n);
  for (long f0 = 0; f0 < count; f0 += run) {
    const long f1 = f0 + run < count ? f0 + run : count;
    float prev[kMaxLag][kLanes][8] = {};
    const long h0 = first_frame + f0, h1 = first_frame + f1, hs = h0 - lag > 0 ? h0 - lag : 0;
    for (long h = hs; h < h1; ++h) {
      float2 v[kLanes][8];
      float cur[kLanes][8];
      walk.frame(h, hop, v, [](int, const float2(&)[8]) {});
      for (int l = 0; l < kLanes; ++l) compressed(l, walk.lc[(size_t)l], v[l], walk.img.data(), compress, cur[l]);
      if (h >= h0) {
        float part[kLanes];
        for (int l = 0; l < kLanes; ++l) part[l] = lane_flux(l, cur[l], prev[lag - 1][l], kmin, kmax);
        flux[h - first_frame] = wave_sum_host(part);
      }
      for (int i = lag - 1; i > 0; --i)
        for (int l = 0; l < kLanes; ++l)
          for (int r = 0; r < 8; ++r) prev[i][l][r] = prev[i - 1][l][r];
      for (int l = 0; l < kLanes; ++l)
        for (int r = 0; r < 8; ++r) prev[0][l][r] = cur[l][r];
    }
  }
}
