// sibilant_core.h — the per-lane arithmetic of the sibilant-feature kernel (sibilant_kernels.hip) behind onset_core.h's
// transform: the real-FFT split into powers, the lane's shares of the three sums and of the zero-crossing count.  Plain C++
// between the kernel's barriers, no intrinsics: tests/emu/sibilant_emu.cpp runs the same functions lane by lane on the CPU.
// Built with -ffp-contract=off: every product and sum rounds as written.
#pragma once
#include "onset_core.h"

namespace mx {
namespace sib {

using namespace onset;

// split without the compression: P[r] = (|X_k| / 512)^2, k = lane + 64 r (bin 0 is computed and never summed).  2 X_k comes
// out of the split, so the scale is 1 / 1024^2: a power of two, exact.
MX_ONSET_HD void powers(int lane, const LaneConsts &c, const float2 (&z)[8], const float2 *img, float (&out)[8]) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const float2 a = z[r], b = img[(kM - k) & (kM - 1)];
    const float2 e = c_mk(a.x + b.x, a.y - b.y), d = c_mk(a.x - b.x, a.y + b.y);
    const float2 t = c_mul(c.ts[r], d);
    const float re = e.x + t.y, im = e.y - t.x;  // 2 X_k
    out[r] = (re * re + im * im) * (1.0f / 1048576.0f);
  }
}
// the lane's shares of low (k in [1, ks)), high (k in [ks, 511]) and sum k P_k (k in [1, 511]): its bins in ascending r
struct LaneSums {
  float low, high, moment;
};
MX_ONSET_HD LaneSums lane_sums(int lane, const float (&P)[8], int ks) {
  LaneSums s;
  s.low = s.high = s.moment = 0.f;
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    if (k >= 1) {
      if (k < ks) s.low += P[r];
      else s.high += P[r];
      s.moment += (float)k * P[r];
    }
  }
  return s;
}
// Zero crossings of the raw frame.  Bit r of the lane's masks: whether its samples 128 r + 2 lane (first) and + 1 (second) are
// negative — v < 0, so zeros, -0 and NaN are not.
MX_ONSET_HD void sign_masks(const float2 (&x)[8], uint32_t &first, uint32_t &second) {
  first = second = 0u;
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    first |= (x[r].x < 0.f ? 1u : 0u) << r;
    second |= (x[r].y < 0.f ? 1u : 0u) << r;
  }
}
MX_ONSET_HD int popcount8(uint32_t m) {
  m = (m & 0x55u) + ((m >> 1) & 0x55u);
  m = (m & 0x33u) + ((m >> 2) & 0x33u);
  return (int)((m + (m >> 4)) & 0x0Fu);
}
// the lane's share of the count: its own 8 pairs, and the 8 boundaries between its second samples and the next samples of
// the frame.  next_first: the `first` mask of lane (lane + 1) & 63.  Lane 63's neighbour is lane 0's sample of row r + 1, and
// row 7 has none (sample 1023 is the frame's last).
MX_ONSET_HD int lane_crossings(int lane, uint32_t first, uint32_t second, uint32_t next_first) {
  const uint32_t nb = lane == kLanes - 1 ? next_first >> 1 : next_first;
  const uint32_t valid = lane == kLanes - 1 ? 0x7Fu : 0xFFu;
  return popcount8(first ^ second) + popcount8((second ^ nb) & valid);
}
// the record's third field from the wavefront's sums
MX_ONSET_HD float centroid_of(float low, float high, float moment) {
  const float tot = low + high;
  return tot == 0.f ? 0.f : moment / tot;
}

}  // namespace sib
}  // namespace mx
