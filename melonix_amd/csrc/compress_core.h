// compress_core.h — the arithmetic of the dynamics compressor (compress_kernels.hip; definition: include/melonix_amd.h "Dynamics
// compressor"), plain C++ for the device and for tests/emu/compress_emu.cpp: the step geometry, a sample's magnitude, the target
// look-up, the recurrence step, the interpolated product, the final quotient, and the geometry of the three launches.  Integers
// from the look-up to the product; one binary64 product and quotient at the end, built with -ffp-contract=off.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"
#include "step_core.h"

namespace mx {
namespace cp {

constexpr int32_t kUnity = 1 << 30;                // gain 1 in Q30
constexpr int32_t kFull = 1 << 24;                 // coefficient 1 in Q24
constexpr int kGroup = 4096, kMaxWarm = 32768;     // Gc, the longest warm-up
constexpr int kCurve = MX_COMPRESS_CURVE;          // 2049 entries, 64 an octave from 2^-24 to 2^8
constexpr uint32_t kBase = (uint32_t)(127 - 24) << 23;  // bits(2^-24)
constexpr uint32_t kTop = (uint32_t)(127 + 8) << 23;    // bits(2^8) = kBase + (2048 << 17)

// D and B (sr in range: the caller's check)
MX_STEP_HD int step_samples(int sr) { return (sr + 500) / 1000; }
MX_STEP_HD int64_t steps_of(int64_t n, int D) { return n > 0 ? (n + D - 1) / D : 0; }
// the steps the recurrence is asked for: [0, B + K), the look-ahead behind the file's end
MX_STEP_HD int64_t curve_steps(int64_t n, int D, int K) { return steps_of(n, D) + K; }

// |x| of a sample that is not NaN, else 0
MX_STEP_HD float magnitude(float x) { return x == x ? __builtin_fabsf(x) : 0.f; }
MX_STEP_HD uint32_t bits_of(float p) {
  union {
    float f;
    uint32_t u;
  } v;
  v.f = p;
  return v.u;
}
// q: the Q30 target of a peak p >= 0 (never NaN), T the 2049-entry curve
MX_STEP_HD int32_t target(const int32_t *T, float p) {
  const uint32_t b = bits_of(p);  // (p >= 0: the bit patterns order as the values do)
  if (b >= kTop) return T[kCurve - 1];
  const uint32_t u = b < kBase ? 0u : b - kBase;
  const int j = (int)(u >> 17);
  const int64_t r = (int64_t)(u & 0x1ffffu);
  return T[j] + (int32_t)(((int64_t)(T[j + 1] - T[j]) * r) >> 17);
}
// one step of the branching one-pole, rounded towards the target
MX_STEP_HD int32_t smoothed(int32_t s, int32_t q, int32_t c_att, int32_t c_rel) {
  if (q < s) return s - (int32_t)(((int64_t)(s - q) * c_att + (kFull - 1)) >> 24);
  return s + (int32_t)(((int64_t)(q - s) * c_rel + (kFull - 1)) >> 24);
}
// G_i of offset o in a step whose two gains are s0 = s_{b+K-1} and s1 = s_{b+K}
MX_STEP_HD int64_t gain_product(int32_t s0, int32_t s1, int D, int o) { return (int64_t)s0 * (D - o) + (int64_t)s1 * o; }
// out_i; the quotient is left out where it is 1 and the make-up is 1: x G / G = x exactly (x G has at most 24 + 39 - 30 bits)
MX_STEP_HD float compressed(float x, float makeup, int64_t G, int D) {
  const int64_t full = (int64_t)D << 30;
  if (G == full && makeup == 1.f) return x;
  return (float)((((double)x * (double)makeup) * (double)G) / (double)full);
}

// ---- launch geometry ----
// Peaks: P consecutive lanes share a step, P the power of two >= the aligned quads a step of D samples can touch
// (ceil((D + 3) / 4) + ... at most (D + 6) / 4 + 1), at most 64: a wavefront takes 64 / P steps at once.
MX_STEP_HD int lanes_per_step(int D) {
  const int quads = (D + 6) / 4;  // a step that begins on the last sample of a quad: 1 + ceil((D - 1) / 4) quads
  int p = 2;
  while (p < quads && p < 64) p *= 2;
  return p;
}
// Curve: the steps group g walks, [start, end): from its warm-up to its last step below `total` (curve_steps)
MX_STEP_HD int64_t group_start(int64_t g, int W) { return g * kGroup - W; }
MX_STEP_HD int64_t group_end(int64_t g, int64_t total) { return (g + 1) * kGroup < total ? (g + 1) * kGroup : total; }
// Apply: the gains outputs [first, first + count) read are s_u, u in [u_lo, u_hi] (u < 0: unity, not stored); count > 0
MX_STEP_HD int64_t gain_lo(int64_t first, int D, int K) {
  const int64_t u = first / D + K - 1;
  return u < 0 ? 0 : u;
}
MX_STEP_HD int64_t gain_hi(int64_t first, int64_t count, int D, int K) { return (first + count - 1) / D + K; }

}  // namespace cp
}  // namespace mx
