// truepeak_core.h — the arithmetic of the true-peak records and the look-ahead limiter (truepeak_kernels.hip; definition:
// include/melonix_amd.h "True peak, limiter and loudness range"), plain C++ for the device and for tests/emu/truepeak_emu.cpp:
// the geometry, the tap table, a sample's peak, the Q30 quotient and the final product.  Built with -ffp-contract=off: every
// product is rounded before its sum.  Everything between the peak and the gain is integer.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"
#include "step_core.h"

namespace mx {
namespace tp {

using namespace step;  // the 10 ms step: step_samples, step_count
constexpr int kTaps = 12, kBefore = 5, kAfter = 6;  // a sample's peak reads x[i - 5 .. i + 6]
constexpr int kMaxLookahead = 1024;
constexpr int32_t kUnity = 1 << 30;  // gain 1 in Q30

// L (sr in range: the caller's check)
MX_STEP_HD int oversampling(int sr) { return sr < 88200 ? 4 : sr < 176400 ? 2 : 1; }

// c_u[d + 5], d = -5 .. 6, for u = 1/4, 1/2, 3/4: (float)(sinc(d - u) * blackman(d - u)) evaluated in binary64
// (tests/test_truepeak_host.py holds the formula against these literals).  mx_true_peak_taps hands them out.
#define MX_TP_TAPS                                                                                                              \
  {                                                                                                                             \
    {-0x1.48d10ep-11f, 0x1.496c9p-8f, -0x1.3ad48ep-6f, 0x1.c6a142p-5f, -0x1.34cd12p-3f, 0x1.c9bbcep-1f, 0x1.20693cp-2f,         \
     -0x1.72b4aap-4f, 0x1.118d78p-5f, -0x1.52760cp-7f, 0x1.1174f4p-9f, -0x1.fd80cep-15f},                                       \
    {-0x1.7f7b26p-12f, 0x1.340734p-8f, -0x1.49c2f4p-6f, 0x1.f4ca88p-5f, -0x1.502f84p-3f, 0x1.3ce71p-1f, 0x1.3ce71p-1f,          \
     -0x1.502f84p-3f, 0x1.f4ca88p-5f, -0x1.49c2f4p-6f, 0x1.340734p-8f, -0x1.7f7b26p-12f},                                       \
    {-0x1.fd80cep-15f, 0x1.1174f4p-9f, -0x1.52760cp-7f, 0x1.118d78p-5f, -0x1.72b4aap-4f, 0x1.20693cp-2f, 0x1.c9bbcep-1f,        \
     -0x1.34cd12p-3f, 0x1.c6a142p-5f, -0x1.3ad48ep-6f, 0x1.496c9p-8f, -0x1.48d10ep-11f},                                        \
  }

// y_{i,u} = sum over d ascending of x[i + d] * c_u[d], from +0.f, each product rounded, then added.  w[k] = x[i - 5 + k].
MX_STEP_HD float interpolated(const float *w, int phase) {
  constexpr float c[3][kTaps] = MX_TP_TAPS;
  float y = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < kTaps; ++k) y = y + w[k] * c[phase][k];
  return y;
}
MX_STEP_HD float magnitude(float v) { return v < 0.f ? -v : v; }
// |x| of a sample that is not NaN, else 0: the sample peak's rule (mx_loud_step.peak's)
MX_STEP_HD float sample_magnitude(float x) { return x == x ? __builtin_fabsf(x) : 0.f; }
// p_i: |x_i| if x_i is not NaN, else 0; then the |y| of every used offset that is larger (a NaN compares false; Inf counts).
// w[k] = x[i - 5 + k], k < 12; L the oversampling (4: all three offsets, 2: 1/2 alone, 1: none).
MX_STEP_HD float sample_peak(const float *w, int L) {
  float p = sample_magnitude(w[kBefore]);
  if (L == 4) {
    const float a = __builtin_fabsf(interpolated(w, 0));
    p = a > p ? a : p;
  }
  if (L >= 2) {
    const float a = __builtin_fabsf(interpolated(w, 1));
    p = a > p ? a : p;
  }
  if (L == 4) {
    const float a = __builtin_fabsf(interpolated(w, 2));
    p = a > p ? a : p;
  }
  return p;
}

// q: the gain in Q30 that brings a peak p to the ceiling c; unity wherever !(p > c); 0 for p = Inf
MX_STEP_HD int32_t required_gain(float p, float c) {
  if (!(p > c)) return kUnity;
  return (int32_t)(((double)c / (double)p) * 1073741824.0);  // (the quotient is in [0, 1): truncation is the floor)
}
// out_i = (float)((double)x_i * g_i), g_i = (double)s_i / (double)((A + 1) << 30), s_i the sum of A + 1 window minima
MX_STEP_HD float limited(float x, int64_t s, int A) {
  const int64_t full = (int64_t)(A + 1) << 30;
  const double g = s == full ? 1.0 : (double)s / (double)full;  // (the quotient of equal numbers is 1.0: no division needed)
  return (float)((double)x * g);
}

// How many consecutive steps one workgroup of the record kernel stages and walks: about 4096 samples' worth, one step at the
// rates whose step is longer than half of that.  No record depends on it.
MX_STEP_HD int steps_per_block(int S) { return S > 2048 ? 1 : 4096 / S; }

}  // namespace tp
}  // namespace mx
