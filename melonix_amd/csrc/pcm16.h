// pcm16.h — the two float -> int16 conversions of the library (definition: include/melonix_amd.h "PCM conversions"), plain
// C++ for the device and the host, defined for EVERY float: the NaN test and the range test come before the cast, and the
// cast goes through int32, so nothing here is left to what a target's conversion instruction does with a value it cannot
// represent.  tests/test_pcm16_host.py compares both with their definitions over all 2^32 bit patterns.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_PCM_HD __host__ __device__ __forceinline__
#else
#define MX_PCM_HD inline
#endif

namespace mx {

// the low 16 bits of an int32 as the int16 with those bits (no narrowing conversion of a value that does not fit)
MX_PCM_HD int16_t pcm16_low_half(int32_t i) {
  const uint32_t u = (uint32_t)i & 0xffffu;
  return (int16_t)((int32_t)(u ^ 0x8000u) - 0x8000);
}

// The reference form (mx_resynth*, mx_export_wav): what the compiled reference's static_cast<int16_t>(v * 32767.)
// (app.cpp:1212) gives.  With d = (double)v * 32767.: the low 16 bits of trunc(d) while |d| < 2^31, 0 otherwise, NaN
// included.  65538.f * 32767 = 2^31 - 2 exactly and the next float above it gives d > 2^31, so |d| < 2^31 is
// |v| <= 65538.f: one binary32 compare, false for NaN.
MX_PCM_HD int16_t pcm16_reference(float v) {
  const float in = __builtin_fabsf(v) <= 65538.f ? v : 0.f;  // (the select before the product: 0 converts to 0)
  return pcm16_low_half((int32_t)((double)in * 32767.));
}

// The clamped form (phase vocoder, PSOLA with its formant and contour renders): NaN -> 0, otherwise
// (int16)(clamp(v, -1, 1) * 32767.), the product in binary64, truncated; +-Inf -> +-32767.
MX_PCM_HD int16_t pcm16_clamped(float v) {
  const float c = v < -1.f ? -1.f : (1.f < v ? 1.f : (v == v ? v : 0.f));
  return (int16_t)(int32_t)((double)c * 32767.);  // |c * 32767.| <= 32767: fits both
}

}  // namespace mx
