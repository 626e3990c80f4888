// step_core.h — the 10 ms step that the loudness records (loudness_core.h) and the true-peak records (truepeak_core.h) are cut
// into (definition: include/melonix_amd.h "Loudness and note levelling"), plain C++ for the host, the device and the emulations of
// tests/emu: the sample rates accepted, a step's samples, a take's steps, and the function macro of the two core headers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_STEP_HD __host__ __device__ __forceinline__
#else
#define MX_STEP_HD inline
#endif

namespace mx {
namespace step {

constexpr int kMinRate = 8000, kMaxRate = 384000;

// S and the step count of a take (sr in range: the caller's check)
MX_STEP_HD int step_samples(int sr) { return (sr + 50) / 100; }
MX_STEP_HD int64_t step_count(int64_t n, int sr) { return n > 0 ? (n + step_samples(sr) - 1) / step_samples(sr) : 0; }

}  // namespace step
}  // namespace mx
