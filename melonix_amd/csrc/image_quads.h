// image_quads.h — how the kernels that stage a stretch of a padded audio image in LDS (truepeak_kernels.hip,
// resample_kernels.hip) fetch it: aligned 16-byte quads, the samples outside the file as zeros whatever the pads hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/melonix_amd.h"

namespace mx {

static_assert(MX_AUDIO_PAD % 4 == 0, "an aligned quad of the image is an aligned quad of the samples");

// the aligned quad `quad` of the padded image, its samples outside [0, n) as zeros
__device__ __forceinline__ float4 load_quad(const float4 *img, int64_t quad, int64_t n) {
  float4 v = img[quad];
  const int64_t i = 4 * quad - MX_AUDIO_PAD;
  if (i < 0 || i + 3 >= n) {
    if (i + 0 < 0 || i + 0 >= n) v.x = 0.f;
    if (i + 1 < 0 || i + 1 >= n) v.y = 0.f;
    if (i + 2 < 0 || i + 2 >= n) v.z = 0.f;
    if (i + 3 < 0 || i + 3 >= n) v.w = 0.f;
  }
  return v;
}

}  // namespace mx
