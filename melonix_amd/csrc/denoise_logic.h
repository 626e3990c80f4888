// denoise_logic.h — the host side of the noise reduction (definition: include/melonix_amd.h "Noise reduction"): the parameter
// and print checks, the two factors, the frames of a region, and the print of a set of power rows.  Plain C++, compiled by the
// library (capi_denoise.cpp, capi_audio.cpp) and by tests/emu/denoise_emu.cpp; the geometry it shares with the kernels is
// denoise_core.h's.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"

namespace mx {

// why the parameters / the print are refused, or null
const char *denoise_params_error(const mx_denoise_params &p);
const char *noise_print_error(const float *print);
// floor = 10^(-reduction_db / 20), sens = 10^(sensitivity_db / 10): binary64, rounded once to binary32 (p: checked)
struct DenoiseFactors {
  float floor, sens;
};
DenoiseFactors denoise_factors(const mx_denoise_params &p);
// The frames that lie wholly inside samples [begin, end) of a take of n samples: -> false where the region is not inside the
// take, or holds no frame or more than 8192
bool noise_region_frames(int64_t n, int64_t begin, int64_t end, int64_t *first_frame, int64_t *count);
// print[k] = (binary64 sum over f < count, ascending, of rows[513 f + k]) / count, rounded to binary32; count >= 1
void noise_print_of_rows(const float *rows, int64_t count, float *print);

}  // namespace mx
