// compress_logic.h — the host side of the dynamics compressor (definition: include/melonix_amd.h "Dynamics compressor"): the
// parameter check, the defaults, the plan and the curve, in binary64.  Plain C++, compiled by the library (capi_compress.cpp,
// capi_audio.cpp) and by tests/emu/compress_emu.cpp; the geometry it shares with the kernels is compress_core.h's.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"

namespace mx {

// why the parameters are refused, or null
const char *compress_params_error(const mx_compress_params &p);
// -18 dB, 4, 6 dB, 5 ms, 100 ms, 0 ms, 1
mx_compress_params compress_defaults();
// D, K, the two Q24 coefficients, W and Gc of checked parameters at a checked rate
mx_compress_plan compress_plan(int sr, const mx_compress_params &p);
// T[0 .. 2049) of checked parameters
void compress_curve(const mx_compress_params &p, int32_t *out);

}  // namespace mx
