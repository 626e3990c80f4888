// resample_logic.h — host logic behind the sample-rate conversion (resample_logic.cpp, plain g++, binary64, no contraction): the
// tap table of a plan.  The definition is include/melonix_amd.h's ("Sample-rate conversion"); the library and
// tests/emu/resample_emu.cpp compile the same unit.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"

namespace mx {

// I0(x), x >= 0: the power series sum of ((x / 2)^k / k!)^2, k ascending, until a term falls below 2^-60 of the sum
double resample_bessel_i0(double x);
// h[phi][k], phi < L, k < taps, as binary32: out holds L * taps floats, a row per phase.  A plan of plan_for, taps > 0.
void resample_table(const mx_resample_plan &p, float *out);
// The same with a row per tap index: out[k * L + phi] = h[phi][k], what the kernels read.
void resample_table_by_tap(const mx_resample_plan &p, float *out);

}  // namespace mx
