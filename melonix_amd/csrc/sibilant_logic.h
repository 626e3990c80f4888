// sibilant_logic.h — host logic behind the sibilant entry points (sibilant_logic.cpp, plain g++, binary64, no contraction):
// segments from per-frame features, the spans protection and balance share, the protected formant curve, the balance's gain
// points.  The definitions are include/melonix_amd.h's ("Sibilant detection, protection and balance"); capi_sibilant.cpp
// checks the plain arguments and hands over.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/melonix_amd.h"

namespace mx {

// feat[i]: frame first_frame + i.  Parameters in range (the caller's check).
std::vector<mx_sibilant> sibilant_segments(const mx_sib_feat *feat, int64_t count, int hop, int64_t first_frame,
                                           const mx_sibilant_params &p);
// The checks of a formant curve and of a sibilant list for an audio of n samples: nullptr, or what is wrong (static text).
const char *formant_curve_error(const mx_formant_point *points, int64_t npoints);
const char *sibilant_list_error(const mx_sibilant *sibs, int64_t nsib, int64_t n);
// Lists that passed those checks, ramp >= 1, n >= 1.
std::vector<mx_formant_point> formant_protect(const mx_formant_point *points, int64_t npoints, const mx_sibilant *sibs, int64_t nsib,
                                              int32_t ramp, int64_t n);
std::vector<mx_gain_point> sibilant_gain_points(const mx_sibilant *sibs, int64_t nsib, double db, int32_t ramp, int64_t n);
// The check of a gain list: nullptr, or what is wrong.
const char *gain_points_error(const mx_gain_point *pts, int64_t npts);

}  // namespace mx
