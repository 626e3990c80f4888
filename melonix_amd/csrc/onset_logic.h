// onset_logic.h — host logic behind the onset entry points (onset_logic.cpp, plain g++, binary64, no contraction): the peak
// picker over an onset-strength curve and the time-warp markers that move anchors onto a tempo grid.  The definitions are
// include/melonix_amd.h's ("Onset detection", "Timing markers"); capi_onset.cpp checks the arguments and hands over.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/melonix_amd.h"

namespace mx {

// flux[i]: frame first_frame + i.  Parameters in range (the caller's check).
std::vector<mx_onset> pick_onsets(const float *flux, int64_t count, int hop, int64_t first_frame, const mx_onset_pick_params &p);
// anchors strictly increasing in [0, n), base strictly increasing in [1, n) with dTime 0, parameters in range (the
// caller's checks).  -> the markers on anchors (those > 0) and base samples, sorted.
std::vector<mx_marker> timing_markers(const int32_t *anchors, int64_t nanchors, int64_t n, int sampleRate, const mx_timing_params &p,
                                      const mx_marker *base, int nbase);

}  // namespace mx
