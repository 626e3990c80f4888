// key_logic.h — host logic of the key, scale and tuning estimate (key_logic.cpp, plain g++ -ffp-contract=off): the key from a
// 40-value chroma sum and from detected notes, the windows of a take, the correction markers on a tuned grid.  The
// definitions are include/melonix_amd.h's ("Key, scale and tuning reference"); tests/key_ref.py restates them operation for
// operation.  capi_key.cpp checks the arguments and hands over.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/melonix_amd.h"

namespace mx {

mx_key key_from_sum(const double *sum40);
// every note finite (the caller's check)
mx_key key_from_notes(const mx_note *notes, int64_t count);
// the {first_frame, frames} spans of mx_key_detect's windows over `count` frames (window_frames 0: none; window_hop >= 1)
std::vector<mx_chroma_job> key_windows(int64_t count, int64_t window_frames, int64_t window_hop);
void correction_markers_tuned(const mx_note *notes, int64_t count, double strength, int mask, double tuning_cents, mx_marker *out);

}  // namespace mx
