// f0_notes.h — host logic of the f0 tracker's consumers (f0_notes.cpp, plain g++): notes cut from a YIN track and the
// correction markers that move them onto a pitch grid.  The definitions are include/melonix_amd.h's; capi_f0.cpp
// checks the arguments and hands over.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/melonix_amd.h"

namespace mx {

// the editor's note law at a period in samples: 24 + 12*log2(sr / period / 55)
double period_note(double period, int sampleRate);
std::vector<mx_note> detect_notes(const mx_f0 *track, int64_t count, int sampleRate, int hop, int64_t first_frame,
                                  const mx_note_params &p);
// nearest integer note whose pitch class (mod 12, A = 0) is in mask (bits 0..11, 0 = all), ties to the lower one
double snap_note(double note, int mask);
void correction_markers(const mx_note *notes, int64_t count, double strength, int mask, mx_marker *out);

}  // namespace mx
