// loudness_logic.h — host logic behind the loudness entry points (loudness_logic.cpp, plain g++, binary64, no contraction): the
// K-weighting coefficients, the windowed curve, BS.1770 gating, the loudness range, note loudness, the levelling points and the export gain.  The
// definitions are include/melonix_amd.h's ("Loudness and note levelling"); capi_loudness.cpp checks the plain arguments.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"

namespace mx {

// {b0, b1, b2, a1, a2} of the shelf, then of the high-pass, for a sample rate in range
void loudness_coeffs(int sr, double out[10]);
// The check of a record list at step length S: nullptr, or what is wrong (static text).
const char *loud_steps_error(const mx_loud_step *steps, int64_t nsteps, int S);
// Lists that passed that check, S the step length, window >= 1.
void loudness_curve(const mx_loud_step *steps, int64_t nsteps, int S, int window, double *out);
void loudness_integrated(const mx_loud_step *steps, int64_t nsteps, int S, mx_loudness *out);
// EBU Tech 3342 over the 3 s mean squares every 100 ms (definition: the header's "True peak, limiter and loudness range")
void loudness_range(const mx_loud_step *steps, int64_t nsteps, int S, mx_loudness_range_result *out);
// false: note `*bad` starts before the file, ends before it starts, or ends beyond the samples the records cover
bool note_loudness(const mx_loud_step *steps, int64_t nsteps, int S, const mx_note *notes, int64_t nnotes, double *lufs, int64_t *bad);
// notes in order, parameters in range; -> the reference
double level_gain_points(const mx_note *notes, int64_t nnotes, const double *lufs, const mx_level_params &p, mx_gain_point *out);
double normalize_amp(double integrated, double peak, double target_lufs, double ceiling_db);

}  // namespace mx
