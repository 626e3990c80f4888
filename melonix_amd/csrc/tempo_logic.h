// tempo_logic.h — host logic behind the tempo entry points (tempo_logic.cpp, plain g++, binary64, libm, no contraction): the
// smoothing weights, the argument checks, the candidate ladder and the estimate itself — coarse windows, refinement levels,
// result — over a comb it is handed (the kernel in the library, tempo_core.h on the CPU in tests/emu/tempo_emu.cpp).  The
// definition is include/melonix_amd.h's ("Tempo and grid-offset estimation"); capi_tempo.cpp owns the device memory.
#pragma once
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/melonix_amd.h"
#include "tempo_core.h"

namespace mx {

extern const mx_tempo_params kTempoDefaults;

// h_|d| of half-width W in [0, 32]
tempo::SmoothWeights smooth_weights(int W);

// What is wrong with the argument, or null: the words of the MX_ERR_INVALID the entry points return.
const char *tempo_params_error(const mx_tempo_params &p);
const char *comb_job_error(const mx_comb_job &job, int64_t count);

// The candidate ladder of a parameter block at sr / hop frames per second.
struct TempoLadder {
  double fr = 0.0;
  std::vector<double> bpm, prior;
  std::vector<uint32_t> period;
};
// null, or what is wrong: sr, hop, or a period outside the Q16 range.  p in range (tempo_params_error).
const char *tempo_ladder(const mx_tempo_params &p, int sampleRate, int hop, TempoLadder &out);

// jobs -> one record each (the vector arrives sized); a status other than 0 ends the estimate and is returned
using CombRunner = std::function<int(const std::vector<mx_comb_job> &, std::vector<mx_comb> &)>;

// The estimate over the smoothed curve e[0, count) whose frame 0 is frame first_frame; count <= INT32_MAX, p and ladder checked.
int tempo_estimate(const float *e, int64_t count, int64_t first_frame, const mx_tempo_params &p, const TempoLadder &ladder,
                   const CombRunner &comb, mx_tempo &out, std::vector<mx_tempo_window> &windows);

}  // namespace mx
