// psola_plan.h — the host side of the PSOLA renderer (definition: include/melonix_amd.h): analysis and synthesis marks from
// an f0 track and the markers, as grain records for psola_kernels.hip; and the check the host-pointer entry point makes of
// records it is handed.  Pure host code like host_logic.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/melonix_amd.h"

namespace mx {

constexpr mx_psola_params kPsolaDefaults{0.15f, 1e-3f, 256.f};
// how far from its centre a grain's window may reach (MX_PSOLA_MAX_HALF + the centre's floor): what the kernel's search for
// the first grain of a tile relies on, and what the record check enforces
constexpr int kPsolaReach = MX_PSOLA_MAX_HALF + 1;
// the Q16 source step of a formant record: an octave either way
constexpr uint32_t kPsolaStepOne = 65536, kPsolaStepMin = kPsolaStepOne / 2, kPsolaStepMax = kPsolaStepOne * 2;

// Arguments checked (the f0 family's conventions), then the plan, one record per synthesis mark.  MX_OK, or MX_ERR_INVALID
// with `err` set.  bend: null, or `count` finite semitone values, one per frame of the track, that a voiced grain adds to the
// markers' bend at the frame its analysis mark reads (definition: "PSOLA follows a bend curve"); null leaves every operation
// of the plan as it was.
int build_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params &p,
                     const mx_marker *markers, int nmarkers, std::vector<mx_psola_grain> &grains, int64_t &nsamples,
                     std::string &err, const float *bend = nullptr);
// The same plan with the formant curve (definition: "Independent formant shift"): the same marks, each record with the Q16
// step of its analysis mark and the source position of its centre.  The curve is checked first.
int build_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params &p,
                     const mx_marker *markers, int nmarkers, const mx_formant_point *points, int npoints,
                     std::vector<mx_psola_fgrain> &fgrains, int64_t &nsamples, std::string &err, const float *bend = nullptr);

// The precondition of mx_psola_synth_dev / mx_psola_synth_formant_dev on `ngrains` records for an audio of n samples.  MX_OK,
// or MX_ERR_INVALID with `err`.
int check_psola_grains(const mx_psola_grain *g, int64_t ngrains, int64_t nsamples, int64_t n, std::string &err);
int check_psola_grains(const mx_psola_fgrain *g, int64_t ngrains, int64_t nsamples, int64_t n, std::string &err);

}  // namespace mx
