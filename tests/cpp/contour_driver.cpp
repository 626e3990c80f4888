// contour_driver.cpp — melonix::PitchContour from a compiled program (tests/test_gpu_contour_facade.py):
//   contour_driver <in.f32> <sampleRate> <drift> <vibrato> <track.bin> <notes.bin> <rec.bin> <stat.bin> <vibrato.bin> <bend.bin> <pcm.f32>
// reads raw float32 samples, writes the decoded track, the notes, the contour records, the per-note statistics and vibrato
// figures, the bend curve for (drift, vibrato) with every note moved to the nearest semitone, and the take rendered along it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "melonix_amd.h"
#include "pitch-contour.hpp"

int main(int argc, char **argv) {
  if (argc != 12) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]);
  const float drift = (float)std::atof(argv[3]), vibrato = (float)std::atof(argv[4]);
  const melonix::PitchContour contour(wav, sr);
  if (!contour.ok() || contour.notes().empty()) return 4;
  std::vector<double> shift;
  for (const mx_note &n : contour.notes()) shift.push_back(std::rint(n.note) - n.note);
  const std::vector<float> bend = contour.bend(drift, vibrato, shift);
  const std::vector<float> pcm = contour.correct(drift, vibrato, shift);
  if (bend.size() != contour.frames().size() || pcm.size() + 1 != wav.size()) return 5;
  if (contour.contour().size() != contour.frames().size() || contour.stats().size() != contour.notes().size() ||
      contour.vibrato().size() != contour.notes().size())
    return 5;
  if (!dump(argv[5], contour.frames()) || !dump(argv[6], contour.notes()) || !dump(argv[7], contour.contour()) ||
      !dump(argv[8], contour.stats()) || !dump(argv[9], contour.vibrato()) || !dump(argv[10], bend) || !dump(argv[11], pcm))
    return 6;
  // a failed call gives empty results: parameters out of range, a shift that is not one per note or not finite
  if (!contour.bend(1.5f, 1.f).empty() || !contour.bend(1.f, 4.5f).empty() || !contour.bend(1.f, 1.f, {}, -1).empty()) return 7;
  std::vector<double> more(shift);
  more.push_back(0.0);
  if (!contour.bend(1.f, 1.f, more).empty() || !contour.correct(1.f, 1.f, more).empty()) return 8;
  shift[0] = NAN;
  if (!contour.bend(1.f, 1.f, shift).empty() || !contour.correct(1.f, 1.f, shift).empty()) return 9;
  for (const melonix::PitchContour &none : {melonix::PitchContour(wav, 0), melonix::PitchContour(wav, sr, 0)})
    if (none.ok() || !none.frames().empty() || !none.notes().empty() || !none.contour().empty() || !none.stats().empty() ||
        !none.vibrato().empty() || !none.bend(1.f, 1.f).empty() || !none.correct(1.f, 1.f).empty())
      return 10;
  // silence: a track and no notes, a zero curve, the input back
  const std::vector<float> quiet(20000, 0.f);
  const melonix::PitchContour silent(quiet, sr);
  if (!silent.ok() || !silent.notes().empty() || silent.bend(1.f, 0.f).size() != silent.frames().size() ||
      silent.correct(1.f, 0.f).size() != quiet.size() - 1)
    return 11;
  std::printf("%zu frames, %zu notes, extent %.2f drift %.2f\n", contour.frames().size(), contour.notes().size(),
              contour.vibrato()[0].extent_cents, contour.vibrato()[0].drift_cents);
  return 0;
}
