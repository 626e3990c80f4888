// psola_driver.cpp — melonix::PitchTrack + melonix::Resynth::renderPSOLA / exportWavPSOLA from a compiled program
// (tests/test_gpu_psola_facade.py, tests/test_gpu_psola_formant_facade.py):
//   psola_driver plain   <in.f32> <sampleRate> <bend> <decoded 0|1> <out.f32> <out.wav>
//   psola_driver formant <in.f32> <sampleRate> <bend> <formant0> <formant1> <out.f32> <out.wav>
// reads raw float32 samples, tracks them, renders them retuned by a constant <bend> semitones, writes the float PCM raw and
// the int16 PCM through saveWav.  plain: with the track's own voicing parameters; formant: through the overloads that take
// formant points, the envelope moved along a ramp from <formant0> at sample 0 to <formant1> at the last sample.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "driver_common.hpp"
#include "melonix_amd.h"
#include "pitch-track.hpp"
#include "resynth.hpp"

int main(int argc, char **argv) {
  const bool formant = argc == 9 && !std::strcmp(argv[1], "formant");
  if (!formant && !(argc == 8 && !std::strcmp(argv[1], "plain"))) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[2], wav)) return 3;
  const int sr = std::atoi(argv[3]);
  const double bend = std::atof(argv[4]);
  melonix::PitchTrack track(wav, sr, 256, 55.f, 1760.f, 0.15f, 0, !formant && std::atoi(argv[5]) != 0);
  if (!track.ok()) return 4;
  melonix::Resynth rs(wav, sr);
  if (!rs.ok()) return 5;
  const std::vector<Marker> mk = {{1, 0, 0, bend}, {(int)wav.size() - 1, 0, 0, bend}};
  const mx_psola_params p = track.psolaParams();
  std::vector<mx_formant_point> pts;
  if (formant) pts = {{0, (float)std::atof(argv[5])}, {(int32_t)wav.size() - 1, (float)std::atof(argv[6])}};
  const std::vector<float> pcm =
      formant ? rs.renderPSOLA(mk, track.frames(), track.hop(), pts) : rs.renderPSOLA(mk, track.frames(), track.hop(), &p);
  if (pcm.empty()) return 6;
  if (!dump(argv[argc - 2], pcm)) return 7;
  if (!(formant ? rs.exportWavPSOLA(argv[argc - 1], mk, track.frames(), track.hop(), pts)
                : rs.exportWavPSOLA(argv[argc - 1], mk, track.frames(), track.hop(), &p)))
    return 8;
  if (!formant) {
    // a track that does not fit the file is refused: an empty vector, no file
    std::vector<mx_f0> shortTrack(track.frames().begin(), track.frames().end() - 1);
    if (!rs.renderPSOLA(mk, shortTrack, track.hop()).empty()) return 9;
    std::printf("%zu frames, %zu samples, threshold %g\n", track.frames().size(), pcm.size(), (double)p.threshold);
    return 0;
  }
  // no points: the plain overload's samples
  if (rs.renderPSOLA(mk, track.frames(), track.hop(), std::vector<mx_formant_point>()) != rs.renderPSOLA(mk, track.frames(), track.hop()))
    return 9;
  // a curve whose samples do not increase is refused: an empty vector, no file
  const std::vector<mx_formant_point> bad = {{100, 1.f}, {100, 2.f}};
  if (!rs.renderPSOLA(mk, track.frames(), track.hop(), bad).empty()) return 10;
  std::printf("%zu frames, %zu samples, %zu points\n", track.frames().size(), pcm.size(), pts.size());
  return 0;
}
