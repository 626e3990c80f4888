// onset_driver.cpp — melonix::OnsetTrack from a compiled program (tests/test_gpu_onset_facade.py):
//   onset_driver <in.f32> <sampleRate> <bpm> <division> <with base 0|1> <flux.f32> <onsets.bin> <markers.bin>
// reads raw float32 samples, writes the onset strength raw, the onsets as mx_onset records and the timing markers as mx_marker
// records.  With a base, two markers of a constant +1 st bend (samples 1000 and n - 1000) are merged in.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "melonix_amd.h"
#include "onset-track.hpp"

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]);
  melonix::OnsetTrack track(wav, sr);
  if (!track.ok()) return 4;
  mx_timing_params tp = melonix::OnsetTrack::timingParams();
  tp.bpm = std::atof(argv[3]);
  tp.division = std::atoi(argv[4]);
  std::vector<Marker> base;
  if (std::atoi(argv[5])) base = {{1000, 45.0, 0.0, 1.0}, {(int)wav.size() - 1000, 45.0, 0.0, 1.0}};
  const std::vector<mx_onset> on = track.onsets();
  const std::vector<Marker> mk = track.timingMarkers(tp, base);
  if (on.empty() || mk.empty()) return 5;
  if (!dump(argv[6], track.flux()) || !dump(argv[7], on) || !dump(argv[8], mk)) return 6;
  // a failed call gives empty results: a base marker with a shift of its own is refused, and so is a tempo off the slider
  const std::vector<Marker> bad = {{1000, 45.0, 0.5, 0.0}};
  if (!track.timingMarkers(tp, bad).empty()) return 7;
  tp.bpm = 10.0;
  if (!track.timingMarkers(tp).empty()) return 8;
  if (melonix::OnsetTrack(wav, sr, 0).ok()) return 9;
  std::printf("%zu frames, %zu onsets, %zu markers\n", track.flux().size(), on.size(), mk.size());
  return 0;
}
