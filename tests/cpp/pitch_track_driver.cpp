// pitch_track_driver.cpp — melonix::PitchTrack from a compiled program (tests/test_gpu_pitch_track.py):
//   pitch_track_driver <in.f32> <sampleRate> <scaleMask> <out.markers>
// reads raw float32 samples, writes correctionMarkers(1, scaleMask) as raw Marker records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "pitch-track.hpp"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  melonix::PitchTrack track(wav, std::atoi(argv[2]));
  if (!track.ok()) return 4;
  const std::vector<Marker> mk = track.correctionMarkers(1.f, std::atoi(argv[3]));
  if (!dump(argv[4], mk)) return 5;
  std::printf("%zu frames, %zu markers\n", track.frames().size(), mk.size());
  return mk.empty() ? 6 : 0;
}
