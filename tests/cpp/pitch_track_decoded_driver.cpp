// pitch_track_decoded_driver.cpp — melonix::PitchTrack's `decoded` option from a compiled program
// (tests/test_gpu_f0_decode.py):
//   pitch_track_decoded_driver <in.f32> <sampleRate> <decoded 0|1> <out.frames>
// reads raw float32 samples, writes frames() as raw mx_f0 records and prints the number of notes() on its last line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "pitch-track.hpp"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  melonix::PitchTrack track(wav, std::atoi(argv[2]), 256, 55.f, 1760.f, 0.15f, 0, std::atoi(argv[3]) != 0);
  if (!track.ok()) return 4;
  if (!dump(argv[4], track.frames())) return 5;
  std::printf("notes %zu\n", track.notes().size());
  return 0;
}
