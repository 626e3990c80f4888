// resample_driver.cpp — melonix::Mastering's export at another rate from a compiled program (tests/test_gpu_resample_facade.py):
//   resample_driver <in.f32> <sampleRate> <outRate> <target> <ceiling> <pcm.i16> <out.wav>
// reads raw float32 samples, writes finishAt()'s int16 raw and the same through exportWavAt(); its status says whether finishAt()
// at the take's own rate is finish(), and whether a refused rate pair gives empty results.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "mastering.hpp"
#include "melonix_amd.h"

int main(int argc, char **argv) {
  if (argc != 8) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]), outRate = std::atoi(argv[3]);
  const double target = std::atof(argv[4]), ceiling = std::atof(argv[5]);
  const melonix::Mastering master(wav, sr);
  if (!master.ok()) return 4;
  const std::vector<int16_t> pcm = master.finishAt(outRate, target, ceiling);
  if ((int64_t)pcm.size() != mx_resample_length((int64_t)wav.size(), sr, outRate)) return 5;
  if (!dump(argv[6], pcm) || !master.exportWavAt(argv[7], outRate, target, ceiling)) return 6;
  // at the take's own rate: finish(), with the default and with a given look-ahead
  const std::vector<int16_t> same = master.finish(target, ceiling);
  if (same.size() != wav.size() || master.finishAt(sr, target, ceiling) != same) return 7;
  if (master.finishAt(sr, target, ceiling, 2.5) != master.finish(target, ceiling, 2.5)) return 8;
  // a rate pair the conversion refuses gives empty results and no file
  if (!master.finishAt(7999, target, ceiling).empty() || !master.finishAt(48001, target, ceiling).empty() ||
      master.exportWavAt(argv[7], 384001, target, ceiling))
    return 9;
  const melonix::Mastering none(wav, 7999);
  if (none.ok() || !none.finishAt(outRate, target, ceiling).empty() || none.exportWavAt(argv[7], outRate, target, ceiling)) return 10;
  std::printf("%zu samples at %d Hz -> %zu at %d Hz\n", wav.size(), sr, pcm.size(), outRate);
  return 0;
}
