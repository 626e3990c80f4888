// denoise_driver.cpp — melonix::NoiseReduction from a compiled program (tests/test_gpu_denoise_facade.py):
//   denoise_driver <in.f32> <sampleRate> <begin> <end> <reductionDb> <sensitivityDb> <print.f32> <out.f32>
// reads raw float32 samples, learns the print of [begin, end), writes the print and the cleaned samples raw; its status says
// whether a set print gives the learned print's samples, and whether refused regions, prints and parameters give false / empty
// results and leave the print alone.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "melonix_amd.h"
#include "noise-reduction.hpp"

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]);
  const long long begin = std::atoll(argv[3]), end = std::atoll(argv[4]);
  const double red = std::atof(argv[5]), sens = std::atof(argv[6]);
  melonix::NoiseReduction clean(wav, sr);
  if (!clean.ok() || !clean.print().empty() || !clean.apply(red, sens).empty()) return 4;
  if (!clean.learn(begin, end) || clean.print().size() != MX_DENOISE_BINS) return 5;
  const std::vector<float> print = clean.print(), out = clean.apply(red, sens);
  if (out.size() != wav.size() || !dump(argv[7], print) || !dump(argv[8], out)) return 6;
  // refused regions, prints and parameters leave the print alone
  if (clean.learn(0, 1023) || clean.learn(-1, 4096) || clean.learn(0, (long long)wav.size() + 1) || clean.print() != print) return 7;
  std::vector<float> bad = print;
  bad[7] = -1.f;
  if (clean.setPrint(bad) || clean.setPrint(std::span<const float>(print.data(), 512)) || clean.print() != print) return 8;
  bad[7] = NAN;
  if (clean.setPrint(bad) || !clean.apply(61.0, sens).empty() || !clean.apply(red, 25.0).empty() || !clean.apply(NAN, sens).empty()) return 9;
  // a set print gives the learned print's samples, from another object too
  melonix::NoiseReduction other(wav, sr);
  if (!other.ok() || !other.setPrint(print) || other.apply(red, sens) != out || clean.apply(red, sens) != out) return 10;
  std::printf("%zu samples at %d Hz cleaned\n", wav.size(), sr);
  return 0;
}
