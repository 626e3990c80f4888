// mastering_driver.cpp — melonix::Mastering from a compiled program (tests/test_gpu_mastering_facade.py):
//   mastering_driver <in.f32> <sampleRate> <target> <ceiling> <lookahead ms> <pcm.i16> <out.wav> <peaks.bin> <summary.bin>
// reads raw float32 samples, writes finish()'s int16 raw, the same through exportWav(), the true-peak records as mx_tp_step,
// and one mx_loudness followed by one mx_loudness_range_result and the two peaks (2 floats).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "driver_common.hpp"
#include "mastering.hpp"
#include "melonix_amd.h"

int main(int argc, char **argv) {
  if (argc != 10) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]);
  const double target = std::atof(argv[3]), ceiling = std::atof(argv[4]), ms = std::atof(argv[5]);
  const melonix::Mastering master(wav, sr);
  if (!master.ok() || master.peaks().empty()) return 4;
  const std::vector<int16_t> pcm = master.finish(target, ceiling, ms);
  if (pcm.size() != wav.size()) return 5;
  if (!dump(argv[6], pcm) || !master.exportWav(argv[7], target, ceiling, ms) || !dump(argv[8], master.peaks())) return 6;
  std::vector<unsigned char> summary(sizeof(mx_loudness) + sizeof(mx_loudness_range_result) + 2 * sizeof(float));
  const float both[2] = {master.truePeak(), master.samplePeak()};
  std::memcpy(summary.data(), &master.loudness(), sizeof(mx_loudness));
  std::memcpy(summary.data() + sizeof(mx_loudness), &master.range(), sizeof(mx_loudness_range_result));
  std::memcpy(summary.data() + sizeof(mx_loudness) + sizeof(mx_loudness_range_result), both, sizeof(both));
  if (!dump(argv[9], summary)) return 7;
  // a failed call gives empty results: a target or a ceiling that is no number, a ceiling above full scale, a path that cannot be written
  if (!master.finish(NAN, ceiling, ms).empty() || !master.finish(target, NAN, ms).empty() || !master.finish(target, 0.5, ms).empty()) return 8;
  if (master.exportWav("/no/such/directory/out.wav", target, ceiling, ms)) return 9;
  // any look-ahead is brought into [1, 1024] samples
  if (master.finish(target, ceiling, 1e-6).size() != wav.size() || master.finish(target, ceiling, 1e6).size() != wav.size()) return 10;
  // after a failed construction ok() is false and the accessors are empty
  const melonix::Mastering none(wav, 7999);
  if (none.ok() || !none.peaks().empty() || !none.finish(target, ceiling).empty() || none.exportWav(argv[7], target, ceiling) ||
      none.loudness().blocks != 0 || none.range().values != 0 || none.truePeak() != 0.f || !std::isinf(none.truePeakDb()))
    return 11;
  const std::vector<float> silence(wav.size(), 0.f);
  const melonix::Mastering quiet(silence, sr);
  if (!quiet.ok() || quiet.truePeak() != 0.f || !quiet.finish(target, ceiling).empty()) return 12;  // (no loudness to normalise)
  std::printf("%zu steps, integrated %.4f LUFS, true peak %.4f dBTP, range %.4f LU\n", master.peaks().size(), master.loudness().integrated,
              master.truePeakDb(), master.range().lra);
  return 0;
}
