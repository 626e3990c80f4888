// compress_driver.cpp — melonix::Compressor and Mastering's compressed chain from a compiled program
// (tests/test_gpu_compress_facade.py):
//   compress_driver <in.f32> <sampleRate> <outRate> <target> <ceiling> <thresholdDb> <ratio> <kneeDb> <attackMs> <releaseMs>
//                   <lookaheadMs> <makeupDb> <out.f32> <reduction.f32> <chain.i16> <chain-at.i16> <chain.wav> <plain.i16> <plain-at.i16>
// reads raw float32 samples; writes apply()'s samples and reductionDb(), finishCompressedAt() at the take's rate and at outRate,
// the latter through exportWavCompressedAt() too, and the untouched finish() / finishAt(); its status says whether refused
// settings give empty results and leave the objects usable.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "compressor.hpp"
#include "driver_common.hpp"
#include "mastering.hpp"
#include "melonix_amd.h"

int main(int argc, char **argv) {
  if (argc != 20) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]), outRate = std::atoi(argv[3]);
  const double target = std::atof(argv[4]), ceiling = std::atof(argv[5]);
  melonix::CompressorSettings set;
  set.thresholdDb = std::atof(argv[6]), set.ratio = std::atof(argv[7]), set.kneeDb = std::atof(argv[8]);
  set.attackMs = std::atof(argv[9]), set.releaseMs = std::atof(argv[10]), set.lookaheadMs = std::atof(argv[11]);
  set.makeupDb = std::atof(argv[12]);
  melonix::Compressor comp(wav, sr);
  if (!comp.ok() || !comp.reductionDb().empty() || comp.stepSamples() != (sr + 500) / 1000) return 4;
  const std::vector<float> out = comp.apply(set);
  const std::vector<float> red = comp.reductionDb();
  if (out.size() != wav.size() || red.size() != (wav.size() + comp.stepSamples() - 1) / comp.stepSamples()) return 5;
  if (!dump(argv[13], out) || !dump(argv[14], red)) return 6;
  // refused settings: empty samples, an emptied curve; the next apply() gives the first one's results
  melonix::CompressorSettings bad = set;
  bad.ratio = 0.5;
  if (!comp.apply(bad).empty() || !comp.reductionDb().empty()) return 7;
  bad = set, bad.makeupDb = 30.0;
  if (!comp.apply(bad).empty()) return 7;
  bad = set, bad.thresholdDb = NAN;
  if (!comp.apply(bad).empty()) return 7;
  if (comp.apply(set) != out || comp.reductionDb() != red) return 8;
  const melonix::Compressor none(wav, 7999);
  if (none.ok()) return 9;
  // the defaults turn nothing up: no output sample is larger than its input
  melonix::Compressor plain(wav, sr);
  const std::vector<float> dflt = plain.apply(melonix::CompressorSettings{});
  if (dflt.size() != wav.size()) return 10;
  for (size_t i = 0; i < wav.size(); ++i)
    if (std::fabs(dflt[i]) > std::fabs(wav[i])) return 10;
  const melonix::Mastering master(wav, sr);
  if (!master.ok()) return 11;
  const std::vector<int16_t> chain = master.finishCompressedAt(sr, set, target, ceiling);
  const std::vector<int16_t> chainAt = master.finishCompressedAt(outRate, set, target, ceiling);
  if (chain.size() != wav.size() || (int64_t)chainAt.size() != mx_resample_length((int64_t)wav.size(), sr, outRate)) return 12;
  if (!dump(argv[15], chain) || !dump(argv[16], chainAt) || !master.exportWavCompressedAt(argv[17], outRate, set, target, ceiling)) return 13;
  if (!dump(argv[18], master.finish(target, ceiling)) || !dump(argv[19], master.finishAt(outRate, target, ceiling))) return 14;
  bad = set, bad.kneeDb = 25.0;
  if (!master.finishCompressedAt(sr, bad, target, ceiling).empty() || !master.finishCompressedAt(sr, set, NAN, ceiling).empty() ||
      !master.finishCompressedAt(sr, set, target, 0.5).empty() || !master.finishCompressedAt(7999, set, target, ceiling).empty() ||
      master.exportWavCompressedAt("/no/such/directory/out.wav", sr, set, target, ceiling))
    return 15;
  std::printf("%zu samples at %d Hz compressed, %zu steps\n", wav.size(), sr, red.size());
  return 0;
}
