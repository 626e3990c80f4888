// sibilant_driver.cpp — melonix::SibilantTrack from a compiled program (tests/test_gpu_sibilant_facade.py):
//   sibilant_driver <in.f32> <sampleRate> <db> <ramp> <features.bin> <sibilants.bin> <curve.bin> <balanced.f32>
// reads raw float32 samples, writes the features as mx_sib_feat records, the segments as mx_sibilant records, the protected
// form of a fixed curve ({0, +4 st}, {n / 2, +2 st}, {n - 1, -3 st}) as mx_formant_point records and the balanced take raw.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "melonix_amd.h"
#include "sibilant-track.hpp"

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]), ramp = std::atoi(argv[4]), n = (int)wav.size();
  const float db = (float)std::atof(argv[3]);
  melonix::SibilantTrack track(wav, sr);
  if (!track.ok()) return 4;
  const std::vector<mx_formant_point> curve = {{0, 4.f}, {n / 2, 2.f}, {n - 1, -3.f}};
  const std::vector<mx_sibilant> sibs = track.sibilants();
  const std::vector<mx_formant_point> prot = track.protect(curve, ramp);
  const std::vector<float> bal = track.balanced(db, ramp);
  if (sibs.empty() || prot.empty() || bal.size() != wav.size()) return 5;
  if (!dump(argv[5], track.features()) || !dump(argv[6], sibs) || !dump(argv[7], prot) || !dump(argv[8], bal)) return 6;
  // a failed call gives empty results: no ramp, a curve out of order, a balance off the scale, parameters out of range
  if (!track.protect(curve, 0).empty() || !track.balanced(db, 0).empty()) return 7;
  if (!track.protect({{100, 1.f}, {100, 2.f}}, ramp).empty() || !track.balanced(500.f, ramp).empty()) return 8;
  mx_sibilant_params p = melonix::SibilantTrack::params();
  p.min_frames = 0;
  if (!track.sibilants(p).empty()) return 9;
  if (!track.protect({}, ramp).empty()) return 10;  // (an empty curve stays empty)
  const melonix::SibilantTrack none(wav, sr, 0);
  if (none.ok() || !none.features().empty() || !none.sibilants().empty() || !none.protect(curve, ramp).empty() || !none.balanced(db, ramp).empty())
    return 11;
  std::printf("%zu frames, %zu sibilants, %zu curve points\n", track.features().size(), sibs.size(), prot.size());
  return 0;
}
