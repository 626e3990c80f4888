// loudness_driver.cpp — melonix::LoudnessTrack from a compiled program (tests/test_gpu_loudness_facade.py):
//   loudness_driver <in.f32> <sampleRate> <notes.bin> <target> <ceiling> <steps.bin> <summary.bin> <curves.f64> <lufs.f64>
//                   <levelled.f32> <normalized.f32>
// reads raw float32 samples and mx_note records, writes the records as mx_loud_step, the summary as one mx_loudness, the
// momentary curve followed by the short-term curve, the note loudness, and the levelled and the normalized take raw.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "loudness-track.hpp"
#include "melonix_amd.h"

int main(int argc, char **argv) {
  if (argc != 12) return 2;
  std::vector<float> wav, raw;
  if (!read_f32(argv[1], wav) || !read_f32(argv[3], raw)) return 3;
  const int sr = std::atoi(argv[2]);
  const float target = (float)std::atof(argv[4]), ceiling = (float)std::atof(argv[5]);
  const mx_note *first = reinterpret_cast<const mx_note *>(raw.data());
  const std::vector<mx_note> notes(first, first + raw.size() * sizeof(float) / sizeof(mx_note));
  melonix::LoudnessTrack track(wav, sr);
  if (!track.ok() || track.steps().empty()) return 4;
  std::vector<double> curves = track.momentary();
  const std::vector<double> slow = track.shortTerm(), lufs = track.noteLoudness(notes);
  if (curves.size() != track.steps().size() || slow.size() != curves.size() || lufs.size() != notes.size()) return 5;
  curves.insert(curves.end(), slow.begin(), slow.end());
  const std::vector<float> lev = track.levelled(notes), norm = track.normalized(target, ceiling);
  if (lev.size() != wav.size() || norm.size() != wav.size()) return 6;
  if (!dump(argv[6], track.steps()) || !dump(argv[7], std::vector<mx_loudness>{track.summary()}) || !dump(argv[8], curves) ||
      !dump(argv[9], lufs) || !dump(argv[10], lev) || !dump(argv[11], norm))
    return 7;
  // a failed call gives empty results: notes out of order, a note beyond the take, parameters out of range, a target that is no number
  std::vector<mx_note> swapped(notes.rbegin(), notes.rend());
  if (notes.size() > 1 && !track.levelled(swapped).empty()) return 8;
  std::vector<mx_note> beyond = notes;
  beyond.back().end_sample = (int32_t)wav.size();
  if (!track.noteLoudness(beyond).empty() || !track.levelled(beyond).empty()) return 9;
  mx_level_params p = melonix::LoudnessTrack::params();
  p.max_db = 41.0;
  if (!track.levelled(notes, p).empty() || !track.normalized(NAN, ceiling).empty()) return 10;
  p = melonix::LoudnessTrack::params();
  p.raise = p.lower = 0.0;
  if (track.levelled(notes, p) != wav) return 11;  // (every gain 1: the take itself)
  // after a failed construction ok() is false and the accessors are empty
  const melonix::LoudnessTrack none(wav, 7999);
  if (none.ok() || !none.steps().empty() || !none.momentary().empty() || !none.shortTerm().empty() || !none.noteLoudness(notes).empty() ||
      !none.levelled(notes).empty() || !none.normalized(target, ceiling).empty() || none.summary().blocks != 0)
    return 12;
  const std::vector<float> silence(wav.size(), 0.f);
  const melonix::LoudnessTrack quiet(silence, sr);
  if (!quiet.ok() || !quiet.normalized(target, ceiling).empty()) return 13;  // (no loudness to normalise)
  std::printf("%zu steps, %zu notes, integrated %.4f LUFS\n", track.steps().size(), notes.size(), track.summary().integrated);
  return 0;
}
