// tempo_driver.cpp — melonix::OnsetTrack::tempo / tempoWindows from a compiled program (tests/test_gpu_tempo_facade.py):
//   tempo_driver <in.f32> <sampleRate> <tempo.bin> <windows.bin>
// reads raw float32 samples, writes the estimate as one mx_tempo record and the window curve as mx_tempo_window records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "melonix_amd.h"
#include "onset-track.hpp"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]);
  melonix::OnsetTrack track(wav, sr);
  if (!track.ok()) return 4;
  const std::vector<mx_tempo> t = {track.tempo()};
  const std::vector<mx_tempo_window> win = track.tempoWindows();
  if (!(t[0].bpm > 0.0) || win.empty()) return 5;
  if (!dump(argv[3], t) || !dump(argv[4], win)) return 6;
  // one run gives both
  mx_tempo t1;
  std::vector<mx_tempo_window> win1;
  if (!track.estimate(melonix::OnsetTrack::tempoParams(), t1, &win1) || t1.bpm != t[0].bpm || t1.offset != t[0].offset ||
      win1.size() != win.size())
    return 11;
  // the estimate drives the grid: the usage of onset-track.hpp
  mx_timing_params tp = melonix::OnsetTrack::timingParams();
  tp.bpm = t[0].bpm;
  tp.offset = t[0].offset;
  if (track.timingMarkers(tp).empty()) return 7;
  // a failed call gives a zeroed estimate and an empty curve: a parameter out of its range
  mx_tempo_params bad = melonix::OnsetTrack::tempoParams();
  bad.per_octave = 7;
  const mx_tempo z = track.tempo(bad);
  if (z.bpm != 0.0 || z.offset != 0.0 || z.score != 0.f || z.clarity != 0.f || z.locked_frames != 0 || z.levels != 0) return 8;
  if (!track.tempoWindows(bad).empty()) return 9;
  // silence: no error, and no pulse
  const std::vector<float> quiet(wav.size(), 0.f);
  melonix::OnsetTrack still(quiet, sr);
  if (!still.ok() || still.tempo().bpm != 0.0 || !still.tempoWindows().empty()) return 10;
  std::printf("%.6f bpm, offset %.6f s, clarity %.3f, %zu windows, %d levels\n", t[0].bpm, t[0].offset, (double)t[0].clarity, win.size(),
              t[0].levels);
  return 0;
}
