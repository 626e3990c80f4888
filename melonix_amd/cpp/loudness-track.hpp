// loudness-track.hpp — NOT in the reference (it has no meter): the build-defined BS.1770 loudness records (mx_loudness_steps),
// the gated, momentary and short-term loudness from them, the loudness of each note, and the two level macros applied to the
// source (mx_level_gain_points / mx_normalize_gain, mx_audio_gain), as a class the App can own next to its melonix::PitchTrack.
//
//   melonix::LoudnessTrack loud(wavData, sampleRate);       // uploads once, the 10 ms records of the whole take on the GPU
//   meter->show(loud.summary().integrated, loud.momentary());        // LUFS, and the curve under the waveform
//   auto even = loud.levelled(track.notes());               // "Level notes": every note moved to the take's median loudness ...
//   resynth = std::make_unique<melonix::Resynth>(even, sampleRate);  // ... as the source of any renderer; the f0 track stays valid
//   auto out = loud.normalized(-14.f, -1.f);                // export at -14 LUFS, sample peak at most -1 dBFS
#pragma once
#include <cstdint>
#include <span>
#include <vector>

#include "melonix_amd.h"

namespace melonix {

class LoudnessTrack {
public:
  // The samples are kept (levelled(), normalized()).  sampleRate in [8000, 384000].
  LoudnessTrack(std::span<const float> wav, int sampleRate, int device = 0);

  bool ok() const { return good; }
  // the record of step b (samples [b * S, (b + 1) * S), S = (sampleRate + 50) / 100); empty after a failed construction
  const std::vector<mx_loud_step> &steps() const { return steps_; }
  // integrated loudness with its gate counts, the largest momentary and short-term values, the sample peak; zeros after a failed
  // construction
  const mx_loudness &summary() const { return summary_; }
  // LUFS per step over the 400 ms / 3 s that end with it (-inf until the window is full); empty after a failed call
  std::vector<double> momentary() const { return curve(40); }
  std::vector<double> shortTerm() const { return curve(300); }
  // LUFS per note; empty after a failed call
  std::vector<double> noteLoudness(const std::vector<mx_note> &notes) const;
  // the defaults (mx_level_params_default), to edit and pass on
  static mx_level_params params();
  // the take with every note moved towards the median note loudness (mx_audio_gain on the GPU); empty after a failed call
  std::vector<float> levelled(const std::vector<mx_note> &notes) const { return levelled(notes, params()); }
  std::vector<float> levelled(const std::vector<mx_note> &notes, const mx_level_params &p) const;
  // the take at targetLufs, its sample peak at most ceilingDb dBFS; empty after a failed call (a silent take has no loudness)
  std::vector<float> normalized(float targetLufs, float ceilingDb) const;

private:
  std::vector<double> curve(int window) const;
  std::vector<float> gained(const std::vector<mx_gain_point> &points) const;

  int sampleRate, device_;
  bool good = false;
  std::vector<float> wav_;
  std::vector<mx_loud_step> steps_;
  mx_loudness summary_{};
};

}  // namespace melonix
