// sibilant-track.hpp — NOT in the reference (it has no notion of a consonant): the build-defined sibilant detector
// (mx_sib_features, mx_sibilants), the formant curve that leaves sibilants alone (mx_formant_protect) and the sibilant balance
// applied to the source (mx_sibilant_gain_points, mx_audio_gain), as a class the App can own next to its melonix::PitchTrack.
//
//   melonix::SibilantTrack sib(wavData, sampleRate);        // uploads once, the features of every frame (hop 256) on the GPU
//   formant = sib.protect(formant, sampleRate / 100);       // "Protect sibilants": the formant knobs skip every "s", 10 ms ramps
//   resynth->exportWavPSOLA(fileName, markers, track.frames(), track.hop(), formant, &p);
//   auto balanced = sib.balanced(-6.f, sampleRate / 100);   // "Sibilant balance": the take with every "s" 6 dB down ...
//   resynth = std::make_unique<melonix::Resynth>(balanced, sampleRate);   // ... as the source of any renderer; the f0 track stays valid
#pragma once
#include <cstdint>
#include <span>
#include <vector>

#include "melonix_amd.h"

namespace melonix {

class SibilantTrack {
public:
  // hop: samples between frame centres.  The feature parameters are the library's defaults.  The samples are kept (balanced()).
  SibilantTrack(std::span<const float> wav, int sampleRate, int hop = 256, int device = 0);

  bool ok() const { return good; }
  int hop() const { return hop_; }
  // the record of frame h (centred on sample h * hop); empty after a failed call
  const std::vector<mx_sib_feat> &features() const { return feat_; }
  // the defaults (mx_sibilant_params_default), to edit and pass on
  static mx_sibilant_params params();
  // the segments of features(); empty after a failed call
  std::vector<mx_sibilant> sibilants() const { return sibilants(params()); }
  std::vector<mx_sibilant> sibilants(const mx_sibilant_params &p) const;
  // `curve` held at 0 st across sibilants(), rampSamples of linear return either side: what the formant overloads of
  // renderPSOLA / exportWavPSOLA take.  Empty after a failed call (and for an empty curve).
  std::vector<mx_formant_point> protect(const std::vector<mx_formant_point> &curve, int rampSamples) const;
  // the take with sibilants() turned by db decibels (mx_audio_gain on the GPU); empty after a failed call
  std::vector<float> balanced(float db, int rampSamples) const;

private:
  int sampleRate, hop_, device_;
  bool good = false;
  std::vector<float> wav_;
  std::vector<mx_sib_feat> feat_;
};

}  // namespace melonix
