// noise-reduction.hpp — NOT in the reference (app.cpp decodes to mono and edits what it got): spectral noise reduction from a noise
// print over the build-defined entry points (mx_noise_print, mx_audio_denoise), the step between loading a take and everything
// that analyses or renders it — as a class the App can own next to its Spec.
//
//   melonix::NoiseReduction clean(wav, sampleRate);          // uploads once
//   clean.learn(roomToneBegin, roomToneEnd);                 // the print of a stretch without signal, on the GPU
//   std::vector<float> take = clean.apply(12.0, 6.0);        // 12 dB down, 6 dB above the print: hand it to Spec, PitchTrack,
//                                                            // Resynth, Mastering in place of wav
//   save(clean.print());  ...  clean.setPrint(saved);        // a print outlives the take it was learned on
//
// A take that is already on the device needs no round trip: mx_audio_denoise gives the audio object every analyser and renderer
// takes as its source.
#pragma once
#include <cstdint>
#include <memory>
#include <span>
#include <vector>

#include "melonix_amd.h"

namespace melonix {

namespace glue {
struct Session;
}

class NoiseReduction {
public:
  // sampleRate is kept for the caller's book-keeping: the framing is in samples (N = 1024, hop 256) at every rate
  NoiseReduction(std::span<const float> wav, int sampleRate, int device = 0);
  ~NoiseReduction();
  NoiseReduction(const NoiseReduction &) = delete;
  NoiseReduction &operator=(const NoiseReduction &) = delete;

  bool ok() const { return good; }
  int sampleRate() const { return sampleRate_; }
  // The print of samples [beginSample, endSample): at least one whole frame of 1024 samples, at most 8192.  false, and the print
  // left as it was, for a region the library refuses.
  bool learn(int64_t beginSample, int64_t endSample);
  // A saved or synthetic print: MX_DENOISE_BINS finite values >= 0.  false, and the print left as it was, otherwise.
  bool setPrint(std::span<const float> print);
  // the print in force; empty before the first learn() / setPrint()
  const std::vector<float> &print() const { return print_; }
  // The cleaned samples: reductionDb in [0, 60], sensitivityDb in [-12, 24].  Empty after a failed call or without a print.
  std::vector<float> apply(double reductionDb, double sensitivityDb) const;

private:
  int sampleRate_;
  bool good = false;
  int64_t n = 0;
  std::unique_ptr<glue::Session> session;
  std::vector<float> print_;
};

}  // namespace melonix
