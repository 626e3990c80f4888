// compressor.hpp — NOT in the reference (app.cpp exports what process() wrote): the dynamics compressor over the build-defined
// entry points (mx_audio_compress, mx_compress_gain), the step between note levelling and the limiter, and its gain-reduction
// curve, the meter an editor draws — as a class the App can own next to its melonix::Mastering.
//
//   melonix::Compressor comp(rendered, sampleRate);           // uploads once
//   melonix::CompressorSettings set;                          // -18 dB, 4 : 1, a 6 dB knee, 5 ms / 100 ms
//   set.makeupDb = 3.0;
//   std::vector<float> take = comp.apply(set);                // hand it to Mastering in place of the render
//   meter->draw(comp.reductionDb(), comp.stepSamples());      // dB per control step of about 1 ms, 0 = no reduction
//
// The whole export chain with dynamics is Mastering::finishCompressedAt / exportWavCompressedAt.  A render that is already on
// the device needs no round trip: mx_audio_compress gives the audio object the meter, the gain and the limiter take.
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

// In dB and ms, as an editor shows them; makeupDb in [-24.08, 24.08] (the library takes an amplitude in [1/16, 16]).
struct CompressorSettings {
  double thresholdDb = -18.0, ratio = 4.0, kneeDb = 6.0, attackMs = 5.0, releaseMs = 100.0, lookaheadMs = 0.0, makeupDb = 0.0;
};
// The library's parameters of `s`: the make-up gain as the amplitude (float)10^(makeupDb / 20).  false for a value that is no
// number; the ranges are the library's to check.
bool compressParams(const CompressorSettings &s, mx_compress_params &out);

class Compressor {
public:
  // sampleRate in [8000, 384000]
  Compressor(std::span<const float> wav, int sampleRate, int device = 0);
  ~Compressor();
  Compressor(const Compressor &) = delete;
  Compressor &operator=(const Compressor &) = delete;

  bool ok() const { return good; }
  int sampleRate() const { return sampleRate_; }
  // D: the samples of a control step, (sampleRate + 500) / 1000
  int stepSamples() const { return (sampleRate_ + 500) / 1000; }
  // The compressed samples, and the curve reductionDb() then returns.  Empty, and the curve emptied, after a failed call:
  // settings outside the library's ranges.
  std::vector<float> apply(const CompressorSettings &settings);
  // The smoothed gain of the last apply() per control step, 20 log10(s_b / 2^30) dB: 0 where nothing is turned down, negative
  // where it is.  Empty before the first apply().
  const std::vector<float> &reductionDb() const { return reduction_; }

private:
  int sampleRate_;
  bool good = false;
  int64_t n = 0;
  std::unique_ptr<glue::Session> session;
  std::vector<float> reduction_;
};

}  // namespace melonix
