// mastering.hpp — NOT in the reference (it has no meter and no limiter): the end of the export chain over the build-defined
// entry points — the take's BS.1770 loudness, its true peak (mx_true_peak_steps) and its loudness range (mx_loudness_range), and
// the finished int16: the gain that brings the take to a target loudness (mx_normalize_gain_tp, mx_audio_gain), then the
// look-ahead limiter under a true-peak ceiling (mx_audio_limit), with the sample-rate conversion between the two where the take is
// delivered at another rate (mx_audio_resample) — as a class the App can own next to its melonix::LoudnessTrack.
//
//   melonix::Mastering master(rendered, sampleRate);         // uploads once; loudness, true peak and range on the GPU
//   meter->show(master.loudness().integrated, master.truePeakDb(), master.range().lra);
//   master.exportWav("take.wav", -16.0, -1.0);               // -16 LUFS under -1 dBTP, a correct RIFF header
//   master.exportWavAt("take-cd.wav", 44100, -16.0, -1.0);   // the same delivered at 44.1 kHz: converted, then limited
//   master.exportWavCompressedAt("loud.wav", 48000, {}, -12.0, -1.0);  // compressed first, measured again, then the same chain
//
// A render that is already on the device needs no round trip: render f32 into a padded device buffer, mx_audio_wrap_device it
// and call mx_audio_gain / mx_audio_limit_dev directly.
#pragma once
#include <cstdint>
#include <span>
#include <string>
#include <vector>

#include "compressor.hpp"
#include "melonix_amd.h"

namespace melonix {

namespace glue {
struct Session;
}

class Mastering {
public:
  // The samples are kept (finish(), exportWav()).  sampleRate in [8000, 384000].
  Mastering(std::span<const float> wav, int sampleRate, int device = 0);

  bool ok() const { return good; }
  // integrated loudness with its gate counts, the largest momentary and short-term values, the sample peak; zeros after a failed
  // construction
  const mx_loudness &loudness() const { return loudness_; }
  // EBU Tech 3342 loudness range; zeros after a failed construction
  const mx_loudness_range_result &range() const { return range_; }
  // true peak and sample peak of step b (10 ms); empty after a failed construction
  const std::vector<mx_tp_step> &peaks() const { return peaks_; }
  // the largest of each, as amplitudes; truePeakDb(): 20 log10 of the first, -inf for silence
  float truePeak() const { return truePeak_; }
  float samplePeak() const { return samplePeak_; }
  double truePeakDb() const;
  // The take at targetLufs — one gain, the loudness term of mx_normalize_gain_tp: the ceiling is the limiter's —, limited under
  // ceilingDbtp with a look-ahead of lookaheadMs (0 or less: the default, 5 ms), as int16.  Empty after a failed call (a silent
  // take has no loudness).
  std::vector<int16_t> finish(double targetLufs, double ceilingDbtp, double lookaheadMs = 0.0) const;
  // finish() into a WAV file with a correct RIFF header (mx_save_wav); false after a failed call
  bool exportWav(const std::string &path, double targetLufs, double ceilingDbtp, double lookaheadMs = 0.0) const;
  // The same delivered at outRate: the gain finish() takes (from the measurement at the take's own rate), then the sample-rate
  // conversion (mx_audio_resample), then the limiter at outRate — after the conversion, since a true peak is a property of the
  // delivered samples —, mx_resample_length(n, sampleRate, outRate) samples of int16; lookaheadMs is taken at outRate.  At the
  // take's own rate: finish().  Empty for a rate pair the conversion refuses.
  std::vector<int16_t> finishAt(int outRate, double targetLufs, double ceilingDbtp, double lookaheadMs = 0.0) const;
  // finishAt() into a WAV file whose header carries outRate
  bool exportWavAt(const std::string &path, int outRate, double targetLufs, double ceilingDbtp, double lookaheadMs = 0.0) const;
  // The chain with dynamics: the take through the compressor (mx_audio_compress), the loudness and the true peak measured again
  // on the compressed object — the compressor changed both —, the gain to targetLufs from that measurement, the conversion, the
  // limiter, int16.  Empty after a failed call: settings the compressor refuses, or whatever finishAt() refuses.
  std::vector<int16_t> finishCompressedAt(int outRate, const CompressorSettings &compressor, double targetLufs, double ceilingDbtp,
                                          double lookaheadMs = 0.0) const;
  bool exportWavCompressedAt(const std::string &path, int outRate, const CompressorSettings &compressor, double targetLufs,
                             double ceilingDbtp, double lookaheadMs = 0.0) const;

private:
  // gain, conversion and limiter from an object of a session (mastering.cpp): what finishAt() and finishCompressedAt() share
  std::vector<int16_t> deliver(glue::Session &s, const mx_audio *src, int slot, float amp, int outRate, const mx_limit_params &p,
                               int64_t m) const;
  int sampleRate, device_;
  bool good = false;
  std::vector<float> wav_;
  std::vector<mx_tp_step> peaks_;
  mx_loudness loudness_{};
  mx_loudness_range_result range_{};
  float truePeak_ = 0.f, samplePeak_ = 0.f;
};

}  // namespace melonix
