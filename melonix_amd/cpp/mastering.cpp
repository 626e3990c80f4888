// mastering.cpp — melonix::Mastering over the C-ABI (see mastering.hpp).  A failed call leaves empty vectors, the way the rest
// of the facade maps errors.
#include "mastering.hpp"

#include <cmath>
#include <limits>

#include "capi-glue.hpp"

namespace melonix {

Mastering::Mastering(std::span<const float> wav, int sampleRate, int device)
    : sampleRate(sampleRate), device_(device), wav_(wav.begin(), wav.end()) {
  // a step every S samples: the file's steps are its frames at hop S (no S for a sample rate out of range: nothing measured)
  const int S = glue::stepSamples(sampleRate);
  std::vector<mx_loud_step> steps;
  good = glue::fileTrack(wav, S, device, steps, [&](mx_ctx *ctx, const mx_audio *audio, int64_t count, mx_loud_step *out) {
    if (const int rc = mx_loudness_steps(ctx, audio, sampleRate, 0, (count + 9) / 10, out)) return rc;
    if (const int rc = mx_loudness_integrated(out, count, sampleRate, &loudness_)) return rc;
    if (const int rc = mx_loudness_range(out, count, sampleRate, &range_)) return rc;
    peaks_.resize((size_t)count);
    if (const int rc = mx_true_peak_steps(ctx, audio, sampleRate, 0, count, peaks_.data())) return rc;
    return mx_true_peak_measure(ctx, audio, sampleRate, &truePeak_, &samplePeak_);
  });
  if (!good) {
    loudness_ = mx_loudness{};
    range_ = mx_loudness_range_result{};
    peaks_.clear();
    truePeak_ = samplePeak_ = 0.f;
  }
}

double Mastering::truePeakDb() const {
  return truePeak_ > 0.f ? 20.0 * std::log10((double)truePeak_) : -std::numeric_limits<double>::infinity();
}

std::vector<int16_t> Mastering::finish(double targetLufs, double ceilingDbtp, double lookaheadMs) const {
  return finishAt(sampleRate, targetLufs, ceilingDbtp, lookaheadMs);
}

// the limiter's parameters at the rate it delivers: the ceiling as an amplitude, any look-ahead brought into [1, 1024] samples
static bool limitParams(int outRate, double ceilingDbtp, double lookaheadMs, mx_limit_params &p) {
  if (mx_limit_params_default(outRate, &p) != MX_OK || !std::isfinite(ceilingDbtp) || !std::isfinite(lookaheadMs)) return false;
  p.ceiling_amp = (float)std::pow(10.0, ceilingDbtp / 20.0);
  if (lookaheadMs > 0.0) {
    const double a = std::floor(lookaheadMs * (double)outRate / 1000.0 + 0.5);
    p.lookahead = a < 1.0 ? 1 : a > 1024.0 ? 1024 : (int32_t)a;
  }
  return true;
}

// The end of the chain from `src`, an object of the session at the take's rate: the gain `amp` (made[slot]), the conversion where
// outRate differs (made[slot + 1]), the limiter (made[slot + 2]) -> int16; empty after a failed call.
std::vector<int16_t> Mastering::deliver(glue::Session &s, const mx_audio *src, int slot, float amp, int outRate, const mx_limit_params &p,
                                        int64_t m) const {
  std::vector<int16_t> out((size_t)m);
  const mx_gain_point point{0, amp};
  bool done = s.ok && mx_audio_gain(s.ctx, src, &point, 1, &s.made[slot]) == MX_OK;
  const mx_audio *levelled = s.made[slot];
  if (done && outRate != sampleRate) {  // conversion before the limiter: a true peak belongs to the delivered samples
    done = mx_audio_resample(s.ctx, levelled, sampleRate, outRate, &s.made[slot + 1]) == MX_OK;
    levelled = s.made[slot + 1];
  }
  done = done && mx_audio_limit(s.ctx, levelled, outRate, &p, &s.made[slot + 2], out.data()) == MX_OK;
  if (!done) out.clear();
  return out;
}

std::vector<int16_t> Mastering::finishAt(int outRate, double targetLufs, double ceilingDbtp, double lookaheadMs) const {
  float amp = 1.f;
  // (a ceiling far above any take: the loudness term alone)
  if (!good || mx_normalize_gain_tp(&loudness_, truePeak_, targetLufs, 200.0, &amp) != MX_OK) return {};
  const int64_t m = mx_resample_length((int64_t)wav_.size(), sampleRate, outRate);
  mx_limit_params p;  // the limiter works at the rate it delivers
  if (m < 0 || !limitParams(outRate, ceilingDbtp, lookaheadMs, p)) return {};
  glue::Session s(device_, wav_);
  return deliver(s, s.audio, 0, amp, outRate, p, m);
}

std::vector<int16_t> Mastering::finishCompressedAt(int outRate, const CompressorSettings &compressor, double targetLufs,
                                                   double ceilingDbtp, double lookaheadMs) const {
  mx_compress_params cp;
  const int64_t m = mx_resample_length((int64_t)wav_.size(), sampleRate, outRate);
  mx_limit_params p;
  if (!good || !compressParams(compressor, cp) || m < 0 || !limitParams(outRate, ceilingDbtp, lookaheadMs, p)) return {};
  glue::Session s(device_, wav_);
  mx_loudness loud{};
  float truePeak = 0.f, amp = 1.f;
  // the loudness the gain is taken from is the compressed take's: the compressor changed it
  const bool levelled = s.ok && mx_audio_compress(s.ctx, s.audio, sampleRate, &cp, &s.made[0]) == MX_OK &&
                        mx_loudness_measure(s.ctx, s.made[0], sampleRate, &loud) == MX_OK &&
                        mx_true_peak_measure(s.ctx, s.made[0], sampleRate, &truePeak, nullptr) == MX_OK &&
                        mx_normalize_gain_tp(&loud, truePeak, targetLufs, 200.0, &amp) == MX_OK;
  if (!levelled) return {};
  return deliver(s, s.made[0], 1, amp, outRate, p, m);
}

bool Mastering::exportWav(const std::string &path, double targetLufs, double ceilingDbtp, double lookaheadMs) const {
  return exportWavAt(path, sampleRate, targetLufs, ceilingDbtp, lookaheadMs);
}

bool Mastering::exportWavAt(const std::string &path, int outRate, double targetLufs, double ceilingDbtp, double lookaheadMs) const {
  const std::vector<int16_t> pcm = finishAt(outRate, targetLufs, ceilingDbtp, lookaheadMs);
  return !pcm.empty() && mx_save_wav(path.c_str(), pcm.data(), (int64_t)pcm.size(), outRate, 0) == MX_OK;
}

bool Mastering::exportWavCompressedAt(const std::string &path, int outRate, const CompressorSettings &compressor, double targetLufs,
                                      double ceilingDbtp, double lookaheadMs) const {
  const std::vector<int16_t> pcm = finishCompressedAt(outRate, compressor, targetLufs, ceilingDbtp, lookaheadMs);
  return !pcm.empty() && mx_save_wav(path.c_str(), pcm.data(), (int64_t)pcm.size(), outRate, 0) == MX_OK;
}

}  // namespace melonix
