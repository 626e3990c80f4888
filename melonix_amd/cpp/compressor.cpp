// compressor.cpp — see compressor.hpp.
#include "compressor.hpp"

#include <cmath>

#include "capi-glue.hpp"

namespace melonix {

bool compressParams(const CompressorSettings &s, mx_compress_params &out) {
  for (const double v : {s.thresholdDb, s.ratio, s.kneeDb, s.attackMs, s.releaseMs, s.lookaheadMs, s.makeupDb})
    if (!std::isfinite(v)) return false;
  out = mx_compress_params{(float)s.thresholdDb, (float)s.ratio,       (float)s.kneeDb,
                           (float)s.attackMs,    (float)s.releaseMs,   (float)s.lookaheadMs,
                           (float)std::pow(10.0, s.makeupDb / 20.0)};
  return true;
}

Compressor::Compressor(std::span<const float> wav, int sampleRate, int device)
    : sampleRate_(sampleRate), n((int64_t)wav.size()), session(new glue::Session(device, wav)) {
  good = session->ok && mx_compress_steps(0, sampleRate) == 0;
}

Compressor::~Compressor() = default;

std::vector<float> Compressor::apply(const CompressorSettings &settings) {
  reduction_.clear();
  mx_compress_params p;
  if (!good || !compressParams(settings, p)) return {};
  std::vector<float> out = glue::derivedSamples(*session, 0, n, [&](mx_ctx *ctx, mx_audio *a, mx_audio **made) {
    return mx_audio_compress(ctx, a, sampleRate_, &p, made);
  });
  if (session->made[0]) {  // (the object has served: the next apply() makes its own)
    mx_audio_free(session->ctx, session->made[0]);
    session->made[0] = nullptr;
  }
  const int64_t steps = mx_compress_steps(n, sampleRate_);
  std::vector<int32_t> s((size_t)(steps > 0 ? steps : 0));
  if (out.size() != (size_t)n || steps < 0 ||
      mx_compress_gain(session->ctx, session->audio, sampleRate_, &p, 0, steps, s.data()) != MX_OK)
    return {};
  reduction_.resize(s.size());
  for (size_t b = 0; b < s.size(); ++b) reduction_[b] = (float)(20.0 * std::log10((double)s[b] / 1073741824.0));
  return out;
}

}  // namespace melonix
