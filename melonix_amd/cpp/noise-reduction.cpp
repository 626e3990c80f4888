// noise-reduction.cpp — see noise-reduction.hpp.
#include "noise-reduction.hpp"

#include <cmath>

#include "capi-glue.hpp"

namespace melonix {

NoiseReduction::NoiseReduction(std::span<const float> wav, int sampleRate, int device)
    : sampleRate_(sampleRate), n((int64_t)wav.size()), session(new glue::Session(device, wav)) {
  good = session->ok && sampleRate > 0;
}

NoiseReduction::~NoiseReduction() = default;

bool NoiseReduction::learn(int64_t beginSample, int64_t endSample) {
  if (!good) return false;
  std::vector<float> p(MX_DENOISE_BINS);
  if (mx_noise_print(session->ctx, session->audio, beginSample, endSample, p.data()) != MX_OK) return false;
  print_ = std::move(p);
  return true;
}

bool NoiseReduction::setPrint(std::span<const float> print) {
  if (print.size() != MX_DENOISE_BINS) return false;
  for (const float v : print)
    if (!(v >= 0.f) || !std::isfinite(v)) return false;
  print_.assign(print.begin(), print.end());
  return true;
}

std::vector<float> NoiseReduction::apply(double reductionDb, double sensitivityDb) const {
  if (!good || print_.empty()) return {};
  const mx_denoise_params p{(float)reductionDb, (float)sensitivityDb};
  std::vector<float> out = glue::derivedSamples(*session, 0, n, [&](mx_ctx *ctx, mx_audio *a, mx_audio **made) {
    return mx_audio_denoise(ctx, a, print_.data(), &p, made);
  });
  if (session->made[0]) {  // (the object has served: the next apply() makes its own)
    mx_audio_free(session->ctx, session->made[0]);
    session->made[0] = nullptr;
  }
  return out;
}

}  // namespace melonix
