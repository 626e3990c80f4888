// sibilant-track.cpp — melonix::SibilantTrack over the C-ABI (see sibilant-track.hpp).  A failed call leaves empty vectors,
// the way the rest of the facade maps errors.
#include "sibilant-track.hpp"

#include "capi-glue.hpp"

namespace melonix {

SibilantTrack::SibilantTrack(std::span<const float> wav, int sampleRate, int hop, int device)
    : sampleRate(sampleRate), hop_(hop), device_(device), wav_(wav.begin(), wav.end()) {
  good = glue::fileTrack(wav, hop, device, feat_, [&](mx_ctx *ctx, const mx_audio *audio, int64_t frames, mx_sib_feat *out) {
    return mx_sib_features(ctx, audio, sampleRate, hop, 0, frames, nullptr, out);
  });
}

mx_sibilant_params SibilantTrack::params() { return glue::defaults(mx_sibilant_params_default); }

std::vector<mx_sibilant> SibilantTrack::sibilants(const mx_sibilant_params &p) const {
  mx_sibilant *v = nullptr;
  int64_t n = 0;
  if (!good || mx_sibilants(feat_.data(), (int64_t)feat_.size(), hop_, 0, &p, &v, &n) != MX_OK) return {};
  return glue::taken<mx_sibilant>(v, n);
}

std::vector<mx_formant_point> SibilantTrack::protect(const std::vector<mx_formant_point> &curve, int rampSamples) const {
  if (!good) return {};
  const std::vector<mx_sibilant> s = sibilants();
  mx_formant_point *v = nullptr;
  int64_t n = 0;
  if (mx_formant_protect(curve.data(), (int)curve.size(), s.data(), (int64_t)s.size(), rampSamples, (int64_t)wav_.size(), &v, &n) != MX_OK)
    return {};
  return glue::taken<mx_formant_point>(v, n);
}

std::vector<float> SibilantTrack::balanced(float db, int rampSamples) const {
  if (!good) return {};
  const std::vector<mx_sibilant> s = sibilants();
  mx_gain_point *pts = nullptr;
  int64_t npts = 0;
  if (mx_sibilant_gain_points(s.data(), (int64_t)s.size(), (double)db, rampSamples, (int64_t)wav_.size(), &pts, &npts) != MX_OK) return {};
  return glue::gained(wav_, device_, glue::taken<mx_gain_point>(pts, npts));
}

}  // namespace melonix
