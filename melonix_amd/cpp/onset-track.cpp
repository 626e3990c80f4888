// onset-track.cpp — melonix::OnsetTrack over the C-ABI (see onset-track.hpp).  A failed call leaves an empty curve / empty
// vectors, the way the rest of the facade maps errors.
#include "onset-track.hpp"

#include "capi-glue.hpp"

namespace melonix {

OnsetTrack::OnsetTrack(std::span<const float> wav, int sampleRate, int hop, int device)
    : sampleRate(sampleRate), hop_(hop), device_(device), n_((int64_t)wav.size()) {
  good = glue::fileTrack(wav, hop, device, flux_, [&](mx_ctx *ctx, const mx_audio *audio, int64_t frames, float *out) {
    return mx_onset_flux(ctx, audio, sampleRate, hop, 0, frames, nullptr, out);
  });
}

mx_onset_pick_params OnsetTrack::pickParams() { return glue::defaults(mx_onset_pick_params_default); }

mx_timing_params OnsetTrack::timingParams() { return glue::defaults(mx_timing_params_default); }

std::vector<mx_onset> OnsetTrack::onsets(const mx_onset_pick_params &p) const {
  mx_onset *v = nullptr;
  int64_t n = 0;
  if (!good || mx_onset_pick(flux_.data(), (int64_t)flux_.size(), hop_, 0, &p, &v, &n) != MX_OK) return {};
  return glue::taken<mx_onset>(v, n);
}

std::vector<Marker> OnsetTrack::timingMarkers(const mx_timing_params &p, const std::vector<Marker> &baseMarkers) const {
  if (!good) return {};
  std::vector<int32_t> anchors;
  for (const mx_onset &o : onsets()) anchors.push_back(o.sample);
  mx_marker *v = nullptr;
  int64_t n = 0;
  if (mx_timing_markers(anchors.data(), (int64_t)anchors.size(), n_, sampleRate, &p,
                        reinterpret_cast<const mx_marker *>(baseMarkers.data()), (int)baseMarkers.size(), &v, &n) != MX_OK)
    return {};
  return glue::taken<Marker>(v, n);
}

mx_tempo_params OnsetTrack::tempoParams() { return glue::defaults(mx_tempo_params_default); }

// the estimate over flux() on a context of its own for the call (the track keeps none); windows null: not wanted
bool OnsetTrack::estimate(const mx_tempo_params &p, mx_tempo &t, std::vector<mx_tempo_window> *windows) const {
  t = mx_tempo{};
  if (windows) windows->clear();
  if (!good) return false;
  glue::Session s(device_);
  mx_tempo_window *v = nullptr;
  int64_t n = 0;
  const bool done = s.ok && mx_tempo_from_flux(s.ctx, flux_.data(), (int64_t)flux_.size(), sampleRate, hop_, 0, &p, &t, windows ? &v : nullptr,
                                       windows ? &n : nullptr) == MX_OK;
  if (!done) t = mx_tempo{};
  else if (windows) *windows = glue::taken<mx_tempo_window>(v, n);
  return done;
}

mx_tempo OnsetTrack::tempo(const mx_tempo_params &p) const {
  mx_tempo t;
  estimate(p, t, nullptr);
  return t;
}

std::vector<mx_tempo_window> OnsetTrack::tempoWindows(const mx_tempo_params &p) const {
  mx_tempo t;
  std::vector<mx_tempo_window> w;
  estimate(p, t, &w);
  return w;
}

}  // namespace melonix
