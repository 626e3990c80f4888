// onset-track.cpp — melonix::OnsetTrack over the C-ABI (see onset-track.hpp).  A failed call leaves an empty curve / empty
// vectors, the way the rest of the facade maps errors.
#include "onset-track.hpp"

namespace melonix {

static_assert(sizeof(Marker) == sizeof(mx_marker), "Marker must stay layout-compatible with mx_marker");

OnsetTrack::OnsetTrack(std::span<const float> wav, int sampleRate, int hop, int device)
    : sampleRate(sampleRate), hop_(hop), n_((int64_t)wav.size()) {
  mx_ctx *ctx = nullptr;
  if (mx_ctx_create(device, &ctx) != MX_OK) return;
  mx_audio *audio = nullptr;
  if (mx_audio_upload(ctx, wav.data(), (int64_t)wav.size(), &audio) == MX_OK) {
    const int64_t frames = mx_frame_count((int64_t)wav.size(), hop);
    if (frames >= 0) {
      flux_.resize((size_t)frames);
      good = mx_onset_flux(ctx, audio, sampleRate, hop, 0, frames, nullptr, flux_.data()) == MX_OK;
      if (!good) flux_.clear();
    }
    mx_audio_free(ctx, audio);
  }
  mx_ctx_destroy(ctx);
}

mx_onset_pick_params OnsetTrack::pickParams() {
  mx_onset_pick_params p;
  mx_onset_pick_params_default(&p);
  return p;
}

mx_timing_params OnsetTrack::timingParams() {
  mx_timing_params p;
  mx_timing_params_default(&p);
  return p;
}

std::vector<mx_onset> OnsetTrack::onsets(const mx_onset_pick_params &p) const {
  mx_onset *v = nullptr;
  int64_t n = 0;
  if (!good || mx_onset_pick(flux_.data(), (int64_t)flux_.size(), hop_, 0, &p, &v, &n) != MX_OK) return {};
  std::vector<mx_onset> out(v, v + n);
  mx_free(v);
  return out;
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
  const Marker *m = reinterpret_cast<const Marker *>(v);
  std::vector<Marker> out(m, m + n);
  mx_free(v);
  return out;
}

}  // namespace melonix
