// pitch-track.cpp — melonix::PitchTrack over the C-ABI (see pitch-track.hpp).  A failed call leaves an empty track /
// empty vectors, the way the rest of the facade maps errors.
#include "pitch-track.hpp"

namespace melonix {

static_assert(sizeof(Marker) == sizeof(mx_marker), "Marker must stay layout-compatible with mx_marker");

PitchTrack::PitchTrack(std::span<const float> wav, int sampleRate, int hop, float fmin, float fmax, float threshold,
                       int device, bool decoded)
    : sampleRate(sampleRate), hop_(hop), threshold_(threshold), decoded_(decoded) {
  mx_ctx *ctx = nullptr;
  if (mx_ctx_create(device, &ctx) != MX_OK) return;
  mx_audio *audio = nullptr;
  if (mx_audio_upload(ctx, wav.data(), (int64_t)wav.size(), &audio) == MX_OK) {
    const int64_t frames = mx_frame_count((int64_t)wav.size(), hop);
    if (frames >= 0) {
      track.resize((size_t)frames);
      good = (decoded ? mx_f0_track_decoded(ctx, audio, sampleRate, hop, 0, frames, fmin, fmax, threshold, nullptr, track.data())
                      : mx_f0_track(ctx, audio, sampleRate, hop, 0, frames, fmin, fmax, threshold, track.data())) == MX_OK;
      if (!good) track.clear();
    }
    mx_audio_free(ctx, audio);
  }
  mx_ctx_destroy(ctx);
}

std::vector<mx_note> PitchTrack::notes() const {
  mx_note_params p;
  mx_note_params_default(&p);
  if (decoded_) p.threshold = 2.f * threshold_;
  return notes(p);
}

mx_psola_params PitchTrack::psolaParams() const {
  mx_psola_params p;
  mx_psola_params_default(&p);
  if (decoded_) p.threshold = 2.f * threshold_;
  return p;
}

std::vector<mx_note> PitchTrack::notes(const mx_note_params &p) const {
  mx_note *v = nullptr;
  int64_t n = 0;
  if (!good || mx_detect_notes(track.data(), (int64_t)track.size(), sampleRate, hop_, 0, &p, &v, &n) != MX_OK) return {};
  std::vector<mx_note> out(v, v + n);
  mx_free(v);
  return out;
}

std::vector<Marker> PitchTrack::correctionMarkers(float strength, int scaleMask) const {
  const std::vector<mx_note> ns = notes();
  std::vector<Marker> out(2 * ns.size());
  if (mx_correction_markers(ns.data(), (int64_t)ns.size(), strength, scaleMask, reinterpret_cast<mx_marker *>(out.data())) != MX_OK)
    return {};
  return out;
}

}  // namespace melonix
