// pitch-track.cpp — melonix::PitchTrack over the C-ABI (see pitch-track.hpp).  A failed call leaves an empty track /
// empty vectors, the way the rest of the facade maps errors.
#include "pitch-track.hpp"

#include "capi-glue.hpp"

namespace melonix {

PitchTrack::PitchTrack(std::span<const float> wav, int sampleRate, int hop, float fmin, float fmax, float threshold,
                       int device, bool decoded)
    : sampleRate(sampleRate), hop_(hop), threshold_(threshold), decoded_(decoded) {
  good = glue::fileTrack(wav, hop, device, track, [&](mx_ctx *ctx, const mx_audio *audio, int64_t frames, mx_f0 *out) {
    return decoded ? mx_f0_track_decoded(ctx, audio, sampleRate, hop, 0, frames, fmin, fmax, threshold, nullptr, out)
                   : mx_f0_track(ctx, audio, sampleRate, hop, 0, frames, fmin, fmax, threshold, out);
  });
}

std::vector<mx_note> PitchTrack::notes() const {
  mx_note_params p = glue::defaults(mx_note_params_default);
  if (decoded_) p.threshold = 2.f * threshold_;
  return notes(p);
}

mx_psola_params PitchTrack::psolaParams() const {
  mx_psola_params p = glue::defaults(mx_psola_params_default);
  if (decoded_) p.threshold = 2.f * threshold_;
  return p;
}

std::vector<mx_note> PitchTrack::notes(const mx_note_params &p) const {
  mx_note *v = nullptr;
  int64_t n = 0;
  if (!good || mx_detect_notes(track.data(), (int64_t)track.size(), sampleRate, hop_, 0, &p, &v, &n) != MX_OK) return {};
  return glue::taken<mx_note>(v, n);
}

std::vector<Marker> PitchTrack::correctionMarkers(float strength, int scaleMask) const {
  const std::vector<mx_note> ns = notes();
  std::vector<Marker> out(2 * ns.size());
  if (mx_correction_markers(ns.data(), (int64_t)ns.size(), strength, scaleMask, reinterpret_cast<mx_marker *>(out.data())) != MX_OK)
    return {};
  return out;
}

}  // namespace melonix
