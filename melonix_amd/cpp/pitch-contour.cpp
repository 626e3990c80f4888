// pitch-contour.cpp — melonix::PitchContour over the C-ABI (see pitch-contour.hpp).  A failed call leaves empty vectors, the
// way the rest of the facade maps errors.
#include "pitch-contour.hpp"

#include "capi-glue.hpp"

namespace melonix {

namespace {
constexpr float kTrackerThreshold = 0.15f;
constexpr float kVoicing = 2.f * kTrackerThreshold;  // a decoded track's, as melonix::PitchTrack reads one
}  // namespace

PitchContour::PitchContour(std::span<const float> wav, int sampleRate, int hop, int device)
    : sampleRate(sampleRate), hop_(hop), device_(device), wav_(wav.begin(), wav.end()) {
  good = glue::fileTrack(wav, hop, device, track, [&](mx_ctx *ctx, const mx_audio *audio, int64_t frames, mx_f0 *out) {
    if (const int rc = mx_f0_track_decoded(ctx, audio, sampleRate, hop, 0, frames, 55.f, 1760.f, kTrackerThreshold, nullptr, out)) return rc;
    mx_note_params np = glue::defaults(mx_note_params_default);
    np.threshold = kVoicing;
    mx_note *v = nullptr;
    int64_t n = 0;
    if (const int rc = mx_detect_notes(out, frames, sampleRate, hop, 0, &np, &v, &n)) return rc;
    notes_ = glue::taken<mx_note>(v, n);
    spans.resize(notes_.size());
    rec.resize((size_t)frames);
    stat.resize(notes_.size());
    if (const int rc = mx_contour_spans(notes_.data(), n, 0, spans.data())) return rc;
    if (const int rc = mx_pitch_contour(ctx, out, frames, sampleRate, hop, 0, notes_.data(), n, kVoicing, np.rms_floor, nullptr,
                                        rec.data(), stat.data()))
      return rc;
    vibrato_.resize(notes_.size());
    for (size_t i = 0; i < notes_.size(); ++i)
      if (const int rc = mx_contour_vibrato(&stat[i], notes_[i].frames, sampleRate, hop, &vibrato_[i])) return rc;
    return (int)MX_OK;
  });
  if (!good) {
    notes_.clear();
    spans.clear();
    rec.clear();
    stat.clear();
    vibrato_.clear();
    wav_.clear();
  }
}

std::vector<float> PitchContour::bend(float drift, float vibrato, std::span<const double> shift, int glideFrames) const {
  if (!good || (!shift.empty() && shift.size() != notes_.size())) return {};
  const mx_bend_params p{drift, vibrato, glideFrames};
  std::vector<float> out(rec.size());
  if (mx_contour_bend(rec.data(), (int64_t)rec.size(), notes_.data(), spans.data(), (int64_t)notes_.size(),
                      shift.empty() ? nullptr : shift.data(), &p, out.data()) != MX_OK)
    return {};
  return out;
}

std::vector<float> PitchContour::correct(float drift, float vibrato, std::span<const double> shift, std::span<const Marker> markers,
                                         std::span<const mx_formant_point> points, int glideFrames) const {
  if (!good) return {};
  const std::vector<float> curve = bend(drift, vibrato, shift, glideFrames);
  if (curve.size() != track.size()) return {};
  const mx_marker *m = reinterpret_cast<const mx_marker *>(markers.data());
  const int64_t n = (int64_t)wav_.size(), len = mx_pv_render_length(n, sampleRate, m, (int)markers.size());
  if (len < 0) return {};
  mx_psola_params pp = glue::defaults(mx_psola_params_default);
  pp.threshold = kVoicing;
  std::vector<float> pcm((size_t)len);
  glue::Session s(device_, wav_);
  const bool done = s.ok && mx_psola_render_bend(s.ctx, s.audio, sampleRate, hop_, track.data(), (int64_t)track.size(), &pp, m,
                                                 (int)markers.size(), points.data(), (int)points.size(), curve.data(), pcm.data(),
                                                 nullptr) == MX_OK;
  if (!done) pcm.clear();
  return pcm;
}

}  // namespace melonix
