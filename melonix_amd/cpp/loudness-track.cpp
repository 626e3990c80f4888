// loudness-track.cpp — melonix::LoudnessTrack over the C-ABI (see loudness-track.hpp).  A failed call leaves empty vectors,
// the way the rest of the facade maps errors.
#include "loudness-track.hpp"

#include "capi-glue.hpp"

namespace melonix {

LoudnessTrack::LoudnessTrack(std::span<const float> wav, int sampleRate, int device)
    : sampleRate(sampleRate), device_(device), wav_(wav.begin(), wav.end()) {
  // a step every S samples: the file's steps are its frames at hop S (no S for a sample rate out of range: no track)
  const int S = glue::stepSamples(sampleRate);
  good = glue::fileTrack(wav, S, device, steps_, [&](mx_ctx *ctx, const mx_audio *audio, int64_t steps, mx_loud_step *out) {
    if (const int rc = mx_loudness_steps(ctx, audio, sampleRate, 0, (steps + 9) / 10, out)) return rc;
    return mx_loudness_integrated(out, steps, sampleRate, &summary_);
  });
  if (!good) summary_ = mx_loudness{};
}

std::vector<double> LoudnessTrack::curve(int window) const {
  std::vector<double> out(steps_.size());
  if (!good || mx_loudness_curve(steps_.data(), (int64_t)steps_.size(), sampleRate, window, out.data()) != MX_OK) return {};
  return out;
}

std::vector<double> LoudnessTrack::noteLoudness(const std::vector<mx_note> &notes) const {
  std::vector<double> out(notes.size());
  if (!good || mx_note_loudness(steps_.data(), (int64_t)steps_.size(), sampleRate, notes.data(), (int64_t)notes.size(), out.data()) != MX_OK)
    return {};
  return out;
}

mx_level_params LoudnessTrack::params() { return glue::defaults(mx_level_params_default); }

std::vector<float> LoudnessTrack::gained(const std::vector<mx_gain_point> &points) const { return glue::gained(wav_, device_, points); }

std::vector<float> LoudnessTrack::levelled(const std::vector<mx_note> &notes, const mx_level_params &p) const {
  const std::vector<double> lufs = noteLoudness(notes);
  if (!good || lufs.size() != notes.size()) return {};
  std::vector<mx_gain_point> points(2 * notes.size());
  if (mx_level_gain_points(notes.data(), (int64_t)notes.size(), lufs.data(), &p, points.data(), nullptr) != MX_OK) return {};
  return gained(points);
}

std::vector<float> LoudnessTrack::normalized(float targetLufs, float ceilingDb) const {
  float amp = 1.f;
  if (!good || mx_normalize_gain(&summary_, (double)targetLufs, (double)ceilingDb, &amp) != MX_OK) return {};
  return gained({mx_gain_point{0, amp}});
}

}  // namespace melonix
