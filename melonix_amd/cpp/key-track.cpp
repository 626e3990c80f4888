// key-track.cpp — melonix::KeyTrack over the C-ABI (see key-track.hpp).  A failed call leaves empty vectors and a zero key,
// the way the rest of the facade maps errors.
#include "key-track.hpp"

#include "capi-glue.hpp"

namespace melonix {

KeyTrack::KeyTrack(std::span<const float> wav, int sampleRate, int hop, int windowFrames, int windowHop, int device) : hop_(hop) {
  good = glue::fileTrack(wav, hop, device, chroma_, [&](mx_ctx *ctx, const mx_audio *audio, int64_t frames, mx_chroma_rec *out) {
    if (const int rc = mx_chroma(ctx, audio, sampleRate, hop, 0, frames, nullptr, out)) return rc;
    mx_key_window *v = nullptr;
    int64_t n = 0;
    if (const int rc = mx_key_detect(ctx, audio, sampleRate, hop, nullptr, windowFrames, windowHop, &key_, &v, &n)) return rc;
    windows_ = glue::taken<mx_key_window>(v, n);
    return (int)MX_OK;
  });
  if (!good) {
    key_ = mx_key{};
    windows_.clear();
  }
}

std::vector<Marker> KeyTrack::correctionMarkers(const std::vector<mx_note> &notes, float strength) const {
  if (!good) return {};
  std::vector<Marker> out(2 * notes.size());
  if (mx_correction_markers_tuned(notes.data(), (int64_t)notes.size(), strength, key_.scale_mask, key_.tuning_cents,
                                  reinterpret_cast<mx_marker *>(out.data())) != MX_OK)
    return {};
  return out;
}

}  // namespace melonix
