// capi-glue.hpp — what the facade's units share over the C-ABI.  Internal: not installed, no part of the drop-in API.
#pragma once
#include <span>
#include <vector>

#include "marker.hpp"
#include "melonix_amd.h"

static_assert(sizeof(Marker) == sizeof(mx_marker), "Marker must stay layout-compatible with mx_marker");

namespace melonix::glue {

// the defaults an mx_*_params_default writes
template <class P>
P defaults(void (*fn)(P *)) {
  P p;
  fn(&p);
  return p;
}

// a library array of n records as a vector of Out (Marker for mx_marker, else the record itself); the array goes back
template <class Out, class T>
std::vector<Out> taken(T *v, int64_t n) {
  const Out *p = reinterpret_cast<const Out *>(v);
  std::vector<Out> out(p, p + n);
  mx_free(v);
  return out;
}

// What a call of the facade holds for its own length: a context on `device`, the upload of a take (the second constructor, or
// upload()), and the audio objects the call makes of it (`made`, filled by the caller).  `ok`: everything asked for so far is
// there.  The destructor frees what is there: made[3] .. made[0], the upload, then the context.
struct Session {
  mx_ctx *ctx = nullptr;
  mx_audio *audio = nullptr, *made[4] = {};
  bool ok;
  explicit Session(int device) : ok(mx_ctx_create(device, &ctx) == MX_OK) {}
  Session(int device, std::span<const float> wav) : Session(device) { upload(wav); }
  Session(const Session &) = delete;
  Session &operator=(const Session &) = delete;
  bool upload(std::span<const float> wav) {
    return ok = ok && mx_audio_upload(ctx, wav.data(), (int64_t)wav.size(), &audio) == MX_OK;
  }
  ~Session() {
    for (mx_audio *a : {made[3], made[2], made[1], made[0], audio})
      if (a) mx_audio_free(ctx, a);
    if (ctx) mx_ctx_destroy(ctx);
  }
};

// One per-frame track over a whole file: a session on `device`, `call(ctx, audio, frames, out.data()) -> status` over the
// file's frames at `hop`.  -> whether the track is there; `out` is empty where it is not.
template <class T, class Call>
bool fileTrack(std::span<const float> wav, int hop, int device, std::vector<T> &out, Call call) {
  Session s(device);
  if (!s.ok) return false;
  const int64_t frames = mx_frame_count((int64_t)wav.size(), hop);
  const bool up = s.upload(wav);
  if (up && frames >= 0) out.resize((size_t)frames);
  const bool good = up && frames >= 0 && call(s.ctx, s.audio, frames, out.data()) == MX_OK;
  if (!good) out.clear();
  return good;
}

// S, the samples of the 10 ms step of the loudness and true-peak records: a file's steps are its frames at hop S (0 for a sample
// rate the library refuses: no frames)
inline int stepSamples(int sampleRate) { return mx_loudness_step_count(1, sampleRate) == 1 ? (sampleRate + 50) / 100 : 0; }

// The samples of an audio object made of the session's take: `make(ctx, audio, &object) -> status` (mx_audio_gain,
// mx_audio_denoise, ...) fills slot `slot` of `made`, which must be free; the object's n samples come back, empty where a call
// fails.  The object stays with the session.
template <class Make>
std::vector<float> derivedSamples(Session &s, int slot, int64_t n, Make make) {
  std::vector<float> out((size_t)n);
  const bool done = s.ok && !s.made[slot] && make(s.ctx, s.audio, &s.made[slot]) == MX_OK &&
                    mx_audio_download(s.ctx, s.made[slot], 0, n, out.data()) == MX_OK;
  if (!done) out.clear();
  return out;
}

// `wav` through mx_audio_gain with `points`, on a session of its own; empty where a call fails
inline std::vector<float> gained(std::span<const float> wav, int device, const std::vector<mx_gain_point> &points) {
  Session s(device, wav);
  return derivedSamples(s, 0, (int64_t)wav.size(), [&](mx_ctx *ctx, mx_audio *a, mx_audio **out) {
    return mx_audio_gain(ctx, a, points.data(), (int64_t)points.size(), out);
  });
}

}  // namespace melonix::glue
