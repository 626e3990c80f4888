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

// One per-frame track over a whole file: a context on `device`, the upload, `call(ctx, audio, frames, out.data()) -> status`
// over the file's frames at `hop`, both handles released.  -> whether the track is there; `out` is empty where it is not.
template <class T, class Call>
bool fileTrack(std::span<const float> wav, int hop, int device, std::vector<T> &out, Call call) {
  mx_ctx *ctx = nullptr;
  if (mx_ctx_create(device, &ctx) != MX_OK) return false;
  mx_audio *audio = nullptr;
  const int64_t n = (int64_t)wav.size(), frames = mx_frame_count(n, hop);
  const bool up = mx_audio_upload(ctx, wav.data(), n, &audio) == MX_OK;
  if (up && frames >= 0) out.resize((size_t)frames);
  const bool good = up && frames >= 0 && call(ctx, audio, frames, out.data()) == MX_OK;
  if (!good) out.clear();
  if (up) mx_audio_free(ctx, audio);
  mx_ctx_destroy(ctx);
  return good;
}

}  // namespace melonix::glue
