// contour_logic.cpp — see contour_logic.h.  Built with g++ -ffp-contract=off: tests/contour_ref.py restates every function in
// Python and expects the same doubles.
#include "contour_logic.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace mx {

mx_contour_params contour_params_default(int sampleRate, int hop) {
  const double fps = (double)sampleRate / (double)hop;
  mx_contour_params p;
  p.half_width = (int32_t)std::min(64.0, std::max(0.0, std::floor(0.125 * fps)));
  p.lag_min = (int32_t)std::min(256.0, std::max(1.0, std::floor(fps / 12.0)));
  p.lag_max = (int32_t)std::max((double)p.lag_min, std::min(256.0, std::ceil(fps / 3.0)));
  return p;
}

const char *contour_spans_error(const mx_contour_span *spans, int64_t nspans, int64_t count, const int32_t *cents) {
  int64_t end = 0;  // of the span before
  for (int64_t i = 0; i < nspans; ++i) {
    const int64_t lo = spans[i].first, F = spans[i].frames;
    if (F < 1) return "a span of fewer than one frame";
    if (lo < end) return "spans out of order, overlapping or before the array";
    if (lo + F > count) return "a span beyond the array";
    end = lo + F;
    if (cents)
      for (int64_t f = lo; f < end; ++f)
        if (cents[f] == MX_CONTOUR_NONE) return "an unvoiced frame (MX_CONTOUR_NONE) inside a span";
  }
  return nullptr;
}

void contour_spans(const mx_note *notes, int64_t nnotes, int64_t first_frame, mx_contour_span *spans) {
  for (int64_t i = 0; i < nnotes; ++i) {
    const int64_t d = (int64_t)notes[i].first_frame - first_frame;
    spans[i].first = (int32_t)std::min<int64_t>(INT32_MAX, std::max<int64_t>(INT32_MIN, d));  // (out of range: refused later)
    spans[i].frames = notes[i].frames;
  }
}

mx_vibrato contour_vibrato(const mx_contour_stat &stat, int32_t frames, int sampleRate, int hop) {
  mx_vibrato v{0., 0., 0., 0.};
  if (stat.lag == 0 || stat.r0 == 0) return v;
  v.rate_hz = (double)sampleRate / (double)hop / (double)stat.lag;
  v.extent_cents = std::sqrt(2.0 * (double)stat.r0 / (double)frames) / 16.0;
  v.strength = ((double)stat.r_lag / (double)stat.r0) * (double)frames / (double)(frames - stat.lag);
  v.drift_cents = ((double)stat.max_smooth - (double)stat.min_smooth) / 16.0;
  return v;
}

const char *bend_params_error(const mx_bend_params &p) {
  if (!(p.drift_amount >= 0.0 && p.drift_amount <= 1.0)) return "drift_amount outside [0, 1]";
  if (!(p.vibrato_scale >= 0.0 && p.vibrato_scale <= 4.0)) return "vibrato_scale outside [0, 4]";
  if (p.glide_frames < 0) return "glide_frames is negative";
  return nullptr;
}

void contour_bend(const mx_contour_rec *rec, int64_t count, const mx_note *notes, const mx_contour_span *spans, int64_t nnotes,
                  const double *shift, const mx_bend_params &p, float *out) {
  std::fill(out, out + count, 0.f);
  for (int64_t i = 0; i < nnotes; ++i) {
    const int64_t lo = spans[i].first, hi = lo + spans[i].frames;
    const double sh = shift ? shift[i] : 0.0;
    for (int64_t h = lo; h < hi; ++h) {
      const double drift = (double)rec[h].smooth / 1600.0 - notes[i].note;
      const double x = sh - p.drift_amount * drift;
      const double v = (p.vibrato_scale - 1.0) * (double)rec[h].vib / 1600.0;
      out[h] = (float)(x + v);
    }
    if (i == 0) continue;
    const int64_t end = (int64_t)spans[i - 1].first + spans[i - 1].frames, G = lo - end;  // the gap before this note
    if (G < 1 || G > (int64_t)p.glide_frames) continue;
    const double x0 = (double)out[end - 1], x1 = (double)out[lo];
    for (int64_t j = 1; j <= G; ++j) out[end - 1 + j] = (float)(x0 + (x1 - x0) * (double)j / (double)(G + 1));
  }
}

}  // namespace mx
