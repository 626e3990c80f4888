// onset_logic.cpp — see onset_logic.h.  Host-only C++17 (no HIP), binary64, built with -ffp-contract=off: tests/onset_ref.py
// restates every expression below in the same order and compares field for field.
#include "onset_logic.h"

#include <algorithm>
#include <cmath>

namespace mx {

std::vector<mx_onset> pick_onsets(const float *flux, int64_t count, int hop, int64_t first_frame, const mx_onset_pick_params &p) {
  std::vector<mx_onset> out;
  auto o = [&](int64_t i) { return std::isfinite(flux[i]) ? (double)flux[i] : 0.0; };
  int64_t last = -1;  // the previous accepted index (none yet)
  for (int64_t f = 0; f < count; ++f) {
    const double of = o(f);
    bool peak = true;
    for (int64_t g = std::max<int64_t>(0, f - p.pre_max); g < f && peak; ++g) peak = of > o(g);
    for (int64_t g = f + 1; g <= std::min<int64_t>(count - 1, f + p.post_max) && peak; ++g) peak = of >= o(g);
    if (!peak) continue;
    const int64_t lo = std::max<int64_t>(0, f - p.pre_avg), hi = std::min<int64_t>(count - 1, f + p.post_avg);
    double sum = 0.0;
    for (int64_t g = lo; g <= hi; ++g) sum += o(g);
    const double thr = p.ratio * (sum / (double)(hi - lo + 1)) + p.delta;
    if (!(of >= thr)) continue;
    if (last >= 0 && !(f - last > p.wait)) continue;
    last = f;
    const int64_t frame = first_frame + f;
    out.push_back(mx_onset{(int32_t)(frame * hop), (int32_t)frame, (float)of, (float)(of - thr)});
  }
  return out;
}

namespace {

// the warp through (0, 0) and (a_i, T_i), in sample2Time's form; the natural rate behind the last anchor.  Queried at
// ascending samples > 0: the segment that holds s is found from where the last query left off
struct Warp {
  const std::vector<int32_t> &a;
  const std::vector<double> &T;
  int sr;
  size_t k = 0;
  double operator()(int32_t s) {
    while (k < a.size() && s > a[k]) ++k;
    const int32_t prevSample = k ? a[k - 1] : 0;
    const double prevTime = k ? T[k - 1] : 0.0;
    if (k < a.size()) return prevTime + (s - prevSample) * (T[k] - prevTime) / (a[k] - prevSample);
    return prevTime + 1. * (s - prevSample) / sr;
  }
};

}  // namespace

std::vector<mx_marker> timing_markers(const int32_t *anchors, int64_t nanchors, int64_t n, int sampleRate, const mx_timing_params &p,
                                      const mx_marker *base, int nbase) {
  const double sr = (double)sampleRate;
  std::vector<int32_t> a;
  for (int64_t i = 0; i < nanchors; ++i)
    if (anchors[i] > 0) a.push_back(anchors[i]);
  // targets and the monotone pass
  const double g = 60.0 / (p.bpm * (double)p.division);
  std::vector<double> T(a.size());
  double Tprev = 0.0;
  int32_t aprev = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    const double t = a[i] / sr;
    const double q = std::floor((t - p.offset) / g + 0.5);
    double d = p.offset + q * g - t;
    if (std::fabs(d) > p.max_shift) d = 0.0;
    const double U = t + p.strength * d;
    const double span = (a[i] - aprev) / sr;
    const double lo = span / p.max_stretch, hi = span * p.max_stretch;
    double step = U - Tprev;
    step = step < lo ? lo : step > hi ? hi : step;
    T[i] = Tprev + step;
    Tprev = T[i];
    aprev = a[i];
  }
  Warp W{a, T, sampleRate};
  // the union of anchors and base samples, sorted
  std::vector<mx_marker> out;
  out.reserve(a.size() + (size_t)nbase);
  size_t ia = 0;
  int ib = 0;
  int32_t sprev = 0;
  double wprev = 0.0;
  while (ia < a.size() || ib < nbase) {
    const bool take_base = ib < nbase && (ia >= a.size() || base[ib].sample <= a[ia]);
    mx_marker m{};
    if (take_base) {
      m = base[ib];
      if (ia < a.size() && a[ia] == m.sample) ++ia;
      ++ib;
    } else {
      m.sample = a[ia++];
      // the bend along time2PitchBend's own curve over the source: (0, 0), the base points, (n - 1, 0); the note between
      // the neighbours, the nearer end's outside them
      int32_t x0 = 0, x1 = (int32_t)(n - 1);
      double y0 = 0.0, y1 = 0.0;
      if (ib > 0) x0 = base[ib - 1].sample, y0 = base[ib - 1].pitchBend;
      if (ib < nbase) x1 = base[ib].sample, y1 = base[ib].pitchBend;
      m.pitchBend = x1 > x0 ? y0 + (m.sample - x0) * (y1 - y0) / (x1 - x0) : y0;
      if (nbase == 0) m.note = 0.0;
      else if (ib == 0) m.note = base[0].note;
      else if (ib == nbase) m.note = base[nbase - 1].note;
      else
        m.note = base[ib - 1].note +
                 (m.sample - base[ib - 1].sample) * (base[ib].note - base[ib - 1].note) / (base[ib].sample - base[ib - 1].sample);
    }
    const double w = W(m.sample);
    double dt = (w - wprev) - (m.sample - sprev) / sr;
    if (std::fabs(dt) < 1e-10) dt = 0.0;  // the rounding residue of two differences, not a shift
    m.dTime = dt;
    out.push_back(m);
    sprev = m.sample;
    wprev = w;
  }
  return out;
}

}  // namespace mx
