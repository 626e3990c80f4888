// sibilant_logic.cpp — see sibilant_logic.h.  Built with -ffp-contract=off: tests/sibilant_ref.py repeats every expression.
#include "sibilant_logic.h"

#include <algorithm>
#include <cmath>

namespace mx {

namespace {

struct FrameView {
  double level, share;
};
FrameView view(const mx_sib_feat &f) {
  const double s = (double)f.low + (double)f.high;
  if (!std::isfinite(s) || !(s > 0.0)) return {0.0, 0.0};
  return {std::sqrt(s), (double)f.high / s};
}

struct Span {
  int64_t lo, start, end, hi;
};
// the merged, clipped spans of a checked sibilant list
std::vector<Span> spans_of(const mx_sibilant *sibs, int64_t nsib, int32_t ramp, int64_t n) {
  std::vector<Span> out;
  for (int64_t i = 0; i < nsib; ++i) {
    const int64_t s = sibs[i].start_sample, e = sibs[i].end_sample;
    if (!out.empty() && s - ramp <= out.back().end + ramp) out.back().end = e;
    else out.push_back({0, s, e, 0});
  }
  for (Span &sp : out) {
    sp.lo = std::max<int64_t>(sp.start - ramp, 0);
    sp.hi = std::min<int64_t>(sp.end + ramp, n - 1);
  }
  return out;
}
// a span's points: `edge(x)` the value at lo / hi, `core` the value on [start, end]
template <class P, class Edge, class V>
void span_points(const Span &sp, Edge &&edge, V core, std::vector<P> &out) {
  if (sp.lo < sp.start) out.push_back(P{(int32_t)sp.lo, edge(sp.lo)});
  out.push_back(P{(int32_t)sp.start, core});
  if (sp.end > sp.start) out.push_back(P{(int32_t)sp.end, core});
  if (sp.hi > sp.end) out.push_back(P{(int32_t)sp.hi, edge(sp.hi)});
}

}  // namespace

std::vector<mx_sibilant> sibilant_segments(const mx_sib_feat *feat, int64_t count, int hop, int64_t first_frame,
                                           const mx_sibilant_params &p) {
  struct Run {
    int64_t first, last;
  };
  std::vector<Run> runs;
  bool open = false;
  int64_t start = 0;
  for (int64_t f = 0; f < count; ++f) {
    const FrameView v = view(feat[f]);
    const bool loud = v.level >= p.level_floor;
    if (!open) {
      if (loud && v.share >= p.share_on && feat[f].zero_crossings >= p.zc_min) open = true, start = f;
    } else if (!(loud && v.share >= p.share_off)) {
      open = false;
      runs.push_back({start, f - 1});
    }
  }
  if (open) runs.push_back({start, count - 1});
  std::vector<Run> merged;
  for (const Run &r : runs) {
    if (!merged.empty() && r.first - merged.back().last - 1 <= (int64_t)p.merge_gap) merged.back().last = r.last;
    else merged.push_back(r);
  }
  std::vector<mx_sibilant> out;
  for (const Run &r : merged) {
    const int64_t frames = r.last - r.first + 1;
    if (frames < (int64_t)p.min_frames) continue;
    double sum = 0.0, top = 0.0;
    for (int64_t f = r.first; f <= r.last; ++f) {
      const FrameView v = view(feat[f]);
      sum += v.share;
      if (v.level > top) top = v.level;
    }
    mx_sibilant s;
    s.start_sample = (int32_t)((first_frame + r.first) * (int64_t)hop);
    s.end_sample = (int32_t)((first_frame + r.last) * (int64_t)hop);
    s.first_frame = (int32_t)(first_frame + r.first);
    s.frames = (int32_t)frames;
    s.share = (float)(sum / (double)frames);
    s.level = (float)top;
    out.push_back(s);
  }
  return out;
}

const char *formant_curve_error(const mx_formant_point *points, int64_t npoints) {
  for (int64_t j = 0; j < npoints; ++j) {
    if (!std::isfinite(points[j].semitones)) return "formant point: semitones not finite";
    if (j > 0 && !(points[j].sample > points[j - 1].sample)) return "formant points: samples do not increase";
  }
  return nullptr;
}

const char *sibilant_list_error(const mx_sibilant *sibs, int64_t nsib, int64_t n) {
  for (int64_t i = 0; i < nsib; ++i) {
    if (sibs[i].start_sample < 0 || sibs[i].end_sample < sibs[i].start_sample || (int64_t)sibs[i].end_sample > n - 1)
      return "sibilant outside [0, n - 1] or ending before it starts";
    if (i > 0 && sibs[i].start_sample <= sibs[i - 1].end_sample) return "sibilants out of order or overlapping";
  }
  return nullptr;
}

std::vector<mx_formant_point> formant_protect(const mx_formant_point *points, int64_t npoints, const mx_sibilant *sibs, int64_t nsib,
                                              int32_t ramp, int64_t n) {
  std::vector<mx_formant_point> out;
  if (npoints == 0) return out;
  // F(x) of "Independent formant shift", expression for expression
  auto curve = [&](int64_t xi) -> float {
    const double x = (double)xi;
    if (x < (double)points[0].sample) return points[0].semitones;
    if (x >= (double)points[npoints - 1].sample) return points[npoints - 1].semitones;
    const mx_formant_point *hi =
        std::upper_bound(points, points + npoints, x, [](double v, const mx_formant_point &q) { return v < (double)q.sample; });
    const mx_formant_point &q0 = hi[-1], &q1 = hi[0];
    return (float)((double)q0.semitones +
                   (x - (double)q0.sample) * ((double)q1.semitones - (double)q0.semitones) / ((double)q1.sample - (double)q0.sample));
  };
  int64_t j = 0;
  for (const Span &sp : spans_of(sibs, nsib, ramp, n)) {
    for (; j < npoints && (int64_t)points[j].sample < sp.lo; ++j) out.push_back(points[j]);
    span_points(sp, curve, 0.f, out);
    while (j < npoints && (int64_t)points[j].sample <= sp.hi) ++j;
  }
  for (; j < npoints; ++j) out.push_back(points[j]);
  return out;
}

std::vector<mx_gain_point> sibilant_gain_points(const mx_sibilant *sibs, int64_t nsib, double db, int32_t ramp, int64_t n) {
  std::vector<mx_gain_point> out;
  const float amp = (float)std::pow(10.0, db / 20.0);
  for (const Span &sp : spans_of(sibs, nsib, ramp, n)) span_points(sp, [](int64_t) { return 1.f; }, amp, out);
  return out;
}

const char *gain_points_error(const mx_gain_point *pts, int64_t npts) {
  for (int64_t j = 0; j < npts; ++j) {
    if (!std::isfinite(pts[j].amp) || !(pts[j].amp > 0.f)) return "gain point: amp must be finite and > 0";
    if (j > 0 && !(pts[j].sample > pts[j - 1].sample)) return "gain points: samples do not increase";
  }
  return nullptr;
}

}  // namespace mx
