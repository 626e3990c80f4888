// compress_logic.cpp — see compress_logic.h.
#include "compress_logic.h"

#include <cmath>
#include <cstring>

#include "compress_core.h"

namespace mx {

const char *compress_params_error(const mx_compress_params &p) {
  if (!(p.threshold_db >= -60.f && p.threshold_db <= 0.f)) return "threshold_db outside [-60, 0]";
  if (!(p.ratio >= 1.f && p.ratio <= 100.f)) return "ratio outside [1, 100]";
  if (!(p.knee_db >= 0.f && p.knee_db <= 24.f)) return "knee_db outside [0, 24]";
  if (!(p.attack_ms >= 0.f && p.attack_ms <= 500.f)) return "attack_ms outside [0, 500]";
  if (!(p.release_ms >= 0.f && p.release_ms <= 2000.f)) return "release_ms outside [0, 2000]";
  if (!(p.lookahead_ms >= 0.f && p.lookahead_ms <= 20.f)) return "lookahead_ms outside [0, 20]";
  if (!std::isnormal(p.makeup_amp) || !(p.makeup_amp >= 0.0625f && p.makeup_amp <= 16.f)) return "makeup_amp outside [1/16, 16]";
  return nullptr;
}

mx_compress_params compress_defaults() { return mx_compress_params{-18.f, 4.f, 6.f, 5.f, 100.f, 0.f, 1.f}; }

// c = round((1 - exp(-D / (sr tau))) 2^24) in [1, 2^24]; tau = 0: 2^24
static int32_t coefficient(int D, int sr, double ms) {
  if (!(ms > 0.0)) return cp::kFull;
  const double c = std::floor((1.0 - std::exp(-(double)D / ((double)sr * (ms / 1000.0)))) * 16777216.0 + 0.5);
  return c < 1.0 ? 1 : c > 16777216.0 ? cp::kFull : (int32_t)c;
}

mx_compress_plan compress_plan(int sr, const mx_compress_params &p) {
  mx_compress_plan q;
  q.D = cp::step_samples(sr);
  q.K = (int32_t)std::floor((double)p.lookahead_ms * (double)sr / (1000.0 * (double)q.D) + 0.5);
  q.c_att = coefficient(q.D, sr, (double)p.attack_ms);
  q.c_rel = coefficient(q.D, sr, (double)p.release_ms);
  const int32_t c = q.c_att < q.c_rel ? q.c_att : q.c_rel;
  const int64_t w = 16 * (int64_t)((cp::kFull + c - 1) / c);
  q.W = (int32_t)(w < cp::kMaxWarm ? w : cp::kMaxWarm);
  q.Gc = cp::kGroup;
  return q;
}

void compress_curve(const mx_compress_params &p, int32_t *out) {
  const double thr = (double)p.threshold_db, knee = (double)p.knee_db, slope = 1.0 / (double)p.ratio - 1.0;
  int32_t low = cp::kUnity;
  for (int j = 0; j < cp::kCurve; ++j) {
    const uint32_t bits = cp::kBase + ((uint32_t)j << 17);
    float pf;
    std::memcpy(&pf, &bits, sizeof pf);
    const double o = 20.0 * std::log10((double)pf) - thr;
    double g;
    if (2.0 * o <= -knee)
      g = 0.0;
    else if (std::fabs(2.0 * o) < knee)
      g = slope * (o + knee / 2.0) * (o + knee / 2.0) / (2.0 * knee);
    else
      g = slope * o;
    const double t = std::floor(std::pow(10.0, g / 20.0) * 1073741824.0);
    const int32_t v = t >= 1073741824.0 ? cp::kUnity : (int32_t)t;
    low = v < low ? v : low;
    out[j] = low;
  }
}

}  // namespace mx
