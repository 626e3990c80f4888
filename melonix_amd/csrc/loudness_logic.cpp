// loudness_logic.cpp — see loudness_logic.h.  Every sum runs in ascending order and every gate is decided on energies, so that
// tests/loudness_ref.py decides alike; log10 and pow are libm's.
#include "loudness_logic.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace mx {
namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kOffset = -0.691;
constexpr double kAbsGate = 0x1.f791ec6e1d5b7p-24;  // 10^((-70 + 0.691) / 10)
constexpr double kInf = std::numeric_limits<double>::infinity();
constexpr int kBlockSteps = 40, kBlockHop = 10, kShortSteps = 300;

double lufs(double mean_square) { return kOffset + 10.0 * std::log10(mean_square); }

// the sum of the energies of steps [first, first + count), ascending
double energy_sum(const mx_loud_step *steps, int64_t first, int64_t count) {
  double s = 0.0;
  for (int64_t j = first; j < first + count; ++j) s += steps[j].energy;
  return s;
}

// the largest value of the curve with `window` steps that is not NaN (-inf: none); `curve`: room for nsteps values
double curve_max(const mx_loud_step *steps, int64_t nsteps, int S, int window, std::vector<double> &curve) {
  loudness_curve(steps, nsteps, S, window, curve.data());
  double m = -kInf;
  for (int64_t b = 0; b < nsteps; ++b)
    if (curve[(size_t)b] > m) m = curve[(size_t)b];
  return m;
}

}  // namespace

void loudness_coeffs(int sr, double out[10]) {
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(kPi * f0 / (double)sr);
    const double Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    out[0] = (Vh + Vb * K / Q + K * K) / a0;
    out[1] = 2.0 * (K * K - Vh) / a0;
    out[2] = (Vh - Vb * K / Q + K * K) / a0;
    out[3] = 2.0 * (K * K - 1.0) / a0;
    out[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(kPi * f0 / (double)sr);
    const double a0 = 1.0 + K / Q + K * K;
    out[5] = 1.0;
    out[6] = -2.0;
    out[7] = 1.0;
    out[8] = 2.0 * (K * K - 1.0) / a0;
    out[9] = (1.0 - K / Q + K * K) / a0;
  }
}

const char *loud_steps_error(const mx_loud_step *steps, int64_t nsteps, int S) {
  for (int64_t b = 0; b < nsteps; ++b)
    if (steps[b].samples < 1 || steps[b].samples > S) return "a step's samples lie outside [1, S]";
  return nullptr;
}

void loudness_curve(const mx_loud_step *steps, int64_t nsteps, int S, int window, double *out) {
  const double den = (double)((int64_t)window * S);
  int64_t full = 0;  // full steps in a row up to and including b
  for (int64_t b = 0; b < nsteps; ++b) {
    full = steps[b].samples == S ? full + 1 : 0;
    out[b] = full >= window ? lufs(energy_sum(steps, b - window + 1, window) / den) : -kInf;
  }
}

void loudness_integrated(const mx_loud_step *steps, int64_t nsteps, int S, mx_loudness *out) {
  mx_loudness m{};
  const double den = (double)((int64_t)kBlockSteps * S);
  std::vector<double> z;
  for (int64_t j = 0; kBlockHop * j + kBlockSteps <= nsteps; ++j) {
    bool whole = true;
    for (int64_t b = kBlockHop * j; b < kBlockHop * j + kBlockSteps; ++b) whole = whole && steps[b].samples == S;
    if (!whole) continue;
    ++m.blocks;
    const double zj = energy_sum(steps, kBlockHop * j, kBlockSteps) / den;
    if (!std::isfinite(zj)) ++m.bad_blocks;
    else z.push_back(zj);
  }
  double sum_abs = 0.0;
  for (double zj : z)
    if (zj > kAbsGate) sum_abs += zj, ++m.passed_abs;
  m.integrated = -kInf;
  if (m.passed_abs > 0) {
    const double gate = 0.1 * (sum_abs / (double)m.passed_abs);
    double sum_rel = 0.0;
    for (double zj : z)
      if (zj > kAbsGate && zj > gate) sum_rel += zj, ++m.passed_rel;
    m.integrated = lufs(sum_rel / (double)m.passed_rel);
  }
  std::vector<double> curve((size_t)std::max<int64_t>(nsteps, 1));
  m.momentary_max = curve_max(steps, nsteps, S, kBlockSteps, curve);
  m.shortterm_max = curve_max(steps, nsteps, S, kShortSteps, curve);
  m.peak = 0.f;
  for (int64_t b = 0; b < nsteps; ++b)
    if (steps[b].peak > m.peak) m.peak = steps[b].peak;
  *out = m;
}

void loudness_range(const mx_loud_step *steps, int64_t nsteps, int S, mx_loudness_range_result *out) {
  mx_loudness_range_result r{};
  const double den = (double)((int64_t)kShortSteps * S);
  std::vector<double> z;
  int64_t full = 0;  // full steps in a row up to and including b, as loudness_curve counts them
  for (int64_t b = 0; b < nsteps; ++b) {
    full = steps[b].samples == S ? full + 1 : 0;
    if (b < kShortSteps - 1 || (b - (kShortSteps - 1)) % kBlockHop != 0 || full < kShortSteps) continue;
    ++r.values;
    const double zk = energy_sum(steps, b - kShortSteps + 1, kShortSteps) / den;
    if (!std::isfinite(zk)) ++r.bad;
    else z.push_back(zk);
  }
  double sum_abs = 0.0;
  int64_t passed_abs = 0;
  for (double zk : z)
    if (zk > kAbsGate) sum_abs += zk, ++passed_abs;
  std::vector<double> kept;
  if (passed_abs > 0) {
    const double gate = 0.01 * (sum_abs / (double)passed_abs);
    for (double zk : z)
      if (zk > kAbsGate && zk > gate) kept.push_back(zk);
  }
  std::sort(kept.begin(), kept.end());
  r.gated = (int64_t)kept.size();
  r.lra = 0.0, r.low_lufs = r.high_lufs = -kInf;
  if (r.gated > 0) {
    const double low = kept[(size_t)std::floor((double)(r.gated - 1) * 0.10 + 0.5)];
    const double high = kept[(size_t)std::floor((double)(r.gated - 1) * 0.95 + 0.5)];
    r.lra = 10.0 * std::log10(high / low);
    r.low_lufs = lufs(low), r.high_lufs = lufs(high);
  }
  *out = r;
}

bool note_loudness(const mx_loud_step *steps, int64_t nsteps, int S, const mx_note *notes, int64_t nnotes, double *out, int64_t *bad) {
  const int64_t total = nsteps > 0 ? (nsteps - 1) * S + steps[nsteps - 1].samples : 0;  // the samples the records cover
  for (int64_t i = 0; i < nnotes; ++i) {
    const int64_t start = notes[i].start_sample, end = notes[i].end_sample;
    *bad = i;
    if (start < 0 || end < start || end >= total) return false;
    int64_t lo = (start + S - 1) / S, hi = (end + 1) / S;  // the steps [lo, hi) lie inside the note
    if (hi <= lo) lo = ((start + end) / 2) / S, hi = lo + 1;
    double e = 0.0;
    int64_t samples = 0;
    bool finite = true;
    for (int64_t b = lo; b < hi; ++b) {
      finite = finite && std::isfinite(steps[b].energy);
      e += steps[b].energy;
      samples += steps[b].samples;
    }
    out[i] = finite ? lufs(e / (double)samples) : std::numeric_limits<double>::quiet_NaN();
  }
  return true;
}

double level_gain_points(const mx_note *notes, int64_t nnotes, const double *lufs_in, const mx_level_params &p, mx_gain_point *out) {
  std::vector<double> v;
  for (int64_t i = 0; i < nnotes; ++i)
    if (std::isfinite(lufs_in[i])) v.push_back(lufs_in[i]);
  std::sort(v.begin(), v.end());
  const size_t k = v.size();
  const double ref = k == 0 ? std::numeric_limits<double>::quiet_NaN() : k % 2 ? v[k / 2] : (v[k / 2 - 1] + v[k / 2]) / 2.0;
  for (int64_t i = 0; i < nnotes; ++i) {
    float amp = 1.f;
    if (std::isfinite(lufs_in[i])) {
      const double d = ref - lufs_in[i];
      double db = (d > 0.0 ? p.raise : p.lower) * d;
      db = db < -p.max_db ? -p.max_db : db > p.max_db ? p.max_db : db;
      amp = (float)std::pow(10.0, db / 20.0);
    }
    out[2 * i] = mx_gain_point{notes[i].start_sample, amp};
    out[2 * i + 1] = mx_gain_point{notes[i].end_sample, amp};
  }
  return ref;
}

double normalize_amp(double integrated, double peak, double target_lufs, double ceiling_db) {
  const double by_loudness = std::pow(10.0, (target_lufs - integrated) / 20.0), by_peak = std::pow(10.0, ceiling_db / 20.0) / peak;
  return by_loudness < by_peak ? by_loudness : by_peak;
}

}  // namespace mx
