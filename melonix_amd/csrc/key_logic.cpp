// key_logic.cpp — key, scale and tuning from a chroma sum or from notes; correction markers on a tuned grid (definitions:
// include/melonix_amd.h).  Pure host code, built with g++ -ffp-contract=off: tests/key_ref.py restates it in Python and
// expects the same doubles, so every sum below runs in the order written and nothing is reassociated.
#include "key_logic.h"

#include <cmath>

#include "f0_notes.h"

namespace mx {
namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kProfiles[2][12] = {{6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88},
                                     {6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17}};
constexpr int kDegrees[2][7] = {{0, 2, 4, 5, 7, 9, 11}, {0, 2, 3, 5, 7, 8, 10}};

// circular distance over the 36 bins
double circ(double b, double q) {
  const double d = std::fmod(std::fabs(b - q), 36.0);
  return d > 18.0 ? 36.0 - d : d;
}

// tuning in (-50, 50] cents and its confidence from the phasor (c, s) of summed weight w
void tuning_of(double c, double s, double w, double &tuning, double &conf) {
  tuning = conf = 0.0;
  const double h = std::sqrt(c * c + s * s);
  if (!(w > 0.0) || h == 0.0) return;
  tuning = 100.0 / (2.0 * kPi) * std::atan2(s, c);
  if (tuning <= -50.0) tuning += 100.0;
  conf = h / w;
}

// the 24 correlations of the twelve-class profile p
mx_key key_of_profile(const double (&p)[12], double tuning, double conf) {
  mx_key key{0, 0, 0, 0, tuning, conf, 0.0, 0.0};
  double s = 0.0;
  for (int c = 0; c < 12; ++c) s += p[c];
  const double pm = s / 12.0;
  double dp[12], vp = 0.0;
  for (int c = 0; c < 12; ++c) dp[c] = p[c] - pm;
  for (int c = 0; c < 12; ++c) vp += dp[c] * dp[c];
  if (!(vp > 0.0) || !std::isfinite(vp)) return key;
  double r[24];
  for (int mode = 0; mode < 2; ++mode) {
    const double *prof = kProfiles[mode];
    s = 0.0;
    for (int c = 0; c < 12; ++c) s += prof[c];
    const double qm = s / 12.0;
    double dq[12], vq = 0.0;
    for (int c = 0; c < 12; ++c) dq[c] = prof[c] - qm;
    for (int c = 0; c < 12; ++c) vq += dq[c] * dq[c];
    const double den = std::sqrt(vp * vq);
    for (int tonic = 0; tonic < 12; ++tonic) {
      double num = 0.0;
      for (int c = 0; c < 12; ++c) num += dp[c] * dq[(c - tonic + 12) % 12];
      r[12 * mode + tonic] = num / den;
    }
  }
  int best = 0;
  for (int i = 1; i < 24; ++i)
    if (r[i] > r[best]) best = i;
  double second = -HUGE_VAL;
  for (int i = 0; i < 24; ++i)
    if (i != best && r[i] > second) second = r[i];
  key.tonic = best % 12;
  key.mode = best / 12;
  key.correlation = r[best];
  key.clarity = r[best] - second;
  for (const int d : kDegrees[key.mode]) key.scale_mask |= 1 << ((key.tonic + d) % 12);
  return key;
}

}  // namespace

mx_key key_from_sum(const double *sum40) {
  double S[40];
  for (int i = 0; i < 40; ++i) S[i] = std::isfinite(sum40[i]) ? sum40[i] : 0.0;
  double tuning, conf;
  tuning_of(S[36], S[37], S[38], tuning, conf);
  double p[12] = {};
  for (int c = 0; c < 12; ++c) {
    const double q = (100.0 * c + tuning) / (100.0 / 3.0);
    for (int b = 0; b < 36; ++b) {
      const double w = 1.0 - circ((double)b, q) / 2.0;
      if (w > 0.0) p[c] += S[b] * w;
    }
  }
  return key_of_profile(p, tuning, conf);
}

mx_key key_from_notes(const mx_note *notes, int64_t count) {
  double cs = 0.0, sn = 0.0, wt = 0.0;
  for (int64_t i = 0; i < count; ++i) {
    if (notes[i].frames <= 0) continue;
    const double w = (double)notes[i].frames, theta = 2.0 * kPi * (notes[i].note - std::rint(notes[i].note));
    cs += w * std::cos(theta);
    sn += w * std::sin(theta);
    wt += w;
  }
  double tuning, conf;
  tuning_of(cs, sn, wt, tuning, conf);
  double p[12] = {};
  for (int64_t i = 0; i < count; ++i) {
    if (notes[i].frames <= 0) continue;
    int c = (int)std::fmod(std::rint(notes[i].note - tuning / 100.0), 12.0);
    if (c < 0) c += 12;
    p[c] += (double)notes[i].frames;
  }
  return key_of_profile(p, tuning, conf);
}

std::vector<mx_chroma_job> key_windows(int64_t count, int64_t window_frames, int64_t window_hop) {
  std::vector<mx_chroma_job> out;
  if (window_frames > 0)
    for (int64_t first = 0; first < count; first += window_hop)
      out.push_back(mx_chroma_job{first, window_frames < count - first ? window_frames : count - first});
  return out;
}

void correction_markers_tuned(const mx_note *notes, int64_t count, double strength, int mask, double tuning_cents, mx_marker *out) {
  const double t = tuning_cents / 100.0;
  for (int64_t i = 0; i < count; ++i) {
    const mx_note &n = notes[i];
    const double b = strength * ((snap_note(n.note - t, mask) + t) - n.note);
    out[2 * i] = mx_marker{n.start_sample, n.note, 0.0, b};
    out[2 * i + 1] = mx_marker{n.end_sample, n.note, 0.0, b};
  }
}

}  // namespace mx
