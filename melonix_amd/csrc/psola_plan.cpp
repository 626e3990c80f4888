// psola_plan.cpp — see psola_plan.h.  Built with g++ -ffp-contract=off: tests/psola_ref.py restates the plan in Python and
// expects the same doubles.
#include "psola_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>

#include "host_logic.h"

namespace mx {

namespace {

constexpr double kTrackerHalf = 2048.0;  // W of the f0 tracker (include/melonix_amd.h: N = 4096, W = N/2)

int invalid(std::string &err, const char *fmt, long long a = 0, long long b = 0) {
  char buf[160];
  snprintf(buf, sizeof buf, fmt, a, b);
  err = buf;
  return MX_ERR_INVALID;
}

// The plan: arguments checked, then the marks, one record per synthesis mark.  The window fields are the same for both record
// kinds; source(record, a_m, s, m) — the record, its analysis mark, its synthesis mark and the mark's index — then fills in
// where the grain reads the source.  bend: null, or count semitone values over the source's frames, added to the markers' bend
// at the frame whose measurement is centred on the grain's analysis mark (fr below).
template <class Rec, class Source>
int plan_marks(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params &p,
               const mx_marker *markers, int nmarkers, const float *bend, std::vector<Rec> &grains, int64_t &nsamples,
               std::string &err, Source source) {
  grains.clear();
  nsamples = 0;
  if (n < 0 || n > (int64_t)INT32_MAX - 2 * MX_AUDIO_PAD) return invalid(err, "%lld samples: outside [0, INT32_MAX - 2*MX_AUDIO_PAD]", n);
  if (sampleRate <= 0) return invalid(err, "sample rate %lld", sampleRate);
  if (hop < 1 || hop > 16384) return invalid(err, "hop %lld outside [1, 16384]", hop);
  if (count != (n + hop - 1) / hop) return invalid(err, "%lld records for a file of %lld frames", count, (n + hop - 1) / hop);
  if (count > 0 && !track) return invalid(err, "null track");
  if (!std::isfinite(p.threshold) || !std::isfinite(p.rms_floor)) return invalid(err, "threshold / rms_floor is not finite");
  if (!(p.unvoiced_period >= 32.f && p.unvoiced_period <= (float)MX_PSOLA_MAX_HALF))
    return invalid(err, "unvoiced period outside [32, %lld]", MX_PSOLA_MAX_HALF);
  for (int64_t h = 0; bend && h < count; ++h)
    if (!std::isfinite(bend[h])) return invalid(err, "bend of frame %lld is not finite", h);
  // the output length, and the marker checks, are the phase vocoder's
  PvPlan pv;
  if (const int rc = build_pv_plan(markers, nmarkers, sampleRate, n, pv, err)) return rc;
  const int64_t L = pv.n_out;
  if (L > (int64_t)INT32_MAX - 2 * kPsolaReach) return invalid(err, "%lld output samples: centres beyond int32", L);
  nsamples = L;
  if (n == 0 || L == 0) return MX_OK;

  const double U = (double)p.unvoiced_period;
  // the frame nearest to source position x
  auto frame_at = [&](double x) {
    const double h = std::floor(x / (double)hop + 0.5);
    return (int64_t)(h < 0. ? 0. : (h > (double)(count - 1) ? (double)(count - 1) : h));
  };
  // P(x) and voiced(x): period_of(x) < 0 marks an unvoiced frame
  auto period_at = [&](double x, bool &voiced) {
    const mx_f0 &r = track[frame_at(x)];
    voiced = r.tau > 0 && r.aperiodicity < p.threshold && r.rms >= p.rms_floor && std::isfinite(r.period) && r.period >= 2.f &&
             r.period <= (float)MX_PSOLA_MAX_HALF;
    return voiced ? (double)r.period : U;
  };

  // analysis marks
  std::vector<double> a, per;
  std::vector<char> vo;
  std::vector<int64_t> fr;  // the frame each mark reads the curve at (where there is one)
  for (double am = 0.;;) {
    bool v;
    const double pm = period_at(am, v);
    if (!(am - pm < (double)n)) break;
    a.push_back(am);
    per.push_back(pm);
    vo.push_back((char)v);
    // the tracker's frame h reads samples [h hop - 2048, h hop + tau): what it measures lies (2048 - period) / 2 before h hop
    if (bend) fr.push_back(frame_at(am + (kTrackerHalf - pm) / 2.0));
    am = am + pm;
  }

  // synthesis marks
  const TimeMap tm(markers, nmarkers, sampleRate, n);
  const double sr = (double)sampleRate;
  int hint_s = -1, hint_b = -1;
  for (double s = 0.;;) {
    const double t = s / sr;
    const int64_t src = std::max<int64_t>(tm.time2sample(t, hint_s), 0);
    // the nearest mark (the marks are strictly increasing); beyond the last mark, the last.  Ties go to the HIGHER index:
    // time2sample truncates, so the position it stands for lies in [src, src + 1) — at a period of 2 the identity map gives
    // src = s - 1 for some even s, halfway between the mark the grain belongs to and the one before
    size_t m = (size_t)(std::upper_bound(a.begin(), a.end(), (double)src) - a.begin());
    if (m == a.size() || (m > 0 && (double)src - a[m - 1] < a[m] - (double)src)) --m;
    const double H = per[m];
    if (!(s - H < (double)L)) break;
    double r = 1.;
    if (vo[m]) {
      double b = (double)tm.time2pitchbend(t, hint_b);
      if (bend) b = b + (double)bend[fr[m]];
      r = std::exp2(b / 12.0);
      r = !(r >= 0.5) ? 0.5 : (r > 2. ? 2. : r);
    }
    Rec g{};
    g.out_lo = (int32_t)std::max(0., std::floor(s - H) + 1.);
    g.out_hi = (int32_t)std::min((double)L, std::ceil(s + H));
    const double cfl = std::floor(s);
    g.centre = (int32_t)cfl;
    g.centre_frac = (float)(s - cfl);
    if (g.centre_frac >= 1.f) {
      g.centre += 1;
      g.centre_frac = 0.f;
    }
    g.inv_half = (float)(1. / H);
    source(g, a[m], s, (int32_t)m);
    grains.push_back(g);
    s = s + H / r;
  }
  return MX_OK;
}

// The record's own fields, beyond the window ...
int check_fields(const mx_psola_grain &r, int64_t k, std::string &err) {
  if (!(r.src_frac >= 0.f && r.src_frac < 1.f)) return invalid(err, "grain %lld: a fraction outside [0, 1)", k);
  return MX_OK;
}
int check_fields(const mx_psola_fgrain &r, int64_t k, std::string &err) {
  if (r.step < kPsolaStepMin || r.step > kPsolaStepMax) return invalid(err, "grain %lld: step outside [32768, 131072]", k);
  if (r.src_q >= kPsolaStepOne) return invalid(err, "grain %lld: src_q is not below 65536", k);
  return MX_OK;
}

// ... and the lowest and highest source index its (non-empty) window reads: psola_kernels.hip's psola_source, which takes
// the samples at idx and idx + 1, at the window's first and last output
void source_span(const mx_psola_grain &r, int64_t &lo, int64_t &hi) {
  lo = (int64_t)r.out_lo + r.src_off;
  hi = (int64_t)r.out_hi + r.src_off;
}
// (pos rises with i)
void source_span(const mx_psola_fgrain &r, int64_t &lo, int64_t &hi) {
  auto idx = [&](int64_t i) { return ((int64_t)r.src_idx * 65536 + (int64_t)r.src_q + (int64_t)r.step * (i - (int64_t)r.centre)) >> 16; };
  lo = idx(r.out_lo);
  hi = idx((int64_t)r.out_hi - 1) + 1;
}

template <class Rec>
int check_grains(const Rec *g, int64_t ngrains, int64_t nsamples, int64_t n, std::string &err) {
  double prev = -HUGE_VAL;  // the last key
  for (int64_t k = 0; k < ngrains; ++k) {
    const Rec &r = g[k];
    if (const int rc = check_fields(r, k, err)) return rc;
    if (!(r.centre_frac >= 0.f && r.centre_frac < 1.f)) return invalid(err, "grain %lld: a fraction outside [0, 1)", k);
    const double key = (double)r.centre + (double)r.centre_frac;
    if (!(key > prev)) return invalid(err, "grain %lld: centre + centre_frac does not increase", k);
    prev = key;
    if (r.out_lo < 0 || r.out_lo > r.out_hi || (int64_t)r.out_hi > nsamples)
      return invalid(err, "grain %lld: window outside the %lld output samples", k, nsamples);
    if (!std::isfinite(r.inv_half) || !(r.inv_half >= 1.f / (float)MX_PSOLA_MAX_HALF))
      return invalid(err, "grain %lld: inv_half is not finite or below 1/%lld", k, MX_PSOLA_MAX_HALF);
    if (r.out_lo == r.out_hi) continue;  // (no output reads it)
    if ((int64_t)r.out_lo < (int64_t)r.centre - kPsolaReach || (int64_t)r.out_hi - 1 > (int64_t)r.centre + kPsolaReach)
      return invalid(err, "grain %lld: window beyond centre +- %lld", k, kPsolaReach);
    int64_t lo, hi;
    source_span(r, lo, hi);
    if (lo < -(int64_t)MX_AUDIO_PAD || hi > n + (int64_t)MX_AUDIO_PAD - 1) return invalid(err, "grain %lld: reads the source outside its pads", k);
  }
  return MX_OK;
}

}  // namespace

int build_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params &p,
                     const mx_marker *markers, int nmarkers, std::vector<mx_psola_grain> &grains, int64_t &nsamples,
                     std::string &err, const float *bend) {
  return plan_marks(n, sampleRate, hop, track, count, p, markers, nmarkers, bend, grains, nsamples, err,
                    [](mx_psola_grain &g, double am, double s, int32_t m) {
                      const double d = am - s, dfl = std::floor(d);
                      g.src_off = (int32_t)dfl;
                      g.src_frac = (float)(d - dfl);
                      if (g.src_frac >= 1.f) {
                        g.src_off += 1;
                        g.src_frac = 0.f;
                      }
                      g.mark = m;
                    });
}

int build_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params &p,
                     const mx_marker *markers, int nmarkers, const mx_formant_point *points, int npoints,
                     std::vector<mx_psola_fgrain> &fgrains, int64_t &nsamples, std::string &err, const float *bend) {
  fgrains.clear();
  nsamples = 0;
  if (npoints < 0 || (npoints > 0 && !points)) return invalid(err, "bad formant curve: %lld points", npoints);
  for (int j = 0; j < npoints; ++j) {
    if (!std::isfinite(points[j].semitones)) return invalid(err, "formant point %lld: semitones not finite", j);
    if (j > 0 && !(points[j].sample > points[j - 1].sample)) return invalid(err, "formant point %lld: samples do not increase", j);
  }
  // F(x): piecewise linear between the points, constant outside them
  auto curve = [&](double x) {
    if (npoints == 0) return 0.;
    if (x < (double)points[0].sample) return (double)points[0].semitones;
    if (x >= (double)points[npoints - 1].sample) return (double)points[npoints - 1].semitones;
    const mx_formant_point *hi =
        std::upper_bound(points, points + npoints, x, [](double v, const mx_formant_point &q) { return v < (double)q.sample; });
    const mx_formant_point &q0 = hi[-1], &q1 = hi[0];
    return (double)q0.semitones +
           (x - (double)q0.sample) * ((double)q1.semitones - (double)q0.semitones) / ((double)q1.sample - (double)q0.sample);
  };
  return plan_marks(n, sampleRate, hop, track, count, p, markers, nmarkers, bend, fgrains, nsamples, err,
                    [&](mx_psola_fgrain &f, double am, double, int32_t) {
                      double phi = std::exp2(curve(am) / 12.0);
                      phi = !(phi >= 0.5) ? 0.5 : (phi > 2. ? 2. : phi);
                      f.step = (uint32_t)(int)std::floor(phi * 65536.0 + 0.5);
                      const double p0 = am - ((double)f.step / 65536.0) * (double)f.centre_frac;
                      const int64_t q = (int64_t)std::floor(p0 * 65536.0 + 0.5);
                      f.src_idx = (int32_t)(q >> 16);
                      f.src_q = (uint32_t)(q & 65535);
                    });
}

int check_psola_grains(const mx_psola_grain *g, int64_t ngrains, int64_t nsamples, int64_t n, std::string &err) {
  return check_grains(g, ngrains, nsamples, n, err);
}
int check_psola_grains(const mx_psola_fgrain *g, int64_t ngrains, int64_t nsamples, int64_t n, std::string &err) {
  return check_grains(g, ngrains, nsamples, n, err);
}

}  // namespace mx
