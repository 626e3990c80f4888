// tempo_logic.cpp — see tempo_logic.h.  Every expression here is repeated by tests/tempo_ref.py with Python's math module (the
// same libm): candidate periods, prior and result come out identical.
#include "tempo_logic.h"

#include <algorithm>
#include <cmath>

namespace mx {

const mx_tempo_params kTempoDefaults{30.0, 250.0, 64, 4, 2048, 512, 120.0, 1.0, 0.5};

tempo::SmoothWeights smooth_weights(int W) {
  tempo::SmoothWeights w{};
  for (int d = 0; d <= W && d <= tempo::kMaxWidth; ++d) w.h[d] = (float)(0.5 + 0.5 * std::cos(M_PI * (double)d / (double)(W + 1)));
  return w;
}

const char *tempo_params_error(const mx_tempo_params &p) {
  if (!(p.bpm_min >= 30.0 && p.bpm_max <= 250.0 && p.bpm_min < p.bpm_max)) return "bpm_min / bpm_max: inside [30, 250], min < max";
  if (p.per_octave < 8 || p.per_octave > 128) return "per_octave outside [8, 128]";
  if (p.smooth < 0 || p.smooth > tempo::kMaxWidth) return "smooth outside [0, 32]";
  if (p.window_frames < 64 || p.window_frames > 65536) return "window_frames outside [64, 65536]";
  if (p.stride_frames < 1 || p.stride_frames > p.window_frames) return "stride_frames outside [1, window_frames]";
  if (!std::isfinite(p.prior_bpm) || !(p.prior_bpm > 0.0)) return "prior_bpm must be finite and > 0";
  if (!std::isfinite(p.prior_octaves) || !(p.prior_octaves > 0.0)) return "prior_octaves must be finite and > 0";
  if (!(p.lock_ratio >= 0.0 && p.lock_ratio <= 1.0)) return "lock_ratio outside [0, 1]";
  return nullptr;
}

const char *comb_job_error(const mx_comb_job &job, int64_t count) {
  if (job.frames < 1) return "a job needs frames >= 1";
  if (job.first < 0 || (int64_t)job.first + job.frames > count) return "a job's segment leaves the curve";
  if (job.period_q16 < tempo::kMinPeriod || job.period_q16 > tempo::kMaxPeriod) return "a job's period is outside [2, 4096] frames";
  return nullptr;
}

const char *tempo_ladder(const mx_tempo_params &p, int sampleRate, int hop, TempoLadder &out) {
  if (sampleRate <= 0) return "sample rate must be > 0";
  if (hop < 1 || hop > 16384) return "hop outside [1, 16384]";
  out = TempoLadder{};
  out.fr = (double)sampleRate / (double)hop;
  for (int c = 0;; ++c) {
    const double bpm = p.bpm_max * std::exp2(-(double)c / (double)p.per_octave);
    if (!(bpm >= p.bpm_min)) break;
    const double q = std::floor(60.0 * out.fr / bpm * 65536.0 + 0.5);
    if (!(q >= (double)tempo::kMinPeriod && q <= (double)tempo::kMaxPeriod))
      return "a candidate's beat period is outside [2, 4096] frames at this sample rate and hop";
    const double z = std::log2(bpm / p.prior_bpm) / p.prior_octaves;
    out.bpm.push_back(bpm);
    out.period.push_back((uint32_t)q);
    out.prior.push_back(std::exp(-0.5 * (z * z)));
  }
  return nullptr;
}

int tempo_estimate(const float *e, int64_t count, int64_t first_frame, const mx_tempo_params &p, const TempoLadder &ladder,
                   const CombRunner &comb, mx_tempo &out, std::vector<mx_tempo_window> &windows) {
  out = mx_tempo{};
  windows.clear();
  double total = 0.0;
  bool any = false;
  for (int64_t f = 0; f < count; ++f) {
    total += (double)e[f];
    any = any || e[f] != 0.f;
  }
  if (!any) return 0;  // (empty or all zero: the empty result)
  const double fr = ladder.fr;
  const int64_t nc = (int64_t)ladder.period.size();
  const int64_t win = std::min<int64_t>(p.window_frames, count);
  const int64_t nw = count < p.window_frames ? 1 : (count - p.window_frames) / p.stride_frames + 1;

  // coarse: one job per (window, candidate)
  std::vector<mx_comb_job> jobs((size_t)(nw * nc));
  for (int64_t w = 0; w < nw; ++w)
    for (int64_t c = 0; c < nc; ++c)
      jobs[(size_t)(w * nc + c)] = mx_comb_job{(int32_t)(w * p.stride_frames), (int32_t)win, ladder.period[(size_t)c]};
  std::vector<mx_comb> T(jobs.size());
  if (const int rc = comb(jobs, T)) return rc;
  int64_t cstar = 0;
  double abest = 0.0;
  for (int64_t c = 0; c < nc; ++c) {
    double s = 0.0;
    for (int64_t w = 0; w < nw; ++w) s += (double)T[(size_t)(w * nc + c)].score;
    const double a = s * ladder.prior[(size_t)c];
    if (c == 0 || a > abest) {
      abest = a;
      cstar = c;
    }
  }
  int64_t anchor = 0;
  for (int64_t w = 1; w < nw; ++w)
    if (T[(size_t)(w * nc + cstar)].score > T[(size_t)(anchor * nc + cstar)].score) anchor = w;
  windows.resize((size_t)nw);
  for (int64_t w = 0; w < nw; ++w) {
    int64_t cw = 0;
    double vbest = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
      const double v = (double)T[(size_t)(w * nc + c)].score * ladder.prior[(size_t)c];
      if (c == 0 || v > vbest) {
        vbest = v;
        cw = c;
      }
    }
    windows[(size_t)w] = mx_tempo_window{(int32_t)(first_frame + w * p.stride_frames), (int32_t)win,
                                         (float)(60.0 * fr * 65536.0 / (double)ladder.period[(size_t)cw]),
                                         T[(size_t)(w * nc + cw)].score};
  }

  // refinement: segment and resolution grow together
  int64_t period = ladder.period[(size_t)cstar];
  int64_t step = std::max<int64_t>(1, (int64_t)((double)period * (std::exp2(1.0 / (double)p.per_octave) - 1.0) / 8.0));
  int64_t L = win;
  const int64_t centre = anchor * p.stride_frames + win / 2;
  double base = 0.0;
  int64_t kept_first = 0, kept_len = 0;
  mx_comb kept{};
  int levels = 0;
  for (;;) {
    const int64_t len = std::min(L, count);
    const int64_t first = std::min(std::max<int64_t>(centre - L / 2, 0), count - len);
    std::vector<int> ks;
    jobs.clear();
    for (int k = -12; k <= 12; ++k) {
      const int64_t q = period + (int64_t)k * step;
      if (q < (int64_t)tempo::kMinPeriod || q > (int64_t)tempo::kMaxPeriod) continue;
      ks.push_back(k);
      jobs.push_back(mx_comb_job{(int32_t)first, (int32_t)len, (uint32_t)q});
    }
    std::vector<mx_comb> rec(jobs.size());
    if (const int rc = comb(jobs, rec)) return rc;
    size_t b = 0;
    for (size_t i = 1; i < rec.size(); ++i) {
      const int ka = std::abs(ks[i]), kb = std::abs(ks[b]);
      if (rec[i].score > rec[b].score || (rec[i].score == rec[b].score && (ka < kb || (ka == kb && ks[i] < ks[b])))) b = i;
    }
    if (levels == 0) base = (double)rec[b].score;
    else if ((double)rec[b].score < p.lock_ratio * base) break;
    period = (int64_t)jobs[b].period_q16;
    kept_first = first;
    kept_len = len;
    kept = rec[b];
    ++levels;
    if (len == count) break;
    L *= 8;
    step = std::max<int64_t>(1, step / 8);
  }

  const double g = ((double)period / 65536.0) / fr;
  const double sp = (double)kept.prev, s0 = (double)kept.score, sn = (double)kept.next;
  const double curv = sp - 2.0 * s0 + sn;
  double delta = 0.0;
  if (curv < 0.0) {
    delta = 0.5 * (sp - sn) / curv;
    delta = delta < -0.5 ? -0.5 : delta > 0.5 ? 0.5 : delta;
  }
  double offset = std::fmod(((double)(first_frame + kept_first + (int64_t)kept.phase) + delta) / fr, g);
  if (offset < 0.0) offset += g;
  if (!(offset < g)) offset = 0.0;
  const double mean = total / (double)count;
  out.bpm = 60.0 / g;
  out.offset = offset;
  out.score = kept.score;
  out.clarity = mean > 0.0 ? (float)(s0 / mean) : 0.f;
  out.locked_frames = kept_len;
  out.levels = levels;
  return 0;
}

}  // namespace mx
