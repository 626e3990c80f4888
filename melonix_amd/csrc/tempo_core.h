// tempo_core.h — the arithmetic of the tempo estimator's two kernels (tempo_kernels.hip; definition: include/melonix_amd.h
// "Tempo and grid-offset estimation") as plain host/device C++: one smoothed value, one phase's score, one job's record from
// its row of scores.  tests/emu/tempo_emu.cpp runs the same functions on the CPU.  Compile with -ffp-contract=off: every
// product is rounded before it is added.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/melonix_amd.h"

#if defined(__HIPCC__)
#define MX_TEMPO_HD __host__ __device__ __forceinline__
#define MX_TEMPO_UNROLL _Pragma("unroll")
#else
#define MX_TEMPO_HD inline
#define MX_TEMPO_UNROLL
#endif

namespace mx {
namespace tempo {

constexpr int kMaxWidth = 32;      // W
constexpr int kMaxPhases = 4096;   // ceil(period) of the longest period
constexpr int kThreads = 256;      // of a comb workgroup: thread t takes phases t, t + 256, ..
constexpr uint32_t kMinPeriod = 2u << 16, kMaxPeriod = 4096u << 16;
// terms of a phase's sum fetched at a time (phase_score); 1 is the plain loop.  The bytes do not depend on it: -DMX_TEMPO_FETCH=1
// builds the library tests/tools/tempo_hour.py --other-lib times against
#ifndef MX_TEMPO_FETCH
#define MX_TEMPO_FETCH 8
#endif
constexpr int kFetch = MX_TEMPO_FETCH;

// h_|d|, d <= W, built on the host in binary64 (tempo_logic.cpp: smooth_weights) and passed to the kernel by value
struct SmoothWeights {
  float h[kMaxWidth + 1];
};

// v, 0 where it is not finite
MX_TEMPO_HD float finite_or_zero(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return (u & 0x7f800000u) == 0x7f800000u ? 0.f : v;
}

// e_f: 2W + 1 taps in ascending d from 0.f; taps outside [0, count) are zeros
MX_TEMPO_HD float smooth_at(const float *o, int64_t count, int64_t f, int W, const SmoothWeights &w) {
  float acc = 0.f;
  for (int d = -W; d <= W; ++d) {
    const int64_t g = f + d;
    const float v = g >= 0 && g < count ? finite_or_zero(o[g]) : 0.f;
    acc = acc + w.h[d < 0 ? -d : d] * v;
  }
  return acc;
}

// ceil(period_q16 / 65536), clamped to what a row holds (a job in range never meets the clamp)
MX_TEMPO_HD int phases(uint32_t period_q16) {
  const uint32_t n = (uint32_t)(((uint64_t)period_q16 + 65535u) >> 16);
  return n < 1u ? 1 : n > (uint32_t)kMaxPhases ? kMaxPhases : (int)n;
}

// one term of a phase's sum: the curve at the Q16 position pos, the index clamped into [0, last]
MX_TEMPO_HD float comb_term(const float *e, int64_t last, int64_t pos) {
  int64_t i0 = pos >> 16, i1 = i0 + 1;
  i0 = i0 < 0 ? 0 : i0 > last ? last : i0;
  i1 = i1 < 0 ? 0 : i1 > last ? last : i1;
  const float fr = (float)(pos & 65535) * (1.f / 65536.f);
  return (1.f - fr) * e[i0] + fr * e[i1];
}

// score_phi of a job over the curve e[0, count), count >= 1.  Every index is clamped into [0, count - 1] and J to count: a job
// outside its range reads the curve's own values and nothing else.  The terms are fetched kFetch (eight) at a time — their loads do not
// wait for one another — and added one by one in ascending j: the sum's bytes are those of the plain loop.
MX_TEMPO_HD float phase_score(const float *e, int64_t count, const mx_comb_job &job, int phi) {
  const int64_t period = job.period_q16 ? (int64_t)job.period_q16 : 1;
  const int64_t start = ((int64_t)job.first + phi) * 65536, lim = ((int64_t)job.first + job.frames - 1) * 65536;
  if (start > lim) return 0.f;
  int64_t J = (lim - start) / period + 1;
  if (J > count) J = count;
  const int64_t last = count - 1;
  double S = 0.0;
  int64_t pos = start, j = 0;
  for (; j + kFetch <= J; j += kFetch, pos += kFetch * period) {
    float x[kFetch];
    MX_TEMPO_UNROLL
    for (int u = 0; u < kFetch; ++u) x[u] = comb_term(e, last, pos + u * period);
    MX_TEMPO_UNROLL
    for (int u = 0; u < kFetch; ++u) S += (double)x[u];
  }
  for (; j < J; ++j, pos += period) S += (double)comb_term(e, last, pos);
  return (float)(S / (double)J);
}

// which of two (score, phase) pairs the record takes: the higher score, the lower phase among equals
MX_TEMPO_HD bool better(float sa, int pa, float sb, int pb) { return sa > sb || (sa == sb && pa < pb); }

// the record of a job whose phases scored row[0, nph), the best of them at `phase`
MX_TEMPO_HD mx_comb record_at(const float *row, int nph, int phase) {
  mx_comb r;
  r.score = row[phase];
  r.phase = phase;
  r.prev = row[phase == 0 ? nph - 1 : phase - 1];
  r.next = row[phase + 1 == nph ? 0 : phase + 1];
  return r;
}

}  // namespace tempo
}  // namespace mx
