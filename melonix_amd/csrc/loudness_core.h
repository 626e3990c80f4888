// loudness_core.h — the arithmetic of the loudness records (loudness_kernels.hip; definition: include/melonix_amd.h "Loudness
// and note levelling"), plain C++ for the device and for tests/emu/loudness_emu.cpp: the geometry, the K-weighting recurrence and a
// step's sums, sample by sample.  Built with -ffp-contract=off: every product is rounded before its sum.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"
#include "step_core.h"

namespace mx {
namespace loud {

constexpr int kGroupSteps = 10;  // G

// S, W and the step / group counts of a take (sr in range: the caller's check)
struct Geometry {
  int64_t n;
  int S, W;
  int64_t steps, groups;
};
MX_STEP_HD Geometry geometry(int64_t n, int sr) {
  Geometry q;
  q.n = n;
  q.S = step::step_samples(sr);
  q.W = 4 * ((32 * sr + 1499) / 1500);
  q.steps = step::step_count(n, sr);
  q.groups = (q.steps + kGroupSteps - 1) / kGroupSteps;
  return q;
}

// {b0, b1, b2, a1, a2} of the shelf, {c0, c1, c2, d1, d2} of the high-pass: mx_loudness_coeffs' ten values
struct Coeffs {
  double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2;
};

// The two stages' states and the sums of the step being walked
struct Lane {
  double s1, s2, t1, t2, energy;
  float peak;
};
MX_STEP_HD Lane lane_zero() { return Lane{0.0, 0.0, 0.0, 0.0, 0.0, 0.f}; }
MX_STEP_HD void step_zero(Lane &l) { l.energy = 0.0, l.peak = 0.f; }

// one sample through both stages -> z
MX_STEP_HD double filter(const Coeffs &c, Lane &l, float x) {
  const double v = (double)x;
  const double y = c.b0 * v + l.s1;
  l.s1 = (c.b1 * v - c.a1 * y) + l.s2;
  l.s2 = c.b2 * v - c.a2 * y;
  const double z = c.c0 * y + l.t1;
  l.t1 = (c.c1 * y - c.d1 * z) + l.t2;
  l.t2 = c.c2 * y - c.d2 * z;
  return z;
}
// a sample of a step: the energy in ascending order, the peak over what is not NaN (a NaN compares false)
MX_STEP_HD void accumulate(Lane &l, float x, double z) {
  l.energy += z * z;
  const float m = x < 0.f ? -x : x;
  if (m > l.peak) l.peak = m;
}
MX_STEP_HD mx_loud_step record(const Lane &l, int32_t samples) {
  mx_loud_step r;
  r.energy = l.energy;
  r.peak = l.peak;
  r.samples = samples;
  return r;
}

}  // namespace loud
}  // namespace mx
