// gain_core.h — the arithmetic of the source gain (gain_kernels.hip; definition: include/melonix_amd.h "Balance"), plain C++
// for the device and for tests/emu/sibilant_emu.cpp.  Built with -ffp-contract=off: the product is rounded before the sum.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_GAIN_HD __host__ __device__ __forceinline__
#else
#define MX_GAIN_HD inline
#endif

namespace mx {
namespace gain {

// The segment around a sample, held in registers while the walk stays inside it: j = the number of points whose sample is
// <= i (npts >= 1).  j == 0 and j == npts are the constant ends; a segment whose two amps are equal — every sample outside
// the ramps — needs no quotient: (a1 - a0) * t is 0 for every finite t, and a0 + 0 is a0.
struct Segment {
  double a0, da, den;  // g = a0 + da * ((double)(i - s0) / den)
  int64_t s0, next;    // next: the first sample of the segment behind this one (INT64_MAX: none)
  bool flat;
};
MX_GAIN_HD Segment segment_at(const mx_gain_point *pts, int64_t npts, int64_t j) {
  Segment g;
  g.next = j < npts ? (int64_t)pts[j].sample : INT64_MAX;
  g.da = 0.0, g.den = 1.0, g.s0 = 0, g.flat = true;
  if (j <= 0 || j >= npts) {
    g.a0 = (double)pts[j <= 0 ? 0 : npts - 1].amp;
    return g;
  }
  const mx_gain_point p0 = pts[j - 1], p1 = pts[j];
  g.a0 = (double)p0.amp;
  g.flat = p0.amp == p1.amp;
  g.da = (double)p1.amp - g.a0;
  g.s0 = (int64_t)p0.sample;
  g.den = (double)((int64_t)p1.sample - (int64_t)p0.sample);
  return g;
}
// g(i) for a sample inside the segment
MX_GAIN_HD double gain_at(const Segment &g, int64_t i) { return g.flat ? g.a0 : g.a0 + g.da * ((double)(i - g.s0) / g.den); }
// out = (float)((double)x * g)
MX_GAIN_HD float gained(float x, double g) { return (float)((double)x * g); }

}  // namespace gain
}  // namespace mx
