// chroma_core.h — the arithmetic of the chroma record behind the N = 4096 transform (definition: include/melonix_amd.h "Key,
// scale and tuning reference"), written once for chroma_kernels.hip and for tests/emu/chroma_emu.cpp, which runs it thread by
// thread on the CPU; and the launch interface of the unit.  Every operation is f32 and rounds as written (-ffp-contract=off
// on both sides).  Private to those two.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_CHROMA_HD __host__ __device__ __forceinline__
#else
#define MX_CHROMA_HD inline __attribute__((always_inline))
#endif

#include "../../include/melonix_amd.h"

namespace mx {
namespace chroma {

constexpr int kN = 4096, kBins = 2048, kCols = 40, kPcp = 36;
// No two neighbouring bins are peaks (m[k] > m[k-1] and m[k-1] >= m[k] cannot both hold), and the band ends at 2046
constexpr int kMaxPeaks = 1023;
static_assert(sizeof(mx_chroma_rec) == kCols * sizeof(float), "a record is forty floats");

// the magnitude image: bin k at k + k/16, so that a thread's 16 consecutive bins (and their two neighbours) sit on their own banks
MX_CHROMA_HD int mag_idx(int k) { return k + (k >> 4); }
constexpr int kMagLen = kBins + kBins / 16;

// One peak as the forty columns need it: weight, place in profile bins [0, 36], the weighted tuning phasor
struct Peak {
  float m, p, c, s;
};

// the peak at bin k from its magnitude and its neighbours' (ma, mb, mc = m[k-1], m[k], m[k+1]); bin_hz = sr / 4096
MX_CHROMA_HD Peak peak_of(int k, float ma, float mb, float mc, float bin_hz) {
  const float la = logf(ma), lb = logf(mb), lc = logf(mc);
  const float den = 2.0f * ((la - 2.0f * lb) + lc);
  float delta = 0.f;
  if (den < 0.f && __builtin_isfinite(la) && __builtin_isfinite(lb) && __builtin_isfinite(lc)) delta = (la - lc) / den;
  delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
  const float f = ((float)k + delta) * bin_hz;
  const float cents = 1200.0f * log2f(f / 55.0f);
  const float in_octave = cents - 1200.0f * floorf(cents / 1200.0f);  // exact; [0, 1200]
  const float semis = cents / 100.0f;
  const float theta = 6.283185307179586f * (semis - rintf(semis));
  Peak q;
  q.m = mb;
  q.p = in_octave * 3.0f / 100.0f;
  q.c = mb * cosf(theta);
  q.s = mb * sinf(theta);
  return q;
}

// what the peak adds to column col
MX_CHROMA_HD float column_term(int col, const Peak &q) {
  if (col < kPcp) {
    float d = fabsf(q.p - (float)col);
    d = d > 18.0f ? 36.0f - d : d;
    const float w = 1.0f - 0.5f * d;
    return w > 0.f ? q.m * (0.5f * w) : 0.f;
  }
  return col == 36 ? q.c : col == 37 ? q.s : col == 38 ? q.m : 1.0f;
}

// bit j set: bin k0 + j is a peak; mv[j] = m[k0 - 1 + j], j < 18 (what lies outside the spectrum reads 0)
MX_CHROMA_HD uint32_t peak_mask(int k0, const float (&mv)[18], int kmin, int kmax, float thr) {
  uint32_t mask = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = k0 + j;
    const bool pk = k >= kmin && k <= kmax && mv[j + 1] > mv[j] && mv[j + 1] >= mv[j + 2] && mv[j + 1] >= thr;
    mask |= pk ? 1u << j : 0u;
  }
  return mask;
}

// the largest magnitude of the thread's band bins, as float bits (non-negative floats order as their bits, NaN above Inf)
MX_CHROMA_HD uint32_t band_max_bits(int k0, const float (&mv)[18], int kmin, int kmax) {
  uint32_t best = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = k0 + j;
    uint32_t b;
    __builtin_memcpy(&b, &mv[j + 1], 4);
    b &= 0x7fffffffu;
    best = (k >= kmin && k <= kmax && b > best) ? b : best;
  }
  return best;
}

MX_CHROMA_HD float threshold_of(float floor_abs, float rel, float band_max) {
  const float r = rel * band_max;
  return r > floor_abs ? r : floor_abs;
}

// a record's value in a window sum: widened, 0 where it is not finite
MX_CHROMA_HD double sum_term(float v) { return __builtin_isfinite(v) ? (double)v : 0.0; }

}  // namespace chroma

#if defined(__HIPCC__)
// Frame first_frame + f (f < count) is centred on sample (first_frame + f) * hop; out[f] its record.  2 <= kmin <= kmax <= 2046,
// floor_abs finite and >= 0, rel in [0, 1]: checked by the caller.
struct ChromaArgs {
  const float *audio;  // padded image (zeros in the pads)
  int hop;
  int64_t first_frame;
  int64_t count;
  int kmin, kmax;
  float floor_abs, rel;
  float bin_hz;                     // sr / 4096
  const float2 *tw2, *tw3, *ubase;  // Plan<4096,16> tables
  const float *hann;                // periodic Hann / 2048: the split leaves 2 X, so |.| comes out as |X| / 1024
  mx_chroma_rec *out;
  int frames_per_block;  // 0: the default.  The output does not depend on it
};
hipError_t launch_chroma(const ChromaArgs &a, hipStream_t s);
// out[40 j + c] = the sum of column c over records [first_frame, first_frame + frames) of job j, clipped to [0, count)
hipError_t launch_chroma_sum(const mx_chroma_rec *rec, int64_t count, const mx_chroma_job *jobs, int64_t njobs, double *out,
                             hipStream_t s);
#endif

}  // namespace mx
