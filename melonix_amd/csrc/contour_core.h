// contour_core.h — the arithmetic of the pitch-contour kernels (contour_kernels.hip; definition: include/melonix_amd.h "Pitch
// drift and vibrato inside notes") as plain host/device C++: one frame's cents, the span a frame lies in, one clipped box mean,
// one piece's partial sums, the order of two lags.  tests/emu/contour_emu.cpp runs the same functions on the CPU.  Stage A is
// binary64 (compile with -ffp-contract=off); everything after it is integer arithmetic, exact whatever the order.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/melonix_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_CONTOUR_HD __host__ __device__ __forceinline__
#else
#define MX_CONTOUR_HD inline
#endif

namespace mx {
namespace contour {

constexpr int kThreads = 256;     // of every workgroup here
constexpr int kTile = 256;        // frames of a smoothing workgroup: a thread per frame
constexpr int kMaxWidth = 64;     // w
constexpr int kMaxLag = 256;      // lag_max
constexpr int kStatTile = 1024;   // frames of a statistics workgroup
// LDS rows of the smoothing kernel: the values of frames [t0 - 2w, t0 + kTile + 2w) and the first pass over [t0 - w, t0 + kTile + w)
constexpr int kCentsRow = kTile + 4 * kMaxWidth, kBoxRow = kTile + 2 * kMaxWidth;
// ... and of the partial kernel: a piece's vib values and kMaxLag more of its span behind them
constexpr int kVibRow = kStatTile + kMaxLag;

// a piece's sums (one piece: the frames of one span inside one statistics tile), and what the last kernel adds up per span
struct Partial {
  int64_t sum_smooth, r0;
  int32_t min_smooth, max_smooth;
};

MX_CONTOUR_HD bool params_ok(const mx_contour_params &p) {
  return p.half_width >= 0 && p.half_width <= kMaxWidth && p.lag_min >= 1 && p.lag_min <= p.lag_max && p.lag_max <= kMaxLag;
}

// the parameters as the kernels use them: each clamped into its range (the entry points refuse what the clamp would change)
MX_CONTOUR_HD mx_contour_params params_clamped(mx_contour_params p) {
  p.half_width = p.half_width < 0 ? 0 : p.half_width > kMaxWidth ? kMaxWidth : p.half_width;
  p.lag_min = p.lag_min < 1 ? 1 : p.lag_min > kMaxLag ? kMaxLag : p.lag_min;
  p.lag_max = p.lag_max < p.lag_min ? p.lag_min : p.lag_max > kMaxLag ? kMaxLag : p.lag_max;
  return p;
}

// stage A: one record's value
MX_CONTOUR_HD int32_t cents_of(const mx_f0 &r, int sampleRate, float threshold, float rms_floor) {
  uint32_t u;
  memcpy(&u, &r.period, 4);
  const bool finite = (u & 0x7f800000u) != 0x7f800000u;
  if (!(r.tau > 0 && r.aperiodicity < threshold && r.rms >= rms_floor && finite && r.period > 0.f)) return MX_CONTOUR_NONE;
  const double note = log2((double)sampleRate / (double)r.period / 55.0);
  return (int32_t)rint(16.0 * (1200.0 * note + 2400.0));
}

// floor(a / b), b > 0
MX_CONTOUR_HD int64_t floor_div(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// span s clipped to the array: frames [lo, hi), 0 <= lo <= hi <= count
MX_CONTOUR_HD void span_frames(const mx_contour_span &s, int64_t count, int64_t &lo, int64_t &hi) {
  lo = s.first < 0 ? 0 : (int64_t)s.first > count ? count : (int64_t)s.first;
  hi = (int64_t)s.first + (int64_t)s.frames;
  hi = hi < lo ? lo : hi > count ? count : hi;
}

// the span frame g lies in: the last span that starts at or before g (a binary search: the spans are sorted), if it reaches g.
// -> its index and [lo, hi), or -1
MX_CONTOUR_HD int64_t span_of(const mx_contour_span *spans, int64_t nspans, int64_t count, int64_t g, int64_t &lo, int64_t &hi) {
  int64_t a = 0, b = nspans;  // the first span with first > g
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if ((int64_t)spans[m].first <= g) a = m + 1;
    else b = m;
  }
  if (a == 0) return -1;
  span_frames(spans[a - 1], count, lo, hi);
  return g >= lo && g < hi ? a - 1 : -1;
}

// the first span that ends behind frame t (first + frames > t); nspans: none
MX_CONTOUR_HD int64_t first_span_beyond(const mx_contour_span *spans, int64_t nspans, int64_t t) {
  int64_t a = 0, b = nspans;
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if ((int64_t)spans[m].first + (int64_t)spans[m].frames <= t) a = m + 1;
    else b = m;
  }
  return a;
}

// mean(v, f) over the window clipped to [lo, hi): row[i] holds v of frame base + i, and the caller has every frame of the
// window in the row
MX_CONTOUR_HD int32_t box_mean(const int32_t *row, int64_t base, int64_t lo, int64_t hi, int64_t f, int w) {
  const int64_t g0 = f - w < lo ? lo : f - w, g1 = f + w > hi - 1 ? hi - 1 : f + w;
  int64_t S = 0;
  for (int64_t g = g0; g <= g1; ++g) S += (int64_t)row[g - base];
  const int64_t c = g1 - g0 + 1;
  return (int32_t)floor_div(2 * S + c, 2 * c);
}

MX_CONTOUR_HD Partial partial_none() { return Partial{0, 0, INT32_MAX, INT32_MIN}; }
MX_CONTOUR_HD void partial_add(Partial &a, const Partial &b) {
  a.sum_smooth += b.sum_smooth;
  a.r0 += b.r0;
  a.min_smooth = b.min_smooth < a.min_smooth ? b.min_smooth : a.min_smooth;
  a.max_smooth = b.max_smooth > a.max_smooth ? b.max_smooth : a.max_smooth;
}
MX_CONTOUR_HD void partial_take(Partial &a, const mx_contour_rec &r) {
  partial_add(a, Partial{(int64_t)r.smooth, (int64_t)r.vib * (int64_t)r.vib, r.smooth, r.smooth});
}

// which of two (r, lag) pairs the statistics take: the greater r, the lower lag among equals; lag 0 is "none" and loses
MX_CONTOUR_HD bool lag_better(int64_t ra, int32_t la, int64_t rb, int32_t lb) {
  if (la == 0) return false;
  if (lb == 0) return true;
  return ra > rb || (ra == rb && la < lb);
}

// the piece of span s inside tile t lands in slot t + s: along the sorted spans the (t, s) pairs of all pieces form a
// staircase, on which t + s never repeats; there are ntiles + nspans slots
MX_CONTOUR_HD int64_t slot_of(int64_t tile, int64_t span) { return tile + span; }

// the highest lag of a span of F frames: min(lag_max, F - 1); below lag_min: none
MX_CONTOUR_HD int top_lag(const mx_contour_params &p, int64_t F) { return (int64_t)p.lag_max < F - 1 ? p.lag_max : (int)(F - 1); }

MX_CONTOUR_HD mx_contour_stat stat_of(const Partial &a, int64_t F, int32_t lag, int64_t r_lag) {
  mx_contour_stat s;
  s.sum_smooth = a.sum_smooth;
  s.min_smooth = F > 0 ? a.min_smooth : 0;
  s.max_smooth = F > 0 ? a.max_smooth : 0;
  s.r0 = a.r0;
  s.lag = lag;
  s.reserved = 0;
  s.r_lag = lag ? r_lag : 0;
  return s;
}

}  // namespace contour

#if defined(__HIPCC__)
// Stage A: a thread per frame.  count <= INT32_MAX.
hipError_t launch_contour_cents(const mx_f0 *d_track, int64_t count, int sampleRate, float threshold, float rms_floor,
                                int32_t *d_cents, hipStream_t s);
// Stage B.  d_rec: count records.  d_stat null: the smoothing launch alone; otherwise d_part (contour_part_bytes) takes the
// pieces' partial sums between the two statistics launches.  The parameters are clamped into range, the spans clipped.
size_t contour_part_bytes(int64_t count, int64_t nspans, const mx_contour_params &p);
hipError_t launch_contour_split(const int32_t *d_cents, int64_t count, const mx_contour_span *d_spans, int64_t nspans,
                                const mx_contour_params &p, mx_contour_rec *d_rec, mx_contour_stat *d_stat, void *d_part,
                                hipStream_t s);
#endif

}  // namespace mx
