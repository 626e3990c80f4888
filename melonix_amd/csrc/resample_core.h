// resample_core.h — the arithmetic of the sample-rate conversion (resample_kernels.hip; definition: include/melonix_amd.h
// "Sample-rate conversion"), plain C++ for the host, the device and tests/emu/resample_emu.cpp: the plan of a rate pair, the map
// from an output to its input sample and phase in 64-bit integers, the same map inside a tile in 32-bit ones, the input window and
// the size of a tile, and the dot product.  Built with -ffp-contract=off: every product is rounded before its sum.
#pragma once
#include <stdint.h>

#include "../../include/melonix_amd.h"
#include "step_core.h"

namespace mx {
namespace rs {

constexpr int kZeroCrossings = 32;  // Z: zero crossings of the prototype a side
constexpr int kMaxPhases = 1024;    // L at most
constexpr int kMaxTaps = 512;       // T at most
constexpr int kKaiserBeta = 12;

MX_STEP_HD int64_t gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The plan of in -> out; false: refused (a rate out of range, L > 1024, T > 512).  Equal rates: {1, 1, 0, 0}, a copy.
MX_STEP_HD bool plan_for(int in, int out, mx_resample_plan *p) {
  if (in < step::kMinRate || in > step::kMaxRate || out < step::kMinRate || out > step::kMaxRate) return false;
  const int64_t g = gcd(in, out), L = out / g, M = in / g;
  if (L == M) {
    *p = mx_resample_plan{1, 1, 0, 0};
    return true;
  }
  const int64_t big = L > M ? L : M, H = ((int64_t)kZeroCrossings * big + L - 1) / L;
  if (L > kMaxPhases || 2 * H > kMaxTaps) return false;
  *p = mx_resample_plan{(int32_t)L, (int32_t)M, (int32_t)(2 * H), (int32_t)H};
  return true;
}

// m = ceil(n L / M) outputs of n >= 0 samples
MX_STEP_HD int64_t out_length(int64_t n, const mx_resample_plan &p) { return (n * p.L + p.M - 1) / p.M; }

// output j >= 0 -> i_j = floor(j M / L), its input sample, and phi_j = (j M) mod L
struct At {
  int64_t i;
  int32_t phase;
};
MX_STEP_HD At at(int64_t j, const mx_resample_plan &p) {
  const int64_t t = j * (int64_t)p.M;
  return At{t / p.L, (int32_t)(t % p.L)};
}
// The same for output j0 + o from `base` = at(j0), o in [0, kMaxTile): phi + o M < 2^31, one 32-bit division.
constexpr int kMaxTile = 2048;
MX_STEP_HD At at_offset(const At &base, int o, const mx_resample_plan &p) {
  const uint32_t t = (uint32_t)base.phase + (uint32_t)o * (uint32_t)p.M;
  return At{base.i + (int64_t)(t / (uint32_t)p.L), (int32_t)(t % (uint32_t)p.L)};
}
static_assert((int64_t)kMaxPhases + (int64_t)kMaxTile * kMaxTaps * kMaxPhases / (2 * kZeroCrossings) < (1ll << 31),
              "phi + o M fits 32 bits (M <= L T / 2Z where M > L)");

// The input window of outputs [j0, j1], j0 <= j1: samples [first, last] = [i(j0) - (H - 1), i(j1) + H]
MX_STEP_HD int64_t window_first(int64_t j0, const mx_resample_plan &p) { return at(j0, p).i - (p.half - 1); }
MX_STEP_HD int64_t window_last(int64_t j1, const mx_resample_plan &p) { return at(j1, p).i + p.half; }

// How many consecutive outputs a workgroup of 256 threads takes so that the aligned quads that cover their window fit `floats`
// of LDS: a multiple of 256 in [256, kMaxTile].  The window of J outputs spans at most (J - 1) M / L + 1 + T samples, the
// alignment adds at most 6.  No output depends on it.
MX_STEP_HD int tile_outputs(const mx_resample_plan &p, int floats) {
  const int64_t fit = ((int64_t)(floats - p.taps - 8) * p.L) / p.M;
  const int64_t J = fit > kMaxTile ? kMaxTile : fit;
  return J < 256 ? 256 : (int)(J / 256) * 256;
}

// The launch's geometry (resample_kernels.hip; tests/emu/resample_emu.cpp walks the same tiles): the staged window takes 32 KiB
// of LDS at most; a table of at most 44 KiB is staged beside it, the two within 64 KiB.
constexpr int kWindowFloats = 32768 / 4, kLdsBytes = 65536, kTableLdsBytes = 44 * 1024;
struct Geometry {
  int tile;       // outputs per workgroup
  int win_quads;  // the 16-byte quads that cover a tile's window: ((tile - 1) M / L + 1 + T samples and the alignment) / 4
  bool lds_table;
};
MX_STEP_HD Geometry geometry(const mx_resample_plan &p) {
  const int table_bytes = p.L * p.taps * (int)sizeof(float);
  Geometry g;
  g.lds_table = table_bytes <= kTableLdsBytes;
  const int room = g.lds_table ? (kLdsBytes - table_bytes) / 16 * 4 : kWindowFloats;  // floats the window may take
  g.tile = tile_outputs(p, room < kWindowFloats ? room : kWindowFloats);
  g.win_quads = (int)(((int64_t)(g.tile - 1) * p.M / p.L + p.taps + 8 + 3) / 4);
  return g;
}
// a tile of 256 outputs fits the smallest window: (256 - 1) M / L + T + 8 with M / L <= T / 2Z
static_assert(255 * (kMaxTaps / (2 * kZeroCrossings)) + kMaxTaps + 8 <= (kLdsBytes - kTableLdsBytes) / 4, "smallest tile");

// y_r = sum over k ascending of x[xo_r + k] * h[ho_r + k * hstride], from +0.f, each product rounded, then added: R outputs side
// by side (independent sums: the order inside each is the definition's).
template <int R>
MX_STEP_HD void dots(const float *x, const int (&xo)[R], const float *h, const int (&ho)[R], int hstride, int taps, float (&y)[R]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < R; ++r) y[r] = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 2
#endif
  for (int k = 0; k < taps; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < R; ++r) y[r] = y[r] + x[xo[r] + k] * h[ho[r] + k * hstride];
  }
}

}  // namespace rs
}  // namespace mx
