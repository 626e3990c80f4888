// contour_kernels.hip — BUILD-DEFINED pitch-contour split (the reference has no such operation; definition:
// include/melonix_amd.h "Pitch drift and vibrato inside notes", restated by tests/contour_ref.py).  The arithmetic is
// contour_core.h's; after stage A it is all integers, so no order of any sum below matters.
//
// contour_cents_kernel: a thread per frame, the record alone.
// contour_split_kernel: a workgroup of 256 threads per tile of 256 frames.  The values of the tile and 2w frames either side go
// to an LDS row, the first box pass over the tile and w frames either side to a second row, the second pass reads that: the
// intermediate never leaves the workgroup.  Each thread finds the span of the frame it works on by a binary search over the
// sorted spans and clips its window to it, so a window never crosses a span boundary and the halo of a tile is recomputed
// by both neighbours to the same integers.
// contour_partial_kernel: a workgroup per tile of 1024 frames walks the pieces of spans that lie in it.  A piece's vib values
// (and lag_max more of its span behind them) go to LDS; the threads add up the piece's sums, six shuffle steps per wave and
// four values through LDS; then wave v takes lags lag_min + v, + 4, ..: 64 lanes over the frames, six shuffle steps, lane 0
// stores.  A piece writes slot tile + span of the work memory and nothing else.
// contour_final_kernel: a workgroup per span adds its pieces up, thread i the autocorrelation at lag_min + i, and takes the
// best lag by a total order (greatest sum, lowest lag), so any reduction tree gives the same pair.
// No atomics, nothing between workgroups beyond the launch order, no scratch.  Every span is clipped to the array and every
// index into its row: bad spans give wrong values and nothing worse.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "contour_core.h"

namespace mx {
namespace {

using namespace contour;

__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int step) {
  const int lo = __shfl_xor((int)(uint32_t)(uint64_t)v, step, 64), hi = __shfl_xor((int)(v >> 32), step, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

__device__ __forceinline__ Partial wave_partial(Partial a) {
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    Partial b;
    b.sum_smooth = shfl_xor64(a.sum_smooth, step);
    b.r0 = shfl_xor64(a.r0, step);
    b.min_smooth = __shfl_xor(a.min_smooth, step, 64);
    b.max_smooth = __shfl_xor(a.max_smooth, step, 64);
    partial_add(a, b);
  }
  return a;
}

__global__ __launch_bounds__(kThreads) void contour_cents_kernel(const mx_f0 *__restrict__ track, int64_t count, int sampleRate,
                                                                  float threshold, float rms_floor, int32_t *__restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (f < count) out[f] = cents_of(track[f], sampleRate, threshold, rms_floor);
}

__global__ __launch_bounds__(kThreads) void contour_split_kernel(const int32_t *__restrict__ cents, int64_t count,
                                                                  const mx_contour_span *__restrict__ spans, int64_t nspans, int w,
                                                                  mx_contour_rec *__restrict__ rec) {
  __shared__ int32_t c_row[kCentsRow];
  __shared__ int32_t b_row[kBoxRow];
  const int t = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kTile, c0 = t0 - 2 * w, b0 = t0 - w;
  for (int i = t; i < kTile + 4 * w; i += kThreads) {
    const int64_t g = c0 + i;
    c_row[i] = g >= 0 && g < count ? cents[g] : MX_CONTOUR_NONE;
  }
  __syncthreads();  // the values are there
  for (int i = t; i < kTile + 2 * w; i += kThreads) {
    const int64_t g = b0 + i;
    int64_t lo, hi;
    b_row[i] = span_of(spans, nspans, count, g, lo, hi) >= 0 ? box_mean(c_row, c0, lo, hi, g, w) : 0;
  }
  __syncthreads();  // the first pass is there
  const int64_t f = t0 + t;
  if (f >= count) return;
  int64_t lo, hi;
  mx_contour_rec r{MX_CONTOUR_NONE, 0};
  if (span_of(spans, nspans, count, f, lo, hi) >= 0) {
    r.smooth = box_mean(b_row, b0, lo, hi, f, w);
    r.vib = (int32_t)((int64_t)c_row[t + 2 * w] - (int64_t)r.smooth);
  }
  rec[f] = r;
}

__global__ __launch_bounds__(kThreads) void contour_partial_kernel(const mx_contour_rec *__restrict__ rec, int64_t count,
                                                                    const mx_contour_span *__restrict__ spans, int64_t nspans,
                                                                    const mx_contour_params p, Partial *__restrict__ part,
                                                                    int64_t *__restrict__ part_r) {
  __shared__ int32_t vib[kVibRow];
  __shared__ Partial wave_part[kThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t tile = blockIdx.x, t0 = tile * kStatTile, t1 = t0 + kStatTile < count ? t0 + kStatTile : count;
  const int nl = p.lag_max - p.lag_min + 1;
  for (int64_t s = first_span_beyond(spans, nspans, t0); s < nspans && (int64_t)spans[s].first < t1; ++s) {
    int64_t lo, hi;
    span_frames(spans[s], count, lo, hi);
    const int64_t plo = lo > t0 ? lo : t0, phi = hi < t1 ? hi : t1;
    if (plo >= phi) continue;  // (the same for every thread)
    const int n = (int)((phi + p.lag_max < hi ? phi + p.lag_max : hi) - plo);  // <= kVibRow
    const int np = (int)(phi - plo);
    Partial a = partial_none();
    for (int i = t; i < n; i += kThreads) {
      const mx_contour_rec r = rec[plo + i];
      vib[i] = r.vib;
      if (i < np) partial_take(a, r);
    }
    a = wave_partial(a);
    if (lane == 0) wave_part[wave] = a;
    __syncthreads();  // the row and the four partial sums are written
    const int64_t slot = slot_of(tile, s);
    if (t == 0) {
      for (int v = 1; v < kThreads / 64; ++v) partial_add(a, wave_part[v]);
      part[slot] = a;
    }
    const int top = top_lag(p, hi - lo);
    for (int L = p.lag_min + wave; L <= top; L += kThreads / 64) {
      const int64_t room = hi - L - plo;  // frames of the piece whose partner lies in the span
      const int m = room < (int64_t)np ? (int)room : np;
      int64_t acc = 0;
      for (int i = lane; i < m; i += 64) acc += (int64_t)vib[i] * (int64_t)vib[i + L];
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) acc += shfl_xor64(acc, step);
      if (lane == 0) part_r[slot * nl + (L - p.lag_min)] = acc;
    }
    __syncthreads();  // the row is free for the next piece
  }
}

__global__ __launch_bounds__(kThreads) void contour_final_kernel(const mx_contour_span *__restrict__ spans, int64_t count,
                                                                  const mx_contour_params p, const Partial *__restrict__ part,
                                                                  const int64_t *__restrict__ part_r,
                                                                  mx_contour_stat *__restrict__ stat) {
  __shared__ Partial wave_part[kThreads / 64];
  __shared__ int64_t wave_r[kThreads / 64];
  __shared__ int32_t wave_lag[kThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t s = blockIdx.x;
  const int nl = p.lag_max - p.lag_min + 1;
  int64_t lo, hi;
  span_frames(spans[s], count, lo, hi);
  const int64_t F = hi - lo;
  Partial a = partial_none();
  int64_t r = 0;
  int32_t lag = 0;
  if (F > 0) {
    const int64_t tlo = lo / kStatTile, thi = (hi - 1) / kStatTile;
    for (int64_t tile = tlo + t; tile <= thi; tile += kThreads) partial_add(a, part[slot_of(tile, s)]);
    if (p.lag_min + t <= top_lag(p, F)) {
      lag = p.lag_min + t;
      for (int64_t tile = tlo; tile <= thi; ++tile) r += part_r[slot_of(tile, s) * nl + t];
    }
  }
  a = wave_partial(a);
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    const int64_t rb = shfl_xor64(r, step);
    const int32_t lb = __shfl_xor(lag, step, 64);
    if (lag_better(rb, lb, r, lag)) {
      r = rb;
      lag = lb;
    }
  }
  if (lane == 0) {
    wave_part[wave] = a;
    wave_r[wave] = r;
    wave_lag[wave] = lag;
  }
  __syncthreads();  // the four partial sums and pairs are written
  if (t == 0) {
    for (int v = 1; v < kThreads / 64; ++v) {
      partial_add(a, wave_part[v]);
      if (lag_better(wave_r[v], wave_lag[v], r, lag)) {
        r = wave_r[v];
        lag = wave_lag[v];
      }
    }
    stat[s] = stat_of(a, F, lag, r);
  }
}

int64_t stat_tiles(int64_t count) { return (count + kStatTile - 1) / kStatTile; }

}  // namespace

hipError_t launch_contour_cents(const mx_f0 *d_track, int64_t count, int sampleRate, float threshold, float rms_floor,
                                int32_t *d_cents, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  if (count > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((count + kThreads - 1) / kThreads)), block(kThreads);
  hipLaunchKernelGGL(contour_cents_kernel, grid, block, 0, s, d_track, count, sampleRate, threshold, rms_floor, d_cents);
  return hipGetLastError();
}

size_t contour_part_bytes(int64_t count, int64_t nspans, const mx_contour_params &p0) {
  const mx_contour_params p = params_clamped(p0);
  const size_t slots = (size_t)(stat_tiles(count) + nspans), nl = (size_t)(p.lag_max - p.lag_min + 1);
  return slots * (sizeof(Partial) + nl * sizeof(int64_t));
}

hipError_t launch_contour_split(const int32_t *d_cents, int64_t count, const mx_contour_span *d_spans, int64_t nspans,
                                const mx_contour_params &p0, mx_contour_rec *d_rec, mx_contour_stat *d_stat, void *d_part,
                                hipStream_t s) {
  if (count <= 0 || nspans < 0) return hipSuccess;
  if (count > INT32_MAX || nspans > count) return hipErrorInvalidValue;
  const mx_contour_params p = params_clamped(p0);
  const dim3 block(kThreads);
  hipLaunchKernelGGL(contour_split_kernel, dim3((unsigned)((count + kTile - 1) / kTile)), block, 0, s, d_cents, count, d_spans,
                     nspans, p.half_width, d_rec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !d_stat || nspans == 0) return e;
  const int64_t tiles = stat_tiles(count);
  Partial *part = static_cast<Partial *>(d_part);
  int64_t *part_r = reinterpret_cast<int64_t *>(part + (tiles + nspans));
  hipLaunchKernelGGL(contour_partial_kernel, dim3((unsigned)tiles), block, 0, s, d_rec, count, d_spans, nspans, p, part, part_r);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(contour_final_kernel, dim3((unsigned)nspans), block, 0, s, d_spans, count, p, part, part_r, d_stat);
  return hipGetLastError();
}

}  // namespace mx
