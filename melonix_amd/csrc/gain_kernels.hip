// gain_kernels.hip — BUILD-DEFINED source gain (definition: include/melonix_amd.h "Sibilant detection, protection and
// balance"): out_i = (float)((double)x_i * g(i)), g piecewise linear in binary64 through {sample, amp} points, constant
// outside them.  No contraction, IEEE division: the bytes are numpy's (gain_core.h holds the arithmetic;
// tests/emu/sibilant_emu.cpp runs it on the CPU).
//
// One workgroup of 256 threads per tile of 2048 consecutive samples, a thread 4 consecutive samples (one 16-byte load and
// store: both images are 16-byte aligned) in each of two rounds.  Thread 0 finds the tile's first segment once — the number of
// points at or below the tile's first sample, a bisection — and leaves it in LDS; every thread walks forward from there, at
// most one step per point inside the tile, and keeps its segment in registers until a sample leaves it.  Memory-bound: 8 bytes per sample.
// The points are not validated here.  Out of order, they make the bisection and the walk end somewhere else — both are
// bounded by npts — and the samples wrong; equal samples divide by zero (Inf / NaN samples).  Stores go to [0, n) only.
#include <hip/hip_runtime.h>

#include "gain_core.h"
#include "kernels.h"

namespace mx {
namespace {

constexpr int kThreads = 256, kPerThread = 4, kRounds = 2, kTile = kThreads * kPerThread * kRounds;

__global__ __launch_bounds__(kThreads) void audio_gain_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n,
                                                              const mx_gain_point *__restrict__ pts, int64_t npts) {
  __shared__ int64_t first_seg;
  const int64_t tile0 = (int64_t)blockIdx.x * kTile;
  if (threadIdx.x == 0) {
    int64_t lo = 0, hi = npts;  // the first j in [0, npts] with pts[j].sample > tile0 (npts: none)
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)pts[mid].sample <= tile0) lo = mid + 1;
      else hi = mid;
    }
    first_seg = lo;
  }
  __syncthreads();
  int64_t j = first_seg;
  gain::Segment seg = gain::segment_at(pts, npts, j);
#pragma unroll
  for (int round = 0; round < kRounds; ++round) {
    const int64_t i0 = tile0 + (int64_t)round * (kThreads * kPerThread) + (int64_t)threadIdx.x * kPerThread;
    if (i0 >= n) break;
    float x[kPerThread], y[kPerThread];
    const bool whole = i0 + kPerThread <= n;
    if (whole) {
      const float4 v = *reinterpret_cast<const float4 *>(src + i0);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
#pragma unroll
      for (int e = 0; e < kPerThread; ++e) x[e] = i0 + e < n ? src[i0 + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
      const int64_t i = i0 + e;
      if (i >= seg.next) {  // (bounded by npts whatever the list holds)
        do ++j;
        while (j < npts && (int64_t)pts[j].sample <= i);
        seg = gain::segment_at(pts, npts, j);
      }
      y[e] = gain::gained(x[e], gain::gain_at(seg, i));
    }
    if (whole) {
      *reinterpret_cast<float4 *>(dst + i0) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int e = 0; e < kPerThread; ++e)
        if (i0 + e < n) dst[i0 + e] = y[e];
    }
  }
}

}  // namespace

hipError_t launch_audio_gain(const float *src, float *dst, int64_t n, const mx_gain_point *pts, int64_t npts, hipStream_t s) {
  if (n <= 0 || npts <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + kTile - 1) / kTile)), block(kThreads);
  hipLaunchKernelGGL(audio_gain_kernel, grid, block, 0, s, src, dst, n, pts, npts);
  return hipGetLastError();
}

}  // namespace mx
