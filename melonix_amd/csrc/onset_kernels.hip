// onset_kernels.hip — BUILD-DEFINED onset strength (the reference has no detector; definition: include/melonix_amd.h "Onset
// detection", restated in f64 by tests/onset_ref.py):
//   frame h: x_j = audio[h*hop - 512 + j], j < 1024 (zeros outside the file: the mx_audio pad), periodic Hann, X = DFT_1024,
//   c_h[k] = log1pf(compress * |X_k| / 512), flux_h = sum_{k = kmin..kmax} max(0, c_h[k] - c_{h-lag}[k]), c_h = 0 for h < 0.
//
// One wavefront (a workgroup of 64 threads) walks a run of consecutive frames (onset_walk.h: the loads, the run, the frame's
// schedule; this kernel's own are the lag rows in front and the flux behind).  The transform is onset_core.h's: a real 1024
// through a complex 512 = 8 x 8 x 8, 16 samples per lane, two transpositions and the split through a 4.5 KiB LDS image.
// A lane ends a frame with the compressed magnitudes of bins lane + 64 r, r < 8, in registers, and keeps the last `lag` such
// rows there (LAG x 8 VGPRs): no spectrum goes to LDS beyond the image, none to HBM.  At the head of its run the walker first
// computes frames h0-lag .. h0-1 (those >= 0) without storing anything; then 4 bytes per frame.
// The reduction has one fixed order — the lane's 8 bins in ascending r, then six cross-lane exchange steps (32, 16, .., 1) —
// so frame h's value depends on nothing but its samples and frame h-lag's: the same bytes whatever the launch split or the
// run length.  No scratch, no atomics.
#include <hip/hip_runtime.h>

#include "onset_walk.h"

namespace mx {
namespace {

using namespace onset;

template <int LAG>
__global__ __launch_bounds__(kLanes) void onset_flux_kernel(const OnsetArgs a) {
  __shared__ __attribute__((aligned(16))) float2 img[kImage];
  const int lane = threadIdx.x;
  const Run run(a, lane);
  if (run.h0 >= run.h1) return;
  LaneConsts lc;
  lane_consts(lane, a.tw, lc);
  float prev[LAG][8];  // prev[i]: the compressed row of frame h - 1 - i
#pragma unroll
  for (int i = 0; i < LAG; ++i)
#pragma unroll
    for (int r = 0; r < 8; ++r) prev[i][r] = 0.f;
  const int64_t h0 = run.h0, h1 = run.h1;
  const int64_t hs = h0 - LAG > 0 ? h0 - LAG : 0;  // (frames before the file are rows of zeros: what prev starts as)
  float2 x[8];
  run.load(hs, x);
  for (int64_t h = hs; h < h1; ++h) {
    float2 v[8];
    transform(lane, lc, x, img, v, [&] {
      if (h + 1 < h1) run.load(h + 1, x);
    });
    float cur[8];
    compressed(lane, lc, v, img, a.compress, cur);
    __syncthreads();  // the image is read: the next frame may write it
    if (h >= h0) {
      const float s = wave_sum(lane_flux(lane, cur, prev[LAG - 1], a.kmin, a.kmax));
      if (lane == 0) a.flux[h - a.first_frame] = s;
    }
#pragma unroll
    for (int i = LAG - 1; i > 0; --i)
#pragma unroll
      for (int r = 0; r < 8; ++r) prev[i][r] = prev[i - 1][r];
#pragma unroll
    for (int r = 0; r < 8; ++r) prev[0][r] = cur[r];
  }
}

}  // namespace

hipError_t launch_onset_flux(const OnsetArgs &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  OnsetArgs a = a0;
  const dim3 grid = walk_grid(a.count, a.run, onset_default_run(a.count)), block(kLanes);
  switch (a.lag) {
    case 1: hipLaunchKernelGGL(onset_flux_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(onset_flux_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(onset_flux_kernel<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(onset_flux_kernel<4>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mx
