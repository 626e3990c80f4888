// onset_kernels.hip — BUILD-DEFINED onset strength (the reference has no detector; definition: include/melonix_amd.h "Onset
// detection", restated in f64 by tests/onset_ref.py):
//   frame h: x_j = audio[h*hop - 512 + j], j < 1024 (zeros outside the file: the mx_audio pad), periodic Hann, X = DFT_1024,
//   c_h[k] = log1pf(compress * |X_k| / 512), flux_h = sum_{k = kmin..kmax} max(0, c_h[k] - c_{h-lag}[k]), c_h = 0 for h < 0.
//
// One wavefront (a workgroup of 64 threads) walks a run of consecutive frames.  The transform is onset_core.h's: a real 1024
// through a complex 512 = 8 x 8 x 8, 16 samples per lane, two transpositions and the split through a 4.5 KiB LDS image.
// A lane ends a frame with the compressed magnitudes of bins lane + 64 r, r < 8, in registers, and keeps the last `lag` such
// rows there (LAG x 8 VGPRs): no spectrum goes to LDS beyond the image, none to HBM.  At the head of its run the walker first
// computes frames h0-lag .. h0-1 (those >= 0) without storing anything; then 4 bytes per frame.
// The reduction has one fixed order — the lane's 8 bins in ascending r, then six cross-lane exchange steps (32, 16, .., 1) —
// so frame h's value depends on nothing but its samples and frame h-lag's: the same bytes whatever the launch split or the
// run length.  No scratch, no atomics.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "onset_core.h"

namespace mx {
namespace {

using namespace onset;

// the lane's 8 sample pairs of the frame centred on sample `centre`: p = the padded image + MX_AUDIO_PAD - 512 + 2 lane
__device__ __forceinline__ void load_frame(const float *p, int64_t centre, bool pairs, float2 (&x)[8]) {
  const float *q = p + centre;
  if (pairs) {  // wave-uniform: the frame starts on an even sample of an 8-byte aligned image
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = *reinterpret_cast<const float2 *>(q + 128 * r);
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = c_mk(q[128 * r], q[128 * r + 1]);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) v = v + __shfl_xor(v, step, 64);
  return v;
}

template <int LAG>
__global__ __launch_bounds__(kLanes) void onset_flux_kernel(const OnsetArgs a) {
  __shared__ __attribute__((aligned(16))) float2 img[kImage];
  const int lane = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * a.run;
  const int64_t f1 = f0 + a.run < a.count ? f0 + a.run : a.count;
  if (f0 >= f1) return;
  LaneConsts lc;
  lane_consts(lane, a.tw, lc);
  float prev[LAG][8];  // prev[i]: the compressed row of frame h - 1 - i
#pragma unroll
  for (int i = 0; i < LAG; ++i)
#pragma unroll
    for (int r = 0; r < 8; ++r) prev[i][r] = 0.f;
  const int64_t h0 = a.first_frame + f0, h1 = a.first_frame + f1;
  const int64_t hs = h0 - LAG > 0 ? h0 - LAG : 0;  // (frames before the file are rows of zeros: what prev starts as)
  const float *const p = a.audio + MX_AUDIO_PAD - kM + 2 * lane;
  const bool aligned = (reinterpret_cast<uintptr_t>(a.audio) & 7) == 0;
  float2 x[8];
  load_frame(p, hs * a.hop, aligned && ((hs * a.hop) & 1) == 0, x);
  for (int64_t h = hs; h < h1; ++h) {
    pass1(lane, lc, x, img);
    if (h + 1 < h1) load_frame(p, (h + 1) * a.hop, aligned && (((h + 1) * a.hop) & 1) == 0, x);  // travels under this frame
    __syncthreads();
    float2 v[8];
    pass2(lane, lc, img, v);
    __syncthreads();
    store2(lane, v, img);
    __syncthreads();
    pass3(lane, img, v);
    __syncthreads();
    store3(lane, v, img);
    __syncthreads();
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

int onset_default_run(int64_t count) {
  // a run pays `lag` frames at its head: long runs where there are frames enough to fill the device with them
  const int64_t want = count / 4096;
  return (int)(want < 1 ? 1 : want > 32 ? 32 : want);
}

hipError_t launch_onset_flux(const OnsetArgs &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  OnsetArgs a = a0;
  if (a.run <= 0) a.run = onset_default_run(a.count);
  while ((a.count + a.run - 1) / a.run > (1ll << 30)) a.run *= 2;  // (the grid's x extent)
  const dim3 grid((unsigned)((a.count + a.run - 1) / a.run)), block(kLanes);
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
