// sibilant_kernels.hip — BUILD-DEFINED sibilant features (the reference has none; definition: include/melonix_amd.h
// "Sibilant detection, protection and balance", restated in f64 by tests/sibilant_ref.py):
//   frame h: x_j = audio[h*hop - 512 + j], j < 1024 (zeros outside the file: the mx_audio pad), periodic Hann, X = DFT_1024,
//   P_k = (|X_k| / 512)^2, low = sum_{k < ks} P_k, high = sum_{k >= ks} P_k (k = 1..511), centroid = sum k P_k / (low + high),
//   zero_crossings = sign changes between neighbouring raw samples of the frame.
//
// The onset-strength kernel's walk (onset_walk.h, shared with onset_kernels.hip) with another head and tail: one wavefront (a workgroup of 64 threads) takes a
// run of consecutive frames through onset_core.h's 8 x 8 x 8 transform — 16 samples per lane, two transpositions and the
// split through the 4.5 KiB LDS image — and ends a frame with the powers of bins lane + 64 r, r < 8, in registers.  No row is
// kept from frame to frame, so a run has no head frames.  The three sums take the flux's order — the lane's 8 bins in
// ascending r, then six cross-lane exchange steps (32, 16, .., 1) —; the zero-crossing count is integer: sign bits of the
// lane's 16 raw samples as two 8-bit masks, one exchange with the next lane for the boundaries between lanes, a wave sum.
// A record depends on its frame's samples alone: the same bytes whatever the launch split or the run length.  No scratch, no
// atomics; 16 bytes per frame, stored by lane 0.
#include <hip/hip_runtime.h>

#include "onset_walk.h"
#include "sibilant_core.h"

namespace mx {
namespace {

using namespace sib;

__global__ __launch_bounds__(kLanes) void sib_features_kernel(const SibArgs a) {
  __shared__ __attribute__((aligned(16))) float2 img[kImage];
  const int lane = threadIdx.x;
  const Run run(a, lane);
  if (run.h0 >= run.h1) return;
  LaneConsts lc;
  lane_consts(lane, a.tw, lc);
  const int64_t h1 = run.h1;
  float2 x[8];
  run.load(run.h0, x);
  for (int64_t h = run.h0; h < h1; ++h) {
    uint32_t first, second;
    sign_masks(x, first, second);  // (of the raw samples, before the next frame's take their registers)
    const int zc = lane_crossings(lane, first, second, (uint32_t)__shfl((int)first, (lane + 1) & (kLanes - 1), 64));
    float2 v[8];
    transform(lane, lc, x, img, v, [&] {
      if (h + 1 < h1) run.load(h + 1, x);
    });
    float P[8];
    powers(lane, lc, v, img, P);
    __syncthreads();  // the image is read: the next frame may write it
    const LaneSums s = lane_sums(lane, P, a.ks);
    mx_sib_feat rec;
    rec.low = wave_sum(s.low);
    rec.high = wave_sum(s.high);
    rec.centroid = centroid_of(rec.low, rec.high, wave_sum(s.moment));
    rec.zero_crossings = wave_sum(zc);
    if (lane == 0) a.out[h - a.first_frame] = rec;
  }
}

}  // namespace

hipError_t launch_sib_features(const SibArgs &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  SibArgs a = a0;
  const dim3 grid = walk_grid(a.count, a.run, onset_default_run(a.count)), block(kLanes);
  hipLaunchKernelGGL(sib_features_kernel, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace mx
