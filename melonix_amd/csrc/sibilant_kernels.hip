// sibilant_kernels.hip — BUILD-DEFINED sibilant features (the reference has none; definition: include/melonix_amd.h
// "Sibilant detection, protection and balance", restated in f64 by tests/sibilant_ref.py):
//   frame h: x_j = audio[h*hop - 512 + j], j < 1024 (zeros outside the file: the mx_audio pad), periodic Hann, X = DFT_1024,
//   P_k = (|X_k| / 512)^2, low = sum_{k < ks} P_k, high = sum_{k >= ks} P_k (k = 1..511), centroid = sum k P_k / (low + high),
//   zero_crossings = sign changes between neighbouring raw samples of the frame.
//
// The onset-strength kernel's walk (onset_kernels.hip) with another tail: one wavefront (a workgroup of 64 threads) takes a
// run of consecutive frames through onset_core.h's 8 x 8 x 8 transform — 16 samples per lane, two transpositions and the
// split through the 4.5 KiB LDS image — and ends a frame with the powers of bins lane + 64 r, r < 8, in registers.  No row is
// kept from frame to frame, so a run has no head frames.  The three sums take the flux's order — the lane's 8 bins in
// ascending r, then six cross-lane exchange steps (32, 16, .., 1) —; the zero-crossing count is integer: sign bits of the
// lane's 16 raw samples as two 8-bit masks, one exchange with the next lane for the boundaries between lanes, a wave sum.
// A record depends on its frame's samples alone: the same bytes whatever the launch split or the run length.  No scratch, no
// atomics; 16 bytes per frame, stored by lane 0.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sibilant_core.h"

namespace mx {
namespace {

using namespace sib;

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

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) v = v + __shfl_xor(v, step, 64);
  return v;
}

__global__ __launch_bounds__(kLanes) void sib_features_kernel(const SibArgs a) {
  __shared__ __attribute__((aligned(16))) float2 img[kImage];
  const int lane = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * a.run;
  const int64_t f1 = f0 + a.run < a.count ? f0 + a.run : a.count;
  if (f0 >= f1) return;
  LaneConsts lc;
  lane_consts(lane, a.tw, lc);
  const int64_t h0 = a.first_frame + f0, h1 = a.first_frame + f1;
  const float *const p = a.audio + MX_AUDIO_PAD - kM + 2 * lane;
  const bool aligned = (reinterpret_cast<uintptr_t>(a.audio) & 7) == 0;
  float2 x[8];
  load_frame(p, h0 * a.hop, aligned && ((h0 * a.hop) & 1) == 0, x);
  for (int64_t h = h0; h < h1; ++h) {
    uint32_t first, second;
    sign_masks(x, first, second);  // (of the raw samples, before the next frame's take their registers)
    const int zc = lane_crossings(lane, first, second, (uint32_t)__shfl((int)first, (lane + 1) & (kLanes - 1), 64));
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
  if (a.run <= 0) a.run = onset_default_run(a.count);
  while ((a.count + a.run - 1) / a.run > (1ll << 30)) a.run *= 2;  // (the grid's x extent)
  const dim3 grid((unsigned)((a.count + a.run - 1) / a.run)), block(kLanes);
  hipLaunchKernelGGL(sib_features_kernel, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace mx
