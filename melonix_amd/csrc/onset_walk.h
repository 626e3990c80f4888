// onset_walk.h — what the two kernels share that walk a run of consecutive frames through onset_core.h's 1024-point transform on
// ONE wavefront: onset_flux_kernel (onset_kernels.hip) and sib_features_kernel (sibilant_kernels.hip).  The device side of
// onset_core.h, which stays free of intrinsics (tests/emu runs it on the CPU): the sample loads, the wavefront's sum, the run of
// a block and the frame's schedule of passes and barriers.  Pieces, not a kernel: what a walker does before the transform (its
// head) and behind it (its tail) stays its own.  Private to those two units.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "onset_core.h"

namespace mx {
namespace onset {

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

// The wavefront's sum (float or int): six exchange steps, lane l adding lane l ^ step's value, step = 32, 16, .., 1 — the order
// onset_core.h's wave_sum_host takes.  Every lane ends with the same bits.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) v = v + __shfl_xor(v, step, 64);
  return v;
}

// The frames of the file a block walks, [h0, h1) (empty: the block has none), and where a lane finds their samples.  Args:
// OnsetArgs or SibArgs — audio, hop, first_frame, count, run.
struct Run {
  int64_t h0, h1;
  const float *p;  // the lane's base pointer (load_frame)
  bool aligned;    // the image is 8-byte aligned
  int hop;
  template <class Args>
  __device__ __forceinline__ Run(const Args &a, int lane) {
    const int64_t f0 = (int64_t)blockIdx.x * a.run;
    const int64_t f1 = f0 + a.run < a.count ? f0 + a.run : a.count;
    h0 = a.first_frame + f0;
    h1 = a.first_frame + f1;
    p = a.audio + MX_AUDIO_PAD - kM + 2 * lane;
    aligned = (reinterpret_cast<uintptr_t>(a.audio) & 7) == 0;
    hop = a.hop;
  }
  __device__ __forceinline__ void load(int64_t h, float2 (&x)[8]) const {
    load_frame(p, h * hop, aligned && ((h * hop) & 1) == 0, x);
  }
};

// One frame through the transform: from the lane's raw pairs x to v = Z[lane + 64 r] in registers and Z in the image in bin
// order, ready for the split (compressed, powers).  `prefetch` runs behind pass 1's last read of x: the next frame's load goes
// there and travels under this frame.  Five barriers; the caller closes the frame with one more once the image is read.
template <class Prefetch>
__device__ __forceinline__ void transform(int lane, const LaneConsts &lc, float2 (&x)[8], float2 *img, float2 (&v)[8],
                                          Prefetch &&prefetch) {
  pass1(lane, lc, x, img);
  prefetch();
  __syncthreads();
  pass2(lane, lc, img, v);
  __syncthreads();
  store2(lane, v, img);
  __syncthreads();
  pass3(lane, img, v);
  __syncthreads();
  store3(lane, v, img);
  __syncthreads();
}

}  // namespace onset
}  // namespace mx
