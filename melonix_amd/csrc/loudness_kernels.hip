// loudness_kernels.hip — BUILD-DEFINED loudness records (definition: include/melonix_amd.h "Loudness and note levelling"): per
// 10 ms step the K-weighted energy in binary64 and the sample peak, 16 bytes.  No contraction: the bytes are numpy's
// (loudness_core.h holds the arithmetic; tests/emu/loudness_emu.cpp runs it on the CPU).
//
// One lane owns one group — W warm-up samples from zero state, then ten steps: the recurrence is serial by definition, the
// parallelism is across groups (36 000 lanes for an hour at 48 kHz, one wavefront per workgroup so that they spread over every
// SIMD).  Consecutive lanes read addresses G*S samples apart, so a lane loads for itself: 16-byte loads of the padded image at
// 16-byte-aligned addresses, four of them (16 samples) a block, the next block's in flight while this one is filtered.  A
// group start that is no multiple of 4 samples (S = 441 at 44.1 kHz: every other group) costs nothing extra: the lane walks the
// aligned blocks that cover [i0, end) and skips the samples outside.  A record leaves as one 16-byte store.  No LDS, no
// atomics, nothing shared between lanes.  Loads stay inside the padded image (i0 >= -W >= -MX_AUDIO_PAD, end <= n), stores
// inside the records of the lane's own group that exist (ceil((end - g G S) / S) <= G).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "loudness_core.h"

namespace mx {
namespace {

constexpr int kThreads = 64;  // one wavefront
constexpr int kQuads = 4;     // 16-byte loads per block
constexpr int kBlock = 4 * kQuads;
static_assert(MX_AUDIO_PAD % kBlock == 0, "an aligned block of the image is an aligned block of the samples");

struct Block {
  float4 q[kQuads];
};
__device__ __forceinline__ Block load_block(const float4 *img, int64_t blk) {
  Block b;
#pragma unroll
  for (int j = 0; j < kQuads; ++j) b.q[j] = img[blk * kQuads + j];
  return b;
}
__device__ __forceinline__ float element(const Block &b, int e) {
  const float4 v = b.q[e >> 2];
  return (e & 3) == 0 ? v.x : (e & 3) == 1 ? v.y : (e & 3) == 2 ? v.z : v.w;
}

__global__ __launch_bounds__(kThreads) void loudness_steps_kernel(const float *__restrict__ image, int64_t n, int S, int W,
                                                                   int64_t first_group, int64_t ngroups, loud::Coeffs c,
                                                                   mx_loud_step *__restrict__ out) {
  const int64_t lane = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (lane >= ngroups) return;
  const int64_t gstart = (first_group + lane) * loud::kGroupSteps * (int64_t)S, i0 = gstart - W;
  const int64_t end = gstart + (int64_t)loud::kGroupSteps * S < n ? gstart + (int64_t)loud::kGroupSteps * S : n;
  // r = i - i0, the sample's place in the lane's walk: [0, len) is walked, r < zeros lies before the file, r >= W is measured
  const int len = (int)(end - i0), zeros = i0 < 0 ? (int)-i0 : 0;
  const int64_t p0 = i0 + MX_AUDIO_PAD;  // (>= 0: W <= MX_AUDIO_PAD)
  const float4 *img = reinterpret_cast<const float4 *>(image);
  uint4 *rec = reinterpret_cast<uint4 *>(out + lane * loud::kGroupSteps);
  loud::Lane l = loud::lane_zero();
  int in_step = 0;
  int64_t blk = p0 / kBlock;
  const int64_t last = (p0 + len - 1) / kBlock;
  int r0 = (int)(blk * kBlock - p0);  // of the block's first sample: in (-kBlock, 0]
  Block cur = load_block(img, blk);
  for (; blk <= last; ++blk, r0 += kBlock) {
    Block nxt = cur;
    if (blk < last) nxt = load_block(img, blk + 1);
#pragma unroll
    for (int e = 0; e < kBlock; ++e) {
      const int r = r0 + e;
      if (r < 0 || r >= len) continue;
      const float x = r < zeros ? 0.f : element(cur, e);
      const double z = loud::filter(c, l, x);
      if (r < W) continue;
      loud::accumulate(l, x, z);
      if (++in_step == S || r == len - 1) {
        const mx_loud_step s = loud::record(l, in_step);
        *rec++ = make_uint4((uint32_t)__double2loint(s.energy), (uint32_t)__double2hiint(s.energy), __float_as_uint(s.peak),
                            (uint32_t)s.samples);
        loud::step_zero(l);
        in_step = 0;
      }
    }
    cur = nxt;
  }
}

}  // namespace

hipError_t launch_loudness_steps(const LoudnessArgs &a, hipStream_t s) {
  if (a.ngroups <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.ngroups + kThreads - 1) / kThreads)), block(kThreads);
  const double *k = a.coeffs;
  const loud::Coeffs c{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9]};
  hipLaunchKernelGGL(loudness_steps_kernel, grid, block, 0, s, a.image, a.n, a.S, a.W, a.first_group, a.ngroups, c, a.out);
  return hipGetLastError();
}

}  // namespace mx
