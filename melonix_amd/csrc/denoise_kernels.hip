// denoise_kernels.hip — BUILD-DEFINED spectral noise reduction from a noise print (the reference has none; definition:
// include/melonix_amd.h "Noise reduction", restated in f64 by tests/denoise_ref.py; denoise_core.h holds the arithmetic,
// tests/emu/denoise_emu.cpp runs it on the CPU):
//   frame f: x_j = audio[(f - 3) 256 + j], j < 1024 (zeros outside the file whatever the pads hold), periodic Hann, X = DFT_1024,
//   a_f[k] = (|X_k| / 512)^2, g = a > sens P[k] ? 1 - sens P[k] / a : 0, at least `floor`; 1-2-1 over f, then over k;
//   y_f = IDFT(G_f X_f) w 2/3;  out[t] = the sum of its four frames in ascending f from +0.f.
//
// denoise_kernel: one wavefront (a workgroup of 64 threads) owns `run` consecutive output blocks of 256 samples, [b0, b1)
// (dn::tile_of).  It analyses frames b0 - 1 .. b1 + 3 (those that exist) through onset_walk.h's transform — 16 samples per
// lane, the next frame's travelling under the current frame's passes —, keeps three frames of raw gains and the middle frame's
// spectrum in registers (bins lane + 64 r, bin 512 beside them), smooths the middle frame's gains over time and then over
// frequency — the neighbour bins come from lanes +- 1, lane 63's upper neighbour from lane 0's next row —, and takes G X back
// through the inverse of the split and the same three passes around conjugation.  The lane ends a frame with the samples it
// began one with, 128 r + 2 lane: four hop segments of two pairs, added into 16 accumulators that stand for blocks f - 3 .. f;
// block f - 3 has its fourth frame then and is stored.  A wavefront writes the blocks it owns and nothing else: the frames a
// tile shares with its neighbour are computed by both, by the same code, so the bytes do not depend on the run or on the split
// of the output range.  No atomics, no fix-up, no scratch; static LDS only (the 8 x 72-point image).
// noise_rows_kernel: the same forward path over a run of frames, the powers to HBM.  noise_print_kernel: one lane per bin walks
// the rows in ascending frame order in binary64.
// Loads stay inside the padded image (a frame reaches at most 768 samples before the file and 1023 behind it, far below
// MX_AUDIO_PAD); stores go to f32 / i16 [0 .. count) and rows [0 .. 513 count) only.
#include <hip/hip_runtime.h>

#include "denoise_core.h"
#include "onset_walk.h"
#include "pcm16.h"

namespace mx {
namespace {

using namespace dn;

// the lane's 8 sample pairs of frame f, masked to the file
__device__ __forceinline__ void load_masked(const float *image, bool aligned, int64_t n, int64_t f, int lane, float2 (&x)[8]) {
  const int64_t s0 = (f - kLead) * kHop + 2 * lane;
  const float *q = image + MX_AUDIO_PAD + s0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t s = s0 + 128 * r;
    const float2 v = aligned ? *reinterpret_cast<const float2 *>(q + 128 * r) : c_mk(q[128 * r], q[128 * r + 1]);
    x[r] = c_mk(masked(v.x, s, n), masked(v.y, s + 1, n));
  }
}

__global__ __launch_bounds__(kLanes) void denoise_kernel(const DenoiseArgs a) {
  __shared__ __attribute__((aligned(16))) float2 img[kImage];
  const int lane = threadIdx.x;
  const Tile t = tile_of(a.first, a.count, a.n, blockIdx.x, a.run);
  if (t.b0 >= t.b1) return;
  const bool aligned = (reinterpret_cast<uintptr_t>(a.image) & 7) == 0;
  LaneConsts lc;
  lane_consts(lane, a.tw, lc);
  float theta[8], theta512;
#pragma unroll
  for (int r = 0; r < 8; ++r) theta[r] = a.sens * a.print[lane + 64 * r];
  theta512 = a.sens * a.print[kM];
  const float flr = a.floor;
  const int64_t out_end = a.first + a.count;

  float gA[8], gB[8], gC[8], gA512 = 0.f, gB512 = 0.f, gC512 = 0.f;  // the raw gains of frames f - 2, f - 1, f
#pragma unroll
  for (int r = 0; r < 8; ++r) gA[r] = gB[r] = gC[r] = 0.f;
  Spec um, uc;  // the spectra of frames f - 1 and f
#pragma unroll
  for (int r = 0; r < 8; ++r) um.u[r] = uc.u[r] = c_mk(0.f, 0.f);
  um.u512 = uc.u512 = 0.f;
  Ola ola;
  ola_clear(ola);

  const int64_t last = t.b1 + 3;  // the iteration that synthesises frame b1 + 2; frames past F - 1 are not analysed
  float2 x[8];
  load_masked(a.image, aligned, a.n, t.fa, lane, x);
  for (int64_t f = t.fa; f <= last; ++f) {
    if (f < t.F) {
      float2 v[8];
      transform(lane, lc, x, img, v, [&] {
        if (f + 1 <= last && f + 1 < t.F) load_masked(a.image, aligned, a.n, f + 1, lane, x);
      });
      float p[8], p512;
      split(lane, lc, v, img, uc, p, p512);
      __syncthreads();  // the image is read: the inverse, or the next frame, may write it
#pragma unroll
      for (int r = 0; r < 8; ++r) gC[r] = raw_gain(p[r], theta[r], flr);
      gC512 = raw_gain(p512, theta512, flr);
    }
    if (f == t.fa) {  // frame -1 is frame 0 (and where fa > 0 frame fa is not synthesised: what it takes for f - 1 has no reader)
#pragma unroll
      for (int r = 0; r < 8; ++r) gB[r] = gC[r];
      gB512 = gC512;
    }
    if (f - 1 >= t.b0) {  // synthesise frame f - 1
      float tt[8], tt512, up[8], dw[8], g[8], g512;
#pragma unroll
      for (int r = 0; r < 8; ++r) tt[r] = s121(gA[r], gB[r], gC[r]);
      tt512 = s121(gA512, gB512, gC512);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        up[r] = __shfl(pub_up(lane, tt, tt512, r), (lane + 1) & (kLanes - 1), 64);
        dw[r] = __shfl(pub_dn(lane, tt, r), (lane - 1) & (kLanes - 1), 64);
      }
      const float t511 = __shfl(tt[7], kLanes - 1, 64);
      smooth_bins(lane, tt, tt512, up, dw, t511, g, g512);
      float2 v[8], c[8];
      scaled(lane, um, g, g512, img, v);
      __syncthreads();
      unsplit(lane, lc, v, img, c);
      __syncthreads();
      ipass1(lane, lc, c, img);
      __syncthreads();
      pass2(lane, lc, img, c);
      __syncthreads();
      store2(lane, c, img);
      __syncthreads();
      pass3(lane, img, c);
      __syncthreads();  // the image is read: the next frame may write it
      float2 y[8];
      windowed(lc, c, y);
      ola_add(ola, y);
      const int64_t b = f - 1 - kLead;  // the block that frame f - 1 completes
      if (b >= t.b0 && b < t.b1) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t s = b * kHop + 128 * h + 2 * lane;
          const float2 o = ola.s[0][h];
          if (s >= a.first && s < out_end) {
            if (a.f32) a.f32[s - a.first] = o.x;
            if (a.i16) a.i16[s - a.first] = pcm16_clamped(o.x);
          }
          if (s + 1 >= a.first && s + 1 < out_end) {
            if (a.f32) a.f32[s + 1 - a.first] = o.y;
            if (a.i16) a.i16[s + 1 - a.first] = pcm16_clamped(o.y);
          }
        }
      }
      ola_shift(ola);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) gA[r] = gB[r], gB[r] = gC[r];
    gA512 = gB512, gB512 = gC512;
    um = uc;
  }
}

__global__ __launch_bounds__(kLanes) void noise_rows_kernel(const NoiseRowsArgs a) {
  __shared__ __attribute__((aligned(16))) float2 img[kImage];
  const int lane = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * a.run, i1 = i0 + a.run < a.count ? i0 + a.run : a.count;
  if (i0 >= i1) return;
  const bool aligned = (reinterpret_cast<uintptr_t>(a.image) & 7) == 0;
  LaneConsts lc;
  lane_consts(lane, a.tw, lc);
  float2 x[8];
  load_masked(a.image, aligned, a.n, a.first_frame + i0, lane, x);
  for (int64_t i = i0; i < i1; ++i) {
    float2 v[8];
    transform(lane, lc, x, img, v, [&] {
      if (i + 1 < i1) load_masked(a.image, aligned, a.n, a.first_frame + i + 1, lane, x);
    });
    Spec u;
    float p[8], p512;
    split(lane, lc, v, img, u, p, p512);
    __syncthreads();  // the image is read: the next frame may write it
    float *row = a.rows + i * kBins;
#pragma unroll
    for (int r = 0; r < 8; ++r) row[lane + 64 * r] = p[r];
    if (lane == 0) row[kM] = p512;
  }
}

__global__ __launch_bounds__(kLanes) void noise_print_kernel(const float *__restrict__ rows, int64_t count, float *__restrict__ print) {
  const int k = blockIdx.x * kLanes + threadIdx.x;
  if (k >= kBins) return;
  double s = 0.0;
  for (int64_t f = 0; f < count; ++f) s += (double)rows[f * kBins + k];
  print[k] = (float)(s / (double)count);
}

}  // namespace

// blocks per wavefront where the caller pins none: long runs (a tile pays five frames of analysis and three of synthesis beyond
// its own) where there are tiles enough to fill the device with them
static int denoise_default_run(int64_t blocks) {
  const int64_t want = blocks / 2048;
  return (int)(want < 4 ? 4 : want > kMaxRun ? kMaxRun : want);
}

hipError_t launch_denoise(const DenoiseArgs &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  DenoiseArgs a = a0;
  const int64_t blocks = (a.first + a.count + kHop - 1) / kHop - a.first / kHop;
  const dim3 grid = walk_grid(blocks, a.run, denoise_default_run(blocks)), block(kLanes);
  hipLaunchKernelGGL(denoise_kernel, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_noise_rows(const NoiseRowsArgs &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  NoiseRowsArgs a = a0;
  const dim3 grid = walk_grid(a.count, a.run, onset_default_run(a.count)), block(kLanes);
  hipLaunchKernelGGL(noise_rows_kernel, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_noise_print(const float *rows, int64_t count, float *print, hipStream_t s) {
  if (count <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(noise_print_kernel, dim3((kBins + kLanes - 1) / kLanes), dim3(kLanes), 0, s, rows, count, print);
  return hipGetLastError();
}

}  // namespace mx
