// compress_kernels.hip — BUILD-DEFINED dynamics compressor (the reference has none; definition: include/melonix_amd.h "Dynamics
// compressor", restated by tests/compress_ref.py; compress_core.h holds the arithmetic, tests/emu/compress_emu.cpp runs it on the
// CPU).  Binary32 comparisons up to a step's peak, integers from the table look-up to the interpolated gain, one binary64 product
// and quotient at the end: the bytes are numpy's whatever the launch split.
//
// compress_peaks_kernel: P consecutive lanes share a control step, P = cp::lanes_per_step(D) the power of two that covers the
// aligned quads a step can touch (16 at 48 kHz, 4 at 8 kHz, 64 — two rounds — at 384 kHz), so a wavefront takes 64 / P steps
// with every lane at work.  A lane loads aligned 16-byte quads (image_quads.h: the samples outside the file as zeros), skips the
// samples outside its step (D = 44: a quad may belong to two steps) and the step's maximum is a shuffle reduction over its P
// lanes — a maximum of values that are never NaN has no order — stored as 4 bytes.  One path for every D.  No atomics.
// compress_curve_kernel: a wavefront per group.  The recurrence is serial by definition, W + Gc steps a group; what is not — the
// targets — is done 64 steps at a time across the lanes, from the 8 KiB table staged in LDS; then s walks the 64 targets as a
// wave-uniform value (readlane), each lane keeping the s of its own step, and the group's own steps leave as one coalesced store
// per 64.  A lane per group (loudness_kernels.hip) would leave 879 lanes at work for the hour and read the peaks 16 KiB apart.
// compress_apply_kernel: a lane per aligned quad of the take; the two gains of the quad's step (three where it crosses into the
// next) come from the curve in L2, G_i and the quotient per sample; a quad wholly inside the range leaves as one 16-byte store
// where the output address allows, single 4-byte / 2-byte stores otherwise.
// Loads stay inside [0, n) of the image's quads, of peaks [peaks_first, ..) and of the curve between cp::gain_lo and
// cp::gain_hi; stores go to [0 .. nsteps) / [out_first, out_end) / [0 .. count) only.
#include <hip/hip_runtime.h>

#include "compress_core.h"
#include "image_quads.h"
#include "kernels.h"
#include "pcm16.h"

namespace mx {
namespace {

constexpr int kThreads = 256, kWave = 64;

__global__ __launch_bounds__(kThreads) void compress_peaks_kernel(const float *__restrict__ image, int64_t n, int D, int P,
                                                                   int64_t first_step, int64_t nsteps, float *__restrict__ out) {
  const int64_t slot = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / P;  // (P divides 64: the lanes of a slot share a wavefront)
  const int sub = (int)threadIdx.x % P;
  const bool live = slot < nsteps;
  float peak = 0.f;
  const int64_t b = first_step + slot;
  const int64_t a0 = b * D, a1 = a0 + D < n ? a0 + D : n;
  if (live && b >= 0 && a0 < n) {  // a step of the file: its quads lie inside the image's [0, n)
    const float4 *img = reinterpret_cast<const float4 *>(image);
    const int64_t ka = (a0 + MX_AUDIO_PAD) / 4, kb = (a1 - 1 + MX_AUDIO_PAD) / 4;
    for (int64_t k = ka + sub; k <= kb; k += P) {
      const float4 v = load_quad(img, k, n);
      const float x[4] = {v.x, v.y, v.z, v.w};
      const int64_t i0 = 4 * k - MX_AUDIO_PAD;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i0 + e < a0 || i0 + e >= a1) continue;
        const float m = cp::magnitude(x[e]);
        peak = m > peak ? m : peak;
      }
    }
  }
  for (int d = P / 2; d > 0; d >>= 1) {
    const float o = __shfl_xor(peak, d, kWave);
    peak = o > peak ? o : peak;
  }
  if (live && sub == 0) out[slot] = peak;
}

__global__ __launch_bounds__(kWave) void compress_curve_kernel(const CompressCurveArgs a) {
  __shared__ int32_t T[cp::kCurve];
  const int lane = threadIdx.x;
  for (int j = lane; j < cp::kCurve; j += kWave) T[j] = a.table[j];
  __syncthreads();
  const int64_t g = a.g0 + blockIdx.x;
  const int64_t start = cp::group_start(g, a.W), end = cp::group_end(g, a.total), own = g * cp::kGroup;
  int32_t s = cp::kUnity;
  for (int64_t c0 = start; c0 < end; c0 += kWave) {
    const int64_t b = c0 + lane;
    const float p = b < end ? a.peaks[b - a.peaks_first] : 0.f;  // (peaks_first <= the first group's start)
    const int32_t q = cp::target(T, p);
    const int cnt = end - c0 < kWave ? (int)(end - c0) : kWave;
    int32_t mine = 0;
#pragma unroll
    for (int i = 0; i < kWave; ++i) {
      if (i < cnt) {
        s = cp::smoothed(s, __builtin_amdgcn_readlane(q, i), a.c_att, a.c_rel);
        if (lane == i) mine = s;
      }
    }
    if (b < end && b >= own && b >= a.out_first && b < a.out_end) a.out[b - a.out_first] = mine;
  }
}

__global__ __launch_bounds__(kThreads) void compress_apply_kernel(const CompressApplyArgs a) {
  const int64_t last = a.first + a.count;  // one past the last output
  const int64_t k = (a.first + MX_AUDIO_PAD) / 4 + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t i0 = 4 * k - MX_AUDIO_PAD;  // in [first - 3, ..): >= 0
  if (i0 >= last) return;
  const int64_t lo = cp::gain_lo(a.first, a.D, a.K), hi = cp::gain_hi(a.first, a.count, a.D, a.K);
  // s_u where an output of the range reads it; unity below step 0 and where none does
  auto gain = [&](int64_t u) { return u < lo || u > hi ? cp::kUnity : a.curve[u - a.curve_first]; };
  const float4 v = load_quad(reinterpret_cast<const float4 *>(a.image), k, a.n);  // (i0 < last <= n: a quad of the file)
  const float x[4] = {v.x, v.y, v.z, v.w};
  int64_t u = i0 / a.D;
  int o = (int)(i0 - u * a.D);
  u += a.K;
  int32_t s0 = gain(u - 1), s1 = gain(u);
  float y[4];
  int16_t pcm[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (o == a.D) {  // the next step
      o = 0;
      ++u;
      s0 = s1;
      s1 = gain(u);
    }
    y[e] = cp::compressed(x[e], a.makeup, cp::gain_product(s0, s1, a.D, o), a.D);
    pcm[e] = pcm16_clamped(y[e]);
    ++o;
  }
  const int64_t at = i0 - a.first;  // of the quad's first sample in the outputs: >= -3
  if (i0 >= a.first && i0 + 4 <= last) {
    if (a.f32) {
      float *dst = a.f32 + at;
      if (reinterpret_cast<uintptr_t>(dst) % 16 == 0) {
        *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = y[e];
      }
    }
    if (a.i16) {
      int16_t *dst = a.i16 + at;
      if (reinterpret_cast<uintptr_t>(dst) % 8 == 0) {
        const uint32_t w0 = (uint32_t)(uint16_t)pcm[0] | ((uint32_t)(uint16_t)pcm[1] << 16);
        const uint32_t w1 = (uint32_t)(uint16_t)pcm[2] | ((uint32_t)(uint16_t)pcm[3] << 16);
        *reinterpret_cast<uint2 *>(dst) = make_uint2(w0, w1);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = pcm[e];
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e >= a.first && i0 + e < last) {
        if (a.f32) a.f32[at + e] = y[e];
        if (a.i16) a.i16[at + e] = pcm[e];
      }
  }
}

}  // namespace

hipError_t launch_compress_peaks(const CompressPeaksArgs &a, hipStream_t s) {
  if (a.nsteps <= 0) return hipSuccess;
  const int P = cp::lanes_per_step(a.D);
  const int64_t blocks = (a.nsteps * P + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compress_peaks_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a.image, a.n, a.D, P, a.first_step,
                     a.nsteps, a.out);
  return hipGetLastError();
}

hipError_t launch_compress_curve(const CompressCurveArgs &a, hipStream_t s) {
  if (a.groups <= 0) return hipSuccess;
  if (a.groups > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compress_curve_kernel, dim3((unsigned)a.groups), dim3(kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_compress_apply(const CompressApplyArgs &a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  const int64_t quads = (a.first + a.count - 1 + MX_AUDIO_PAD) / 4 - (a.first + MX_AUDIO_PAD) / 4 + 1;
  hipLaunchKernelGGL(compress_apply_kernel, dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace mx
