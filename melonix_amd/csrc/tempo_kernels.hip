// tempo_kernels.hip — BUILD-DEFINED tempo estimation (the reference has a Tempo slider and no estimator; definition:
// include/melonix_amd.h "Tempo and grid-offset estimation", restated by tests/tempo_ref.py).  The arithmetic is tempo_core.h's.
//
// tempo_smooth_kernel: a thread per frame, 2W + 1 coalesced taps of the flux curve, the weights in the kernel's arguments.
// tempo_comb_kernel: a workgroup of 256 threads (four 64-lane waves) per job.  Thread t scores phases t, t + 256, ..: each a
// sequential binary64 sum of f32 interpolations in ascending j, so a phase's bytes do not depend on who computes it; the lanes
// of a wave read adjacent frames.  The scores go to an LDS row of 4096 floats (16 KiB); the argmax — the highest score, the
// lowest phase among equals, a total order, so any reduction tree gives the same pair — is a per-thread pass in ascending
// phase, six shuffle steps per wave and four pairs through LDS; thread 0 writes the 16-byte record.  No atomics, nothing
// between workgroups, no scratch.  A job outside its range reads clamped indices of the curve and writes its own record only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "tempo_core.h"

namespace mx {
namespace {

using namespace tempo;

__global__ __launch_bounds__(kThreads) void tempo_smooth_kernel(const float *__restrict__ flux, int64_t count, int W,
                                                                 const SmoothWeights w, float *__restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (f < count) out[f] = smooth_at(flux, count, f, W, w);
}

__global__ __launch_bounds__(kThreads) void tempo_comb_kernel(const float *__restrict__ curve, int64_t count,
                                                               const mx_comb_job *__restrict__ jobs, int64_t job0,
                                                               mx_comb *__restrict__ out) {
  __shared__ float row[kMaxPhases];
  __shared__ float wave_score[kThreads / 64];
  __shared__ int wave_phase[kThreads / 64];
  const int t = threadIdx.x;
  const int64_t j = job0 + blockIdx.x;
  const mx_comb_job job = jobs[j];
  const int nph = phases(job.period_q16);
  float best = 0.f;
  int best_phi = kMaxPhases;  // (no phase: loses against every real one)
  for (int phi = t; phi < nph; phi += kThreads) {
    const float s = phase_score(curve, count, job, phi);
    row[phi] = s;
    if (best_phi == kMaxPhases || better(s, phi, best, best_phi)) {
      best = s;
      best_phi = phi;
    }
  }
#pragma unroll
  for (int step = 32; step >= 1; step >>= 1) {
    const float s = __shfl_xor(best, step, 64);
    const int p = __shfl_xor(best_phi, step, 64);
    if (p != kMaxPhases && (best_phi == kMaxPhases || better(s, p, best, best_phi))) {
      best = s;
      best_phi = p;
    }
  }
  if ((t & 63) == 0) {
    wave_score[t >> 6] = best;
    wave_phase[t >> 6] = best_phi;
  }
  __syncthreads();  // the row and the four pairs are written
  if (t == 0) {
    for (int w = 1; w < kThreads / 64; ++w)
      if (wave_phase[w] != kMaxPhases && better(wave_score[w], wave_phase[w], best, best_phi)) {
        best = wave_score[w];
        best_phi = wave_phase[w];
      }
    out[j] = record_at(row, nph, best_phi);  // (thread 0 always holds phase 0: best_phi < nph)
  }
}

}  // namespace

hipError_t launch_tempo_smooth(const float *d_flux, int64_t count, int width, const tempo::SmoothWeights &w, float *d_out,
                               hipStream_t s) {
  if (count <= 0) return hipSuccess;
  if (width < 0 || width > kMaxWidth || count > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((count + kThreads - 1) / kThreads)), block(kThreads);
  hipLaunchKernelGGL(tempo_smooth_kernel, grid, block, 0, s, d_flux, count, width, w, d_out);
  return hipGetLastError();
}

hipError_t launch_tempo_comb(const float *d_curve, int64_t count, const mx_comb_job *d_jobs, int64_t njobs, mx_comb *d_out,
                             hipStream_t s) {
  if (njobs <= 0) return hipSuccess;
  if (count < 1) return hipErrorInvalidValue;
  const int64_t kSlice = 1ll << 30;  // (the grid's x extent)
  for (int64_t job0 = 0; job0 < njobs; job0 += kSlice) {
    const dim3 grid((unsigned)std::min(kSlice, njobs - job0)), block(kThreads);
    hipLaunchKernelGGL(tempo_comb_kernel, grid, block, 0, s, d_curve, count, d_jobs, job0, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mx
