// chroma_kernels.hip — BUILD-DEFINED chroma records and their window sums (the reference has no detector; definition:
// include/melonix_amd.h "Key, scale and tuning reference", restated in f64 by tests/key_ref.py; arithmetic: chroma_core.h).
//
// chroma_frames: the f0 tracker's walk (f0_kernels.hip) with a Hann window in front and another tail.  One workgroup
// (Plan<4096,16>: 128 threads, two wavefronts) takes a run of consecutive frames; per frame ONE forward real transform —
// stft_core.h's three passes and the real-FFT split, through wave_walk.h — where the tracker runs three and an inverse.  The
// window table carries 1/2048, so the split's 2 X comes out as X / 1024 and a magnitude is one square root.  The tail:
//   the 2048 magnitudes go to an LDS image of their own in bin order (padded one word per 16: a thread's 16 consecutive bins and
//   their two neighbours sit on their own banks), so the FFT image is free as soon as every wave has left pass 3;
//   the band maximum: each thread over its 16 bins, a DPP reduction of the float bits, one LDS word per wave;
//   the peaks: a 16-bit mask per thread, an inclusive DPP scan of the counts over the wave, the first wave's total added to the
//   second — so the frame's peaks are compacted into the FFT image in ascending bin order, 16 bytes each (at most 1023: no two
//   neighbouring bins are peaks), every peak's logarithms, cents and phasor computed once by the thread that owns its bin;
//   forty lanes of wave 0 then walk that list front to back, each adding what falls into its column.
// One accumulation order per column and no atomics: a record depends on its frame's samples alone, the same bytes whatever the
// launch split or the run length.  A frame holding Inf or NaN has no finite bin (every output of the transform is a sum over
// every input), so its band maximum is not finite and it has no peaks: forty zeros, like a silent frame.  No scratch, no
// spectrum to HBM, 160 bytes per frame written.
//
// chroma_sum: one lane per (job, column) walks its window's records front to back into a binary64 sum: the forty lanes of a
// job read one record's 160 bytes together.
#include <hip/hip_runtime.h>

#include "chroma_core.h"
#include "kernels.h"
#include "wave_walk.h"

namespace mx {
namespace {

using namespace chroma;
using FP = Plan<4096, 16>;
static_assert(kPlan4096E == 16 && FP::T == 128 && FP::R3 == 8 && FP::M == kBins, "the chroma kernel runs on Plan<4096,16>");
static_assert(t1_size<FP>() == FP::M, "one spectrum fills the FFT image");
static_assert(4 * (kMaxPeaks + 1) <= 2 * FP::M, "the peak list fits the FFT image (as floats)");
static_assert(16 * FP::T == kBins && kCols <= 64, "16 bins per thread, the columns in one wave");

// wave_walk.h's three passes on the register image Y (thread t's point c = t + T*e in Y[e]) and the real-FFT split:
// X[o] = 2 * DFT_N(y)[out_bin(t, o)].  The passes' first barrier is behind every wave's last read of the previous frame's peak
// list.  Leaves the image busy: the caller synchronises before it writes it.
__device__ __forceinline__ void forward(int t, bool wave0, const cpx (&Y)[FP::E], cpx (&X)[FP::E], cpx *img, const cpx *ltw2,
                                        const cpx (&w3b)[3], cpx ulo0, cpx uhi0) {
  cpx v[FP::E];
  walk_passes<FP>(t, wave0, Y, v, img, ltw2, w3b);
  post_split<FP>(t, wave0, ulo0, uhi0, v, X);
}

__global__ __launch_bounds__(FP::T) void chroma_frames(const ChromaArgs a) {
  using P = FP;
  __shared__ __attribute__((aligned(16))) float2 img[P::M];     // FFT image; then the frame's peaks, 16 bytes each
  __shared__ __attribute__((aligned(16))) float2 ltw2[P::TW2];  // pass-2 twiddles
  __shared__ float mag[kMagLen];                                // the magnitudes in bin order
  __shared__ unsigned s_max[2];                                 // the band maximum's bits, per wavefront
  __shared__ int s_cnt[2];                                      // the peaks, per wavefront
  float *const list = reinterpret_cast<float *>(img);
  const int t_ = threadIdx.x;
  const bool wave0 = __builtin_amdgcn_readfirstlane(t_) < 64;
  const int lane = t_ & 63;
  cpx ulo0, uhi0;
  post_bases<P>(t_, a.ubase, ulo0, uhi0);
  cpx w3b[3];
  load_w3_bases<P>(a.tw3, t_ ? t_ : P::NS3 / 2, w3b);
  fill_ltw2<P>(t_, a.tw2, ltw2);

  int64_t f0, f1;
  block_run(a.frames_per_block, a.count, f0, f1);
  if (f0 >= f1) return;
  const float *const base = a.audio + MX_AUDIO_PAD - kBins;
  cpx xr[P::E];
  load_raw<P, false>(t_, xr, base + (a.first_frame + f0) * (int64_t)a.hop);
  __syncthreads();  // the twiddles are there

  for (int64_t f = f0; f < f1; ++f) {
    int t = t_;
    asm volatile("" : "+v"(t));
    cpx Y[P::E], X[P::E];
    apply_window<P, 1, true>(t, Y, xr, a.hann);
    if (f + 1 < f1) load_raw<P, false>(t, xr, base + (a.first_frame + f + 1) * (int64_t)a.hop);  // travels under this frame
    forward(t, wave0, Y, X, img, ltw2, w3b, ulo0, uhi0);
#pragma unroll
    for (int o = 0; o < P::E; ++o) mag[mag_idx(out_bin<P>(t, o))] = __builtin_sqrtf(X[o].x * X[o].x + X[o].y * X[o].y);
    __syncthreads();  // the magnitudes are complete; every wave has left pass 3: the FFT image is free
    const int k0 = 16 * t;
    float mv[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      const int k = k0 - 1 + j;
      mv[j] = k >= 0 && k < kBins ? mag[mag_idx(k)] : 0.f;
    }
    const unsigned wmax = wave_reduce_u32<true>(band_max_bits(k0, mv, a.kmin, a.kmax));
    if (lane == 0) s_max[t >> 6] = wmax;
    __syncthreads();
    const unsigned mbits = s_max[0] > s_max[1] ? s_max[0] : s_max[1];
    uint32_t mask = 0;  // (a frame holding Inf or NaN: no peaks)
    if (mbits < 0x7f800000u) mask = peak_mask(k0, mv, a.kmin, a.kmax, threshold_of(a.floor_abs, a.rel, __uint_as_float(mbits)));
    const int cnt = __popc(mask);
    const int incl = wave_scan_add(cnt);
    if (lane == 63) s_cnt[t >> 6] = incl;
    __syncthreads();
    int at = incl - cnt + (wave0 ? 0 : s_cnt[0]);
    const int total = s_cnt[0] + s_cnt[1];
    while (mask) {  // the thread's peaks, in ascending bin order, behind those of the threads before it
      const int k = k0 + __builtin_ctz(mask);
      mask &= mask - 1;
      const Peak q = peak_of(k, mag[mag_idx(k - 1)], mag[mag_idx(k)], mag[mag_idx(k + 1)], a.bin_hz);
      float *const e = list + 4 * at++;
      e[0] = q.m, e[1] = q.p, e[2] = q.c, e[3] = q.s;
    }
    __syncthreads();  // the list is complete
    if (t < kCols) {
      float acc = 0.f;
      for (int i = 0; i < total; ++i) {
        const float *const e = list + 4 * i;  // (one address for every lane: a broadcast)
        acc += column_term(t, Peak{e[0], e[1], e[2], e[3]});
      }
      reinterpret_cast<float *>(a.out + f)[t] = acc;
    }
    // (the next frame writes the image behind forward()'s first barrier, the magnitudes and the two counters behind more)
  }
}

__global__ __launch_bounds__(64) void chroma_sum(const float *rec, int64_t count, const mx_chroma_job *jobs, double *out) {
  const int col = threadIdx.x;
  if (col >= kCols) return;
  const mx_chroma_job job = jobs[blockIdx.x];
  const int64_t lo = job.first_frame < 0 ? 0 : job.first_frame < count ? job.first_frame : count;
  const int64_t n = job.frames < 0 ? 0 : job.frames < count - lo ? job.frames : count - lo;
  const float *p = rec + lo * kCols + col;
  double acc = 0.0;
  int64_t i = 0;
  for (; i + 8 <= n; i += 8) {  // eight loads in flight, added in frame order
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[(i + j) * kCols];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += sum_term(v[j]);
  }
  for (; i < n; ++i) acc += sum_term(p[i * kCols]);
  out[(int64_t)blockIdx.x * kCols + col] = acc;
}

}  // namespace

hipError_t launch_chroma(const ChromaArgs &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  ChromaArgs a = a0;
  const dim3 grid = walk_grid(a.count, a.frames_per_block, kPlan4096Run);
  hipLaunchKernelGGL(chroma_frames, grid, dim3(FP::T), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_chroma_sum(const mx_chroma_rec *rec, int64_t count, const mx_chroma_job *jobs, int64_t njobs, double *out,
                             hipStream_t s) {
  if (njobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(chroma_sum, dim3((unsigned)njobs), dim3(64), 0, s, reinterpret_cast<const float *>(rec), count, jobs, out);
  return hipGetLastError();
}

}  // namespace mx
