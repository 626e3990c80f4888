// truepeak_kernels.hip — BUILD-DEFINED true-peak records and look-ahead limiter (definition: include/melonix_amd.h "True peak,
// limiter and loudness range"; truepeak_core.h holds the arithmetic, tests/emu/truepeak_emu.cpp runs it on the CPU).  Binary32
// without contraction up to a sample's peak, integers from there to the gain, one binary64 quotient and product at the end: the
// bytes are numpy's whatever the tiling.
//
// truepeak_steps_kernel: a workgroup of 256 threads takes a run of consecutive steps (about 4096 samples, steps_per_block),
// stages the run with its halo — the aligned quads that cover [first sample - 5, last sample + 6], 16-byte loads, samples
// outside the file as zeros — in LDS once, then each wavefront walks whole steps of the run: a lane takes an aligned quad of
// LDS with its two neighbours either side (five ds_read_b128, conflict-free: consecutive lanes, consecutive slots), which holds
// the 12-sample window of each of its four samples, and skips the samples outside the step (S = 441: a quad may belong to two
// steps).  The step's two maxima are a shuffle reduction over the wavefront — a maximum of values that are never NaN has no
// order — and leave as one 8-byte store.  No atomics.
//
// limit_kernel: one launch, a workgroup per tile of 2048 outputs.  Staged x over the tile +- (A + 6) -> p -> q (Q30) over the
// tile +- A; the sliding minimum of width A + 1 as a sparse table, floor(log2(A + 1)) doubling passes that ping-pong between the
// two LDS buffers (a lane moves quads: the shift is a multiple of 4 from the third pass on, the first two take the next quad
// too), then min(M[t], M[t + A + 1 - 2^K]); each thread keeps its 12 consecutive minima in registers, their int64 prefix sums
// (wave scan by shuffles, four wave totals through LDS) overlay both buffers, and s_i is a difference of two of them.  The
// x of the outputs is read again from the image (L2) for the product.  A tile whose q are all unity skips the passes: its sums
// are (A + 1) << 30, the same bytes.  33 KiB of static LDS whatever A is.
// Loads stay inside the padded image (at most A + 6 + 11 + the tile's rest, far below MX_AUDIO_PAD, either side); stores go to
// [0, n) of the outputs only.
#include <hip/hip_runtime.h>

#include "image_quads.h"
#include "kernels.h"
#include "pcm16.h"
#include "truepeak_core.h"

namespace mx {
namespace {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr int kHalo = 2;  // quads either side of a lane's quad: 8 samples, at least the 5 before and the 6 after a sample
static_assert(4 * kHalo >= tp::kAfter && 4 * kHalo >= tp::kBefore, "the halo holds every window of the quad");

// quads k - 2 .. k + 2 of an LDS image as 20 floats: w[8 + e] is sample e of quad k
__device__ __forceinline__ void read_window(const float4 *lds, int k, float (&w)[4 * (2 * kHalo + 1)]) {
#pragma unroll
  for (int j = 0; j < 2 * kHalo + 1; ++j) {
    const float4 v = lds[k - kHalo + j];
    w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const float o = __shfl_xor(v, d, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// ---- records ----
constexpr int kStageQuads = 4096 / 4 + 2 * kHalo + 4;  // a run of at most 4096 samples (steps_per_block), its halo, the alignment

__global__ __launch_bounds__(kThreads) void truepeak_steps_kernel(const float *__restrict__ image, int64_t n, int S, int L,
                                                                   int64_t first_step, int64_t nsteps, int run,
                                                                   mx_tp_step *__restrict__ out) {
  __shared__ float4 stage[kStageQuads];
  const int64_t r0 = (int64_t)blockIdx.x * run;  // the run's first record
  const int cnt = (int)(nsteps - r0 < run ? nsteps - r0 : run);
  const int64_t s0 = (first_step + r0) * S;
  const int64_t s1 = s0 + (int64_t)cnt * S < n ? s0 + (int64_t)cnt * S : n;  // (s0 < n: the step exists)
  const int64_t q0 = (s0 + MX_AUDIO_PAD) / 4 - kHalo;                          // >= MX_AUDIO_PAD / 4 - 2
  const int nq = (int)((s1 - 1 + MX_AUDIO_PAD) / 4 + kHalo - q0) + 1;          // <= cnt * S / 4 + 2 * kHalo + 2
  const float4 *img = reinterpret_cast<const float4 *>(image);
  for (int k = threadIdx.x; k < nq && k < kStageQuads; k += kThreads) stage[k] = load_quad(img, q0 + k, n);
  __syncthreads();
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  for (int st = wave; st < cnt; st += kWaves) {
    const int64_t a0 = s0 + (int64_t)st * S, a1 = a0 + S < n ? a0 + S : n;
    const int ka = (int)((a0 + MX_AUDIO_PAD) / 4 - q0), kb = (int)((a1 - 1 + MX_AUDIO_PAD) / 4 - q0);  // 2 <= ka, kb <= nq - 3
    float true_peak = 0.f, sample_peak = 0.f;
    for (int k = ka + lane; k <= kb; k += kWave) {
      float w[4 * (2 * kHalo + 1)];
      read_window(stage, k, w);
      const int64_t i0 = 4 * (q0 + k) - MX_AUDIO_PAD;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i0 + e < a0 || i0 + e >= a1) continue;
        const float p = tp::sample_peak(&w[4 * kHalo + e - tp::kBefore], L), m = tp::sample_magnitude(w[4 * kHalo + e]);
        true_peak = p > true_peak ? p : true_peak;
        sample_peak = m > sample_peak ? m : sample_peak;
      }
    }
    true_peak = wave_max(true_peak);
    sample_peak = wave_max(sample_peak);
    if (lane == 0) *reinterpret_cast<float2 *>(out + r0 + st) = make_float2(true_peak, sample_peak);
  }
}

// ---- limiter ----
constexpr int kTile = 2048;                                                  // outputs per workgroup
constexpr int kBufQuads = (kTile + 2 * tp::kMaxLookahead) / 4 + 2 * kHalo + 4;  // x, then q, over the tile +- A, halo and alignment
constexpr int kChunk = (kTile + tp::kMaxLookahead + kThreads - 1) / kThreads;  // window minima per thread: 12
static_assert(kTile % 4 == 0 && kTile / 4 == 2 * kThreads, "two output quads per thread");
static_assert((size_t)2 * kBufQuads * sizeof(int4) >= (size_t)(kTile + tp::kMaxLookahead) * sizeof(int64_t), "the prefix sums fit");
static_assert((size_t)2 * kBufQuads * sizeof(int4) + kWaves * sizeof(int64_t) <= 65536, "static LDS");

__device__ __forceinline__ int imin(int a, int b) { return b < a ? b : a; }
__device__ __forceinline__ int4 min4(int4 a, int4 b) { return make_int4(imin(a.x, b.x), imin(a.y, b.y), imin(a.z, b.z), imin(a.w, b.w)); }

__global__ __launch_bounds__(kThreads) void limit_kernel(const float *__restrict__ image, int64_t n, int L, float ceiling, int A,
                                                          float *__restrict__ dst, int16_t *__restrict__ pcm) {
  __shared__ int4 buf[2][kBufQuads];
  __shared__ int64_t wave_total[kWaves];
  const int64_t t0 = (int64_t)blockIdx.x * kTile;
  // local index l <-> sample base + l, base a multiple of 4 at least 4 * kHalo below the first q (sample t0 - A)
  const int64_t bq = (t0 - A + MX_AUDIO_PAD) / 4 - kHalo;  // the staged image's first quad (> 0: A + 8 < MX_AUDIO_PAD)
  const int64_t base = 4 * bq - MX_AUDIO_PAD;
  const int off = (int)(t0 - A - base);                   // of the first q: in [4 * kHalo, 4 * kHalo + 3]
  const int nQ = kTile + 2 * A;                           // q values: samples [t0 - A, t0 + kTile + A)
  const int lastq = (off + nQ - 1) / 4;                   // the quad of the last q
  const int nquads = lastq + kHalo + 1;                   // staged: <= (11 + 4096 - 1) / 4 + 3 = 1029 <= kBufQuads
  const float4 *img = reinterpret_cast<const float4 *>(image);
  float4 *xs = reinterpret_cast<float4 *>(buf[0]);
  for (int k = threadIdx.x; k < nquads; k += kThreads) xs[k] = load_quad(img, bq + k, n);
  __syncthreads();
  // p -> q of quads [kHalo, lastq] into buf[1]; unity outside the file (and outside the q range: never read)
  int over = 0;  // a q of this thread's below unity
  for (int k = threadIdx.x; k < nquads; k += kThreads) {
    int4 q = make_int4(tp::kUnity, tp::kUnity, tp::kUnity, tp::kUnity);
    const int64_t i0 = base + 4 * k;
    if (k >= kHalo && k <= lastq && i0 + 3 >= 0 && i0 < n) {
      float w[4 * (2 * kHalo + 1)];
      read_window(xs, k, w);
      int v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool inside = i0 + e >= 0 && i0 + e < n;
        v[e] = inside ? tp::required_gain(tp::sample_peak(&w[4 * kHalo + e - tp::kBefore], L), ceiling) : tp::kUnity;
        over |= v[e] != tp::kUnity;
      }
      q = make_int4(v[0], v[1], v[2], v[3]);
    }
    buf[1][k] = q;
  }
  // A tile with every q at unity — nothing within A of it is over the ceiling — has every window minimum at unity and every sum
  // at (A + 1) << 30: the passes below would compute just that.  Most tiles of a take that needs a limiter at all are such.
  const bool idle = !__syncthreads_or(over);
  const int64_t *P = reinterpret_cast<const int64_t *>(&buf[0][0]);  // P[e] = m_0 + .. + m_e, once the passes have run
  if (!idle) {
    // sparse table: after pass j, M[l] = min q[l .. l + 2^(j+1)); entries whose range passes the staged end hold less and are not read
    const int width = A + 1;
    int cur = 1, span = 1;
    for (; 2 * span <= width; span *= 2, cur ^= 1) {
      const int4 *src = buf[cur];
      int4 *to = buf[cur ^ 1];
      const int4 unity = make_int4(tp::kUnity, tp::kUnity, tp::kUnity, tp::kUnity);
      for (int k = threadIdx.x; k < nquads; k += kThreads) {
        const int4 a = src[k];
        int4 b;
        if (span >= 4) {
          b = k + span / 4 < nquads ? src[k + span / 4] : unity;
        } else {
          const int4 c = k + 1 < nquads ? src[k + 1] : unity;
          b = span == 1 ? make_int4(a.y, a.z, a.w, c.x) : make_int4(a.z, a.w, c.x, c.y);
        }
        to[k] = min4(a, b);
      }
      __syncthreads();
    }
    // m_t = min(M[t], M[t + width - span]) for the kTile + A window starts t = t0 - A + e: a thread's kChunk consecutive ones
    const int *M = reinterpret_cast<const int *>(buf[cur]);
    const int nm = kTile + A, e0 = threadIdx.x * kChunk;
    int m[kChunk];
    int64_t sum = 0;
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      const int e = e0 + r;
      m[r] = e < nm ? imin(M[off + e], M[off + e + width - span]) : 0;
      sum += m[r];
    }
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    int64_t incl = sum;  // inclusive scan of the threads' sums over the wavefront
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
      const int64_t o = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();  // (every read of M lies before it: the prefix sums may overlay both buffers)
    int64_t before = incl - sum;
    for (int v = 0; v < wave; ++v) before += wave_total[v];
    int64_t *Pw = reinterpret_cast<int64_t *>(&buf[0][0]);
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      before += m[r];
      if (e0 + r < nm) Pw[e0 + r] = before;
    }
    __syncthreads();
  }
  // s_i = sum of m over t in [i - A, i] = P[io + A] - P[io - 1], io = i - t0
  const bool pcm_quads = pcm && reinterpret_cast<uintptr_t>(pcm) % 8 == 0;
#pragma unroll
  for (int round = 0; round < kTile / 4 / kThreads; ++round) {
    const int io = 4 * (round * kThreads + (int)threadIdx.x);
    const int64_t i = t0 + io;
    if (i >= n) break;
    const float4 xv = *reinterpret_cast<const float4 *>(image + MX_AUDIO_PAD + i);  // (inside the padded image: i < n)
    const float x[4] = {xv.x, xv.y, xv.z, xv.w};
    float y[4];
    int16_t s16[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t s = idle ? (int64_t)(A + 1) << 30 : P[io + e + A] - (io + e > 0 ? P[io + e - 1] : 0);
      y[e] = tp::limited(x[e], s, A);
      s16[e] = pcm16_clamped(y[e]);
    }
    if (i + 4 <= n) {
      *reinterpret_cast<float4 *>(dst + i) = make_float4(y[0], y[1], y[2], y[3]);
      if (pcm_quads) {
        const uint32_t lo = (uint32_t)(uint16_t)s16[0] | ((uint32_t)(uint16_t)s16[1] << 16);
        const uint32_t hi = (uint32_t)(uint16_t)s16[2] | ((uint32_t)(uint16_t)s16[3] << 16);
        *reinterpret_cast<uint2 *>(pcm + i) = make_uint2(lo, hi);
      } else if (pcm) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pcm[i + e] = s16[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < n) {
          dst[i + e] = y[e];
          if (pcm) pcm[i + e] = s16[e];
        }
    }
  }
}

}  // namespace

hipError_t launch_true_peak_steps(const TruePeakArgs &a, hipStream_t s) {
  if (a.nsteps <= 0) return hipSuccess;
  const int run = tp::steps_per_block(a.S);
  const dim3 grid((unsigned)((a.nsteps + run - 1) / run)), block(kThreads);
  hipLaunchKernelGGL(truepeak_steps_kernel, grid, block, 0, s, a.image, a.n, a.S, a.L, a.first_step, a.nsteps, run, a.out);
  return hipGetLastError();
}

hipError_t launch_audio_limit(const LimitArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n + kTile - 1) / kTile)), block(kThreads);
  hipLaunchKernelGGL(limit_kernel, grid, block, 0, s, a.image, a.n, a.L, a.ceiling, a.lookahead, a.dst, a.pcm16);
  return hipGetLastError();
}

}  // namespace mx
