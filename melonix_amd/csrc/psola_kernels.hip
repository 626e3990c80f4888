// psola_kernels.hip — the overlap-add of the build-defined PSOLA renderer (definition: include/melonix_amd.h; no reference
// counterpart).  The host plans the grains (psola_plan.cpp); given the records every output sample is independent.
//
// One workgroup per tile of kPsolaTile consecutive outputs.  The records are ordered by centre + centre_frac and no window
// reaches further than kPsolaReach from its centre, so the grains that can touch a tile are one run of the array: a 256-ary
// search (one probe per thread and round: three rounds for a million grains, where a binary search would be twenty dependent
// loads) finds its first record, and the workgroup walks on from there in chunks of kPsolaChunk records staged in LDS until
// a chunk holds a record beyond the tile's reach.  Every thread walks a chunk in record order for its kPsolaPer samples
// (tile_lo + tid + 256 q: a wave's 64 samples are consecutive, loads and stores coalesce), so each sample's two sums take
// their terms in ascending k whatever the tiling.
//
// The device form cannot validate its records: every scan stays inside [0, ngrains), the source index is clamped into the
// padded buffer, and nothing is stored outside [0, nsamples) — bad records give wrong samples, never a fault.
//
// Two instantiations of the one tile walk, on the record: mx_psola_grain reads the source at i + src_off with the record's
// fraction; mx_psola_fgrain (the formant shift) at the Q16 position src_idx.src_q + step (i - centre).  Only psola_source —
// the source index and fraction of a sample — differs; search, staging, order, sums and stores are written once.
//
// Built with -ffp-contract=off: x = (1 - f) * a0 + f * a1 is the resampler's form (resynth_kernels.hip), and S += w * x rounds
// the product before the sum, as the f64 restatement orders it.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pcm16.h"
#include "psola_plan.h"

#pragma clang fp contract(off)

namespace mx {

namespace {

constexpr int kPsolaThreads = 256;
constexpr int kPsolaPer = 4;
constexpr int kPsolaTile = kPsolaThreads * kPsolaPer;
constexpr int kPsolaChunk = kPsolaThreads;  // one record per thread and chunk: 8 KiB of LDS
// a grain's samples lie within kPsolaReach of `centre`, and centre <= centre + centre_frac < centre + 1
constexpr int kPsolaKeyReach = kPsolaReach + 1;

static_assert(sizeof(mx_psola_grain) == 32 && sizeof(mx_psola_fgrain) == 32, "two 16-byte LDS reads per record");

template <class Rec>
__device__ __forceinline__ double psola_key(const Rec *g) {
  return (double)g->centre + (double)g->centre_frac;
}

// where output sample i of a grain reads the source: index (not yet clamped) and fraction
__device__ __forceinline__ void psola_source(const mx_psola_grain &g, int i, int64_t &idx, float &f) {
  idx = (int64_t)i + (int64_t)g.src_off;
  f = g.src_frac;
}
// pos = (src_idx << 16) + src_q + step (i - centre): the low part stays under 2^30 for records that keep the precondition
// (src_q < 2^16, step <= 2^17, |i - centre| <= 2049); unsigned, so that records that break it wrap instead of overflowing
__device__ __forceinline__ void psola_source(const mx_psola_fgrain &g, int i, int64_t &idx, float &f) {
  const unsigned t = g.src_q + g.step * ((unsigned)i - (unsigned)g.centre);
  idx = (int64_t)g.src_idx + (int64_t)((int)t >> 16);
  f = (float)(t & 65535u) * (1.f / 65536.f);
}

template <class Rec>
__global__ __launch_bounds__(kPsolaThreads) void psola_kernel(const PsolaArgsT<Rec> a) {
  __shared__ __attribute__((aligned(16))) Rec recs[kPsolaChunk];
  __shared__ int wave_count[kPsolaThreads / 64];
  __shared__ int past_tile;
  const int tid = threadIdx.x;
  const int64_t tile_lo = (int64_t)blockIdx.x * kPsolaTile;
  const double key_lo = (double)(tile_lo - kPsolaKeyReach), key_hi = (double)(tile_lo + kPsolaTile - 1 + kPsolaKeyReach);
  if (tid == 0) past_tile = 0;

  // the first record with key >= key_lo, in [lo, hi]: thread t probes the end of the t-th of 256 equal pieces
  int64_t lo = 0, hi = a.ngrains;
  while (hi > lo) {
    const int64_t step = (hi - lo + kPsolaThreads - 1) / kPsolaThreads;
    const int64_t p = lo + (int64_t)(tid + 1) * step - 1;
    const bool below = p < hi && psola_key(a.grains + p) < key_lo;
    const unsigned long long b = __ballot(below);
    if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(b);
    __syncthreads();
    const int c = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    __syncthreads();
    // (sorted keys: the first c probes are below.  Unsorted ones give some c in [0, 256]: the interval shrinks all the same)
    const int64_t nlo = lo + (int64_t)c * step, nhi = lo + (int64_t)(c + 1) * step - 1;
    hi = nhi < hi ? nhi : hi;
    lo = nlo < hi ? nlo : hi;
  }

  const unsigned i0 = (unsigned)tile_lo + (unsigned)tid;  // (the last tile of a 2^31-sample render passes INT32_MAX: no store there)
  const int64_t idx_max = a.n + (int64_t)MX_AUDIO_PAD - 2;  // idx + 1 is read as well
  const float *src = a.audio + MX_AUDIO_PAD;
  float S[kPsolaPer], W[kPsolaPer];
#pragma unroll
  for (int q = 0; q < kPsolaPer; ++q) S[q] = W[q] = 0.f;

  for (int64_t base = lo; base < a.ngrains; base += kPsolaChunk) {
    const int64_t rest = a.ngrains - base;
    const int cnt = rest < kPsolaChunk ? (int)rest : kPsolaChunk;
    if (tid < cnt) {
      const Rec g = a.grains[base + tid];
      recs[tid] = g;
      if (psola_key(&g) > key_hi) past_tile = 1;
    }
    __syncthreads();
    const int last = past_tile;
    for (int j = 0; j < cnt; ++j) {
      const Rec g = recs[j];  // (the same address in every lane: a broadcast)
#pragma unroll
      for (int q = 0; q < kPsolaPer; ++q) {
        const int i = (int)(i0 + (unsigned)(q * kPsolaThreads));
        if (i < g.out_lo || i >= g.out_hi) continue;
        const float u = ((float)(int)((unsigned)i - (unsigned)g.centre) - g.centre_frac) * g.inv_half;
        if (!(fabsf(u) < 1.f)) continue;
        const float w = 0.5f + 0.5f * cospif(u);
        int64_t idx;
        float f;
        psola_source(g, i, idx, f);
        idx = idx < -(int64_t)MX_AUDIO_PAD ? -(int64_t)MX_AUDIO_PAD : (idx > idx_max ? idx_max : idx);
        const float x = (1.f - f) * src[idx] + f * src[idx + 1];
        S[q] += w * x;
        W[q] += w;
      }
    }
    if (last) break;
    __syncthreads();  // the next chunk overwrites recs
  }

#pragma unroll
  for (int q = 0; q < kPsolaPer; ++q) {
    const int64_t i = tile_lo + tid + q * kPsolaThreads;
    if (i >= a.nsamples) continue;
    const float y = W[q] > 0.f ? S[q] / (W[q] > 0.25f ? W[q] : 0.25f) : 0.f;
    if (a.pcm_f32) a.pcm_f32[i] = y;
    if (a.pcm_i16) a.pcm_i16[i] = pcm16_clamped(y);
  }
}

template <class Rec>
hipError_t launch(const PsolaArgsT<Rec> &a, hipStream_t s) {
  if (a.nsamples <= 0) return hipSuccess;
  if (a.nsamples > 0x7fffffffLL || a.ngrains < 0 || a.n < 0) return hipErrorInvalidValue;
  const int64_t blocks = (a.nsamples + kPsolaTile - 1) / kPsolaTile;
  hipLaunchKernelGGL(psola_kernel<Rec>, dim3((unsigned)blocks), dim3(kPsolaThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_psola(const PsolaArgs &a, hipStream_t s) { return launch(a, s); }
hipError_t launch_psola(const PsolaFormantArgs &a, hipStream_t s) { return launch(a, s); }

}  // namespace mx
