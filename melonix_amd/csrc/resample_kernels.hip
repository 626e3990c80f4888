// resample_kernels.hip — BUILD-DEFINED sample-rate conversion (definition: include/melonix_amd.h "Sample-rate conversion";
// resample_core.h holds the arithmetic, tests/emu/resample_emu.cpp runs it on the CPU).  Binary32 without contraction, every sum
// in ascending tap order from +0.f: the bytes are numpy's whatever the tiling or the launch split.
//
// resample_kernel: a workgroup of 256 threads takes a tile of consecutive outputs (rs::tile_outputs: up to 2048, fewer where
// the ratio makes their input window long), stages the window [i(j0) - (H - 1), i(j1) + H] — the aligned quads that cover it,
// 16-byte loads, samples outside the file as zeros — in LDS once, then a lane takes outputs j0 + lane + 256 q, four of them side
// by side (four independent sums hide the latency of one), x from LDS.  The taps are read with a row per tap index, h[k][phi]:
// the 64 lanes of one k touch L consecutive floats, a few cache lines.  Where the whole table fits beside the window
// (kLdsTable: L T floats within 44 KiB — 147/160, 160/147, 1/2, 2/1 and their like) it is staged in LDS too.
// The map from an output to its sample and phase is one 64-bit division per workgroup (rs::at of j0) and one 32-bit division
// per output (rs::at_offset).
// Loads stay inside the padded image (the window reaches at most 255 samples before the file and 256 behind it, far below
// MX_AUDIO_PAD); stores go to out[0 .. count) only.
#include <hip/hip_runtime.h>

#include "image_quads.h"
#include "kernels.h"
#include "resample_core.h"

namespace mx {
namespace {

constexpr int kThreads = 256;
constexpr int kSlots = 4;  // outputs a lane sums side by side
static_assert(rs::kMaxTile % (kSlots * kThreads) == 0, "a full tile is whole rounds of the slots");

template <bool kLdsTable>
__global__ __launch_bounds__(kThreads) void resample_kernel(const float *__restrict__ image, int64_t n, mx_resample_plan p,
                                                             const float *__restrict__ table, int64_t first_out, int64_t count,
                                                             int tile, int win_quads, float *__restrict__ out) {
  extern __shared__ float4 smem[];  // win_quads quads of the window, then (kLdsTable) the table
  const int64_t t0 = (int64_t)blockIdx.x * tile;  // the tile's first output, from first_out
  const int cnt = (int)(count - t0 < tile ? count - t0 : tile);
  const rs::At base = rs::at(first_out + t0, p), last = rs::at_offset(base, cnt - 1, p);
  const int64_t lo = base.i - (p.half - 1), hi = last.i + p.half;  // the window: lo >= -255, hi <= n + 255
  const int64_t q0 = (lo + MX_AUDIO_PAD) >> 2;
  const int nq = (int)(((hi + MX_AUDIO_PAD) >> 2) - q0) + 1;  // <= win_quads (rs::tile_outputs)
  const float4 *img = reinterpret_cast<const float4 *>(image);
  for (int k = threadIdx.x; k < nq && k < win_quads; k += kThreads) smem[k] = load_quad(img, q0 + k, n);
  float *tab = reinterpret_cast<float *>(smem + win_quads);
  if (kLdsTable)
    for (int k = threadIdx.x; k < p.L * p.taps; k += kThreads) tab[k] = table[k];
  __syncthreads();
  const float *x = reinterpret_cast<const float *>(smem);
  const float *h = kLdsTable ? tab : table;
  const int x0 = (int)(lo - (4 * q0 - MX_AUDIO_PAD));  // where sample lo lies in the staged quads: 0 .. 3
  for (int o0 = threadIdx.x; o0 < cnt; o0 += kSlots * kThreads) {
    int xo[kSlots], ho[kSlots];
#pragma unroll
    for (int e = 0; e < kSlots; ++e) {
      const int o = o0 + e * kThreads;
      const rs::At a = rs::at_offset(base, o < cnt ? o : o0, p);  // (a slot past the tile's end repeats the first: nothing stored)
      xo[e] = x0 + (int)(a.i - base.i);
      ho[e] = a.phase;
    }
    float y[kSlots];
    rs::dots<kSlots>(x, xo, h, ho, p.L, p.taps, y);
#pragma unroll
    for (int e = 0; e < kSlots; ++e) {
      const int o = o0 + e * kThreads;
      if (o < cnt) out[t0 + o] = y[e];
    }
  }
}

}  // namespace

hipError_t launch_resample(const ResampleArgs &a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  const mx_resample_plan &p = a.plan;
  const rs::Geometry g = rs::geometry(p);
  const int64_t blocks = (a.count + g.tile - 1) / g.tile;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kThreads);
  const size_t lds = (size_t)g.win_quads * sizeof(float4) + (g.lds_table ? (size_t)p.L * p.taps * sizeof(float) : 0);  // <= rs::kLdsBytes
  if (g.lds_table)
    hipLaunchKernelGGL(resample_kernel<true>, grid, block, lds, s, a.image, a.n, p, a.table, a.first_out, a.count, g.tile, g.win_quads, a.out);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, block, lds, s, a.image, a.n, p, a.table, a.first_out, a.count, g.tile, g.win_quads, a.out);
  return hipGetLastError();
}

}  // namespace mx
