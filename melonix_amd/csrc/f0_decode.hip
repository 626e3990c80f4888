// f0_decode.hip — BUILD-DEFINED Viterbi decode over the YIN candidate ladder (f0_kernels.hip), exact and parallel.  The
// definition is the header's ("Decoder"); tests/f0_decode_ref.py restates it in Python integers.
//
// The recurrence V_f = V_{f-1} (x) M_f, M_f(i, j) = T_f(i, j) + O_f(j), is a product of 5 x 5 matrices over (min, +).  All
// costs are integers, so the product is associative exactly and every grouping gives the serial V_f bit for bit — the
// trick of the phase scan in pv_lock.hip.  Frame 0 fits the same form with T_0 = 0 and zeros before it.  In chunks of C:
//   f0_dec_products  a thread per (chunk, row i): the walk from the unit row e_i (0 at i, "no path" elsewhere) through the
//                    chunk's frames = row i of the chunk's product                                          C steps
//   f0_dec_starts    one thread over the chunk products (staged through LDS by its block): V before every chunk's first
//                    frame, left in the product's first row                                           count / C steps
//   f0_dec_walk      a thread per chunk re-walks from that V: bp_f (5 x 3 bits a frame), the chunk's map (state at its
//                    last frame -> state before its first; bp composed on the way) and the last chunk's V      C steps
//   f0_dec_ends      one thread over the chunk maps from the end state: the path's state at every chunk's last frame,
//                    left in the map's word                                                           count / C steps
//   f0_dec_path      a thread per chunk walks bp back from that state and writes the records and states       C steps
// No dependent chain grows like count: with C ~ sqrt(count) / 3 none is longer than 3 sqrt(count) steps.  No atomics; every word of
// scratch is written by one thread and read after the launch that wrote it.
// Sizes: an entry is a sum of real costs (< count * 2^27 < 2^58 for any count the frame indexing allows) plus at most one INF
// = 2^56 (a path may end in an empty slot, never pass through one: unvoiced is always open) or the start row's 2^60.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace mx {
namespace {

constexpr int kStates = MX_F0_CANDS + 1;
constexpr int kUnvoiced = MX_F0_CANDS;
constexpr int64_t kQ = 65536, kInf = (int64_t)1 << 56, kNoPath = (int64_t)1 << 60;
constexpr int kDecT = 256;
constexpr int kProdTile = 256;   // chunk products per LDS tile of f0_dec_starts (50 KiB)
constexpr int kMapTile = 4096;   // chunk maps per LDS tile of f0_dec_ends

// The scratch layout, owned here.  prod holds kProdWords int64 per chunk: the chunk's product row-major, as f0_dec_products
// leaves it; from f0_dec_starts on, its first row is V before the chunk's first frame, and behind the last chunk's f0_dec_walk
// leaves V_{F-1}.  bp: a word per frame; map: a word per chunk.
constexpr int kProdWords = kStates * kStates;
__device__ __forceinline__ int64_t *prod_row(const F0DecodeArgs &a, int64_t c, int row) {
  return a.prod + c * kProdWords + row * kStates;
}
__device__ __forceinline__ int64_t *start_vec(const F0DecodeArgs &a, int64_t c) { return prod_row(a, c, 0); }
__device__ __forceinline__ int64_t *end_vec(const F0DecodeArgs &a, int64_t nchunks) { return prod_row(a, nchunks - 1, 1); }
__host__ __device__ constexpr int64_t chunk_count(int64_t count, int64_t chunk) { return (count + chunk - 1) / chunk; }

// chunk c's frames [fa, fb)
__device__ __forceinline__ void chunk_bounds(const F0DecodeArgs &a, int64_t c, int64_t &fa, int64_t &fb) {
  fa = c * a.chunk;
  fb = fa + a.chunk < a.count ? fa + a.chunk : a.count;
}

// The min-plus step: min over the predecessors i of V[i] + cost(i) and, in bi, the lowest i attaining it — the first strictly
// smaller value wins, the unvoiced state is compared last.
template <class Cost>
__device__ __forceinline__ int64_t best_pred(const int64_t (&V)[kStates], unsigned &bi, Cost &&cost) {
  int64_t best = V[0] + cost(0);
  bi = 0;
#pragma unroll
  for (int i = 1; i < kStates; ++i) {
    const int64_t v = V[i] + cost(i);
    if (v < best) {
      best = v;
      bi = i;
    }
  }
  return best;
}

struct DecFrame {
  int32_t cents[MX_F0_CANDS];
  unsigned filled;  // bit j: slot j holds a candidate
  int64_t obs[kStates];
};

__device__ __forceinline__ void load_frame(const F0DecodeArgs &a, int64_t f, DecFrame &fr) {
  fr.filled = 0;
#pragma unroll
  for (int j = 0; j < MX_F0_CANDS; ++j) {
    const mx_f0_cand c = a.cands[f * MX_F0_CANDS + j];
    const bool on = c.tau > 0;
    const float ap = c.aperiodicity;
    fr.filled |= (unsigned)on << j;
    fr.cents[j] = c.cents;
    // min(q(ap), 2Q), at least 0; 2Q for a NaN.  ap * Q is exact below 2
    const int64_t o = !(ap < 2.0f) ? 2 * kQ : ap > 0.f ? (int64_t)rintf(ap * 65536.0f) : 0;
    fr.obs[j] = on ? o : kInf;
  }
  fr.obs[kUnvoiced] = a.q_unvoiced;
}

// V <- V (x) M_f from the frames f-1 (p) and f (c); first: f is frame 0 (T = 0, p is not read).  -> bp_f, 3 bits per state.
__device__ __forceinline__ unsigned dec_step(const F0DecodeArgs &a, int64_t (&V)[kStates], const DecFrame &p, const DecFrame &c,
                                             bool first) {
  const int64_t qs = first ? 0 : a.q_switch;
  const unsigned pf = first ? 0u : p.filled;
  int64_t Vn[kStates];
  unsigned bp = 0, bi;
#pragma unroll
  for (int j = 0; j < MX_F0_CANDS; ++j) {
    const int64_t best = best_pred(V, bi, [&](int i) -> int64_t {
      if (i == kUnvoiced) return qs;
      int64_t t = 0;
      if ((pf >> i & 1u) && (c.filled >> j & 1u)) {
        const int32_t x = c.cents[j], y = p.cents[i];
        int64_t dc = (uint32_t)(x > y ? x : y) - (uint32_t)(x < y ? x : y);  // |x - y|: fits 32 bits unsigned
        dc = dc < a.max_jump_cents ? dc : a.max_jump_cents;
        t = (int64_t)((uint64_t)(a.q_jump * dc) / 100u);
      }
      return t;
    });
    Vn[j] = best + c.obs[j];
    bp |= bi << (3 * j);
  }
  Vn[kUnvoiced] = best_pred(V, bi, [&](int i) { return i == kUnvoiced ? (int64_t)0 : qs; }) + c.obs[kUnvoiced];
  bp |= bi << (3 * kUnvoiced);
#pragma unroll
  for (int j = 0; j < kStates; ++j) V[j] = Vn[j];
  return bp;
}

// The walk over frames [fa, fb) from V; KEEP: bp_f to a.bp and the composed map returned (identity for an empty walk).
template <bool KEEP>
__device__ __forceinline__ unsigned dec_walk(const F0DecodeArgs &a, int64_t fa, int64_t fb, int64_t (&V)[kStates]) {
  DecFrame prev{}, cur;
  if (fa > 0) load_frame(a, fa - 1, prev);
  unsigned map = 0 | 1 << 3 | 2 << 6 | 3 << 9 | 4 << 12;
  for (int64_t f = fa; f < fb; ++f) {
    load_frame(a, f, cur);
    const unsigned bp = dec_step(a, V, prev, cur, f == 0);
    if (KEEP) {
      a.bp[f] = (uint16_t)bp;
      unsigned m = 0;
#pragma unroll
      for (int j = 0; j < kStates; ++j) m |= (map >> (3 * (bp >> (3 * j) & 7u)) & 7u) << (3 * j);
      map = m;
    }
    prev = cur;
  }
  return map;
}

__global__ __launch_bounds__(kDecT) void f0_dec_products(const F0DecodeArgs a, int64_t nchunks) {
  const int64_t g = (int64_t)blockIdx.x * kDecT + threadIdx.x;
  const int64_t c = g / kStates;
  const int row = (int)(g - c * kStates);
  if (c >= nchunks) return;
  int64_t fa, fb;
  chunk_bounds(a, c, fa, fb);
  int64_t V[kStates];
#pragma unroll
  for (int j = 0; j < kStates; ++j) V[j] = j == row ? 0 : kNoPath;
  dec_walk<false>(a, fa, fb, V);
#pragma unroll
  for (int j = 0; j < kStates; ++j) prod_row(a, c, row)[j] = V[j];
}

__global__ __launch_bounds__(kDecT) void f0_dec_starts(const F0DecodeArgs a, int64_t nchunks) {
  __shared__ int64_t tile[kProdTile * kProdWords];
  int64_t V[kStates] = {0, 0, 0, 0, 0};
  for (int64_t c0 = 0; c0 < nchunks; c0 += kProdTile) {
    const int n = (int)(nchunks - c0 < kProdTile ? nchunks - c0 : kProdTile);
    for (int i = threadIdx.x; i < n * kProdWords; i += kDecT) tile[i] = prod_row(a, c0, 0)[i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 0; k < n; ++k) {
        const int64_t *P = tile + k * kProdWords;
        int64_t Vn[kStates];
        unsigned bi;
#pragma unroll
        for (int j = 0; j < kStates; ++j) {
          start_vec(a, c0 + k)[j] = V[j];
          Vn[j] = best_pred(V, bi, [&](int i) { return P[i * kStates + j]; });
        }
#pragma unroll
        for (int j = 0; j < kStates; ++j) V[j] = Vn[j];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kDecT) void f0_dec_walk(const F0DecodeArgs a, int64_t nchunks) {
  const int64_t c = (int64_t)blockIdx.x * kDecT + threadIdx.x;
  if (c >= nchunks) return;
  int64_t fa, fb;
  chunk_bounds(a, c, fa, fb);
  int64_t V[kStates];
#pragma unroll
  for (int j = 0; j < kStates; ++j) V[j] = start_vec(a, c)[j];
  a.map[c] = (uint16_t)dec_walk<true>(a, fa, fb, V);
  if (c == nchunks - 1) {
#pragma unroll
    for (int j = 0; j < kStates; ++j) end_vec(a, nchunks)[j] = V[j];
  }
}

__global__ __launch_bounds__(kDecT) void f0_dec_ends(const F0DecodeArgs a, int64_t nchunks) {
  __shared__ uint16_t tile[kMapTile];
  unsigned s = 0;
  if (threadIdx.x == 0) {  // the lowest j attaining min V_{F-1}
    const int64_t *V = end_vec(a, nchunks);
    int64_t best = V[0];
    for (int j = 1; j < kStates; ++j)
      if (V[j] < best) {
        best = V[j];
        s = j;
      }
  }
  for (int64_t c1 = nchunks; c1 > 0; c1 -= kMapTile) {
    const int64_t c0 = c1 > kMapTile ? c1 - kMapTile : 0;
    const int n = (int)(c1 - c0);
    for (int i = threadIdx.x; i < n; i += kDecT) tile[i] = a.map[c0 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = n - 1; k >= 0; --k) {
        const unsigned m = tile[k];
        a.map[c0 + k] = (uint16_t)s;
        s = m >> (3 * s) & 7u;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kDecT) void f0_dec_path(const F0DecodeArgs a, int64_t nchunks) {
  const int64_t c = (int64_t)blockIdx.x * kDecT + threadIdx.x;
  if (c >= nchunks) return;
  int64_t fa, fb;
  chunk_bounds(a, c, fa, fb);
  unsigned s = a.map[c];
  for (int64_t f = fb - 1; f >= fa; --f) {
    mx_f0 r{0, 0.f, 1.f, a.track[f].rms};  // unvoiced (rms read before the write below: out may be track)
    if (s != kUnvoiced) {
      const mx_f0_cand k = a.cands[f * MX_F0_CANDS + s];
      r.tau = k.tau;
      r.period = k.period;
      r.aperiodicity = k.aperiodicity;
    }
    a.out[f] = r;
    if (a.state) a.state[f] = (uint8_t)s;
    s = a.bp[f] >> (3 * s) & 7u;
  }
}

}  // namespace

// sqrt(count) / 3, at least 32: a chunk's frame costs the three per-chunk walks about nine times what a chunk costs the two
// passes over the chunks (measured over the hour: chunks of 64 / 256 / 1024 / 4096 frames take 4.2 / 2.0 / 4.4 / 14.1 ms)
int64_t f0_decode_default_chunk(int64_t count) {
  int64_t c = 32;
  while (9 * c * c < count) ++c;
  return c;
}

F0DecodeScratch f0_decode_scratch(int64_t count, int64_t chunk) {
  const size_t nchunks = (size_t)chunk_count(count, chunk);
  return {(size_t)count * sizeof(uint16_t), nchunks * kProdWords * sizeof(int64_t), nchunks * sizeof(uint16_t)};
}

hipError_t launch_f0_decode(const F0DecodeArgs &a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  const int64_t nchunks = chunk_count(a.count, a.chunk);
  const dim3 per_chunk((unsigned)((nchunks + kDecT - 1) / kDecT));
  hipLaunchKernelGGL(f0_dec_products, dim3((unsigned)((nchunks * kStates + kDecT - 1) / kDecT)), dim3(kDecT), 0, s, a, nchunks);
  hipLaunchKernelGGL(f0_dec_starts, dim3(1), dim3(kDecT), 0, s, a, nchunks);
  hipLaunchKernelGGL(f0_dec_walk, per_chunk, dim3(kDecT), 0, s, a, nchunks);
  hipLaunchKernelGGL(f0_dec_ends, dim3(1), dim3(kDecT), 0, s, a, nchunks);
  hipLaunchKernelGGL(f0_dec_path, per_chunk, dim3(kDecT), 0, s, a, nchunks);
  return hipGetLastError();
}

}  // namespace mx
