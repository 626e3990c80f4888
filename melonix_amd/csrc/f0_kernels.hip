// f0_kernels.hip — BUILD-DEFINED frame-parallel YIN f0 tracker (the reference has no detector: Marker::note comes from
// the mouse, app.cpp:923,937).  Parity is against the build's own definition, restated in f64 by tests/yin_ref.py.
//
// Definition (N = 4096, W = N/2 = 2048, sr the caller's):
//   frame h is centred on sample h*hop: x_j = audio[h*hop - W + j], j = 0..N-1, zeros outside [0, n) (the mx_audio pad)
//   1. d(tau) = sum_{j<W} (x_j - x_{j+tau})^2, tau = 0..W, clamped to >= 0; computed as e0 + e_tau - 2 r(tau) with
//      r the cross-correlation of x[0:W] with x[0:N] (N-point transforms) and e_tau = sum_{j<W} x_{j+tau}^2 (prefix sums)
//   2. d'(0) = 1, d'(tau) = d(tau) * tau / sum_{j=1..tau} d(j); 1 where that sum is 0
//   3. search range tau_min = max(2, floor(sr/fmax)) .. tau_max = min(W-1, ceil(sr/fmin)) (the C-ABI checks it)
//   4. tau* = smallest tau in range with d'(tau) < theta, then step forward while tau+1 <= tau_max and
//      d'(tau+1) < d'(tau); none under theta: argmin of d' over the range, ties to the smallest tau
//   5. parabolic refinement on d at tau*-1, tau*, tau*+1: delta = (d- - d+) / (2 (d- - 2 d0 + d+)) clamped to
//      [-1/2, 1/2], 0 where the denominator is <= 0
//   6. mx_f0 {tau*, tau* + delta, d'(tau*), sqrt(sum_{j<N} x_j^2 / N)}; rms == 0 (every x_j == 0): {0, 0, 1, 0}
//
// One workgroup (Plan<4096,16>: 128 threads, two wavefronts) walks a run of consecutive frames; per frame:
//   the level: x is scaled by 2^-s so that max_j |x_j| lands in [1, 2) (s from the block maximum of the magnitude bits;
//   s = 0 for a frame of zeros or one holding Inf / NaN).  Scaling by a power of two is exact and commutes with every
//   f32 operation below barring under- and overflow, which the fixed binade keeps away: the sum of x^2 lies in
//   [1, 2^14), so a frame's level alone no longer squares its samples to 0 or subnormals (a quiet frame reported
//   silent, d without precision) nor overflows its sums.  A frame is silent exactly when its samples are all zero;
//   tau, period and d' do not depend on the level (2^k x gives the same bits while it is exact in f32); rms is
//   ldexp(rms of the scaled frame, s).  The maximum is reduced at the end of the previous frame, under its last barrier;
//   forward transform of a = x[0:W] zero-padded and of x (stft_core.h's three passes + the real-FFT split, post_cplx),
//   P = conj(A) X in registers, P to LDS in bin order, the inverse split (E + i O from P[c], P[M-c]), the same three
//   passes on its conjugate = the N-point real inverse: r(2m) + i r(2m+1) = conj(out[m]) / (8M) (the split leaves
//   2X, the product 4P, the pre-split 8Z — powers of two);
//   the prefix sums of x^2 and of d: a 32- (16-) element run per thread, a DPP scan over the wavefront, the first
//   wavefront's total added to the second — the same order on every frame, so a frame's record depends on nothing
//   but its samples (bit for bit the same whatever the launch split);
//   the first-under-theta tau, the argmin and the end of the descent: block minima (DPP + one LDS word per wave).
// No atomics.  All LDS images below are padded one word per 32 (16) elements so that a thread's contiguous run sits
// on its own bank.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_walk.h"

namespace mx {
namespace {

using FP = Plan<4096, 16>;
constexpr int kF0N = 4096, kF0W = 2048, kF0M = 2048;
static_assert(kPlan4096E == 16 && FP::T == 128 && FP::R3 == 8, "the f0 tracker runs on Plan<4096,16>");
static_assert(t1_size<FP>() == kF0M, "one spectrum fills the FFT image");

// x^2 / prefix sums: element i at i + i/32 (thread t's 32 elements are 33t .. 33t+31)
__device__ __forceinline__ int sq_idx(int i) { return i + (i >> 5); }
// d / d': element tau at tau + tau/16 (thread t's 16 elements start at 17t + 1)
__device__ __forceinline__ int dd_idx(int i) { return i + (i >> 4); }
constexpr int kSqLen = kF0N + kF0N / 32 + 1;
constexpr int kDdLen = kF0W + kF0W / 16 + 2;
static_assert(kDdLen <= 2 * kF0M, "d fits the FFT image (as floats)");

// max |x| over the thread's 32 samples and then the wavefront, as float bits (|x| orders as its bits; NaN above Inf), to
// the wavefront's word of s_max: the level of the frame that xr holds
__device__ __forceinline__ void wave_absmax_bits(int t, int lane, const cpx (&xr)[FP::E], unsigned *s_max) {
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < FP::E; ++e) {
    const unsigned a = __float_as_uint(xr[e].x) & 0x7fffffffu, b = __float_as_uint(xr[e].y) & 0x7fffffffu;
    m = m > a ? m : a;
    m = m > b ? m : b;
  }
  m = wave_reduce_u32<true>(m);
  if (lane == 0) s_max[t >> 6] = m;
}

// s with 2^s <= |x| < 2^(s+1) for the magnitude bits m of a finite non-zero |x|; 0 for 0, Inf and NaN
__device__ __forceinline__ int level_exp(unsigned m) {
  if (m == 0 || m >= 0x7f800000u) return 0;
  if (m >= 0x00800000u) return (int)(m >> 23) - 127;
  return -118 - __builtin_clz(m);  // subnormal: m 2^-149, top bit 31 - clz(m)
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
  const unsigned hi = wave_reduce_u32<false>((unsigned)(k >> 32));
  const unsigned lo = wave_reduce_u32<false>((unsigned)(k >> 32) == hi ? (unsigned)k : 0xffffffffu);
  return ((unsigned long long)hi << 32) | lo;
}

// Forward real transform (wave_walk.h's passes and split): X[o] = 2 * DFT_N(x)[out_bin(t, o)]; ny (thread 0) =
// 2 * DFT_N(x)[M], the Nyquist bin post() replaces by bin M/2.
__device__ __forceinline__ void f0_forward(int t, bool wave0, const cpx (&Y)[FP::E], cpx (&X)[FP::E], float &ny, cpx *img,
                                           const cpx *ltw2, const cpx (&w3b)[3], cpx ulo0, cpx uhi0) {
  using P = FP;
  cpx v[P::E];
  walk_passes<P>(t, wave0, Y, v, img, ltw2, w3b);
  ny = 2.0f * (v[0].x - v[0].y);  // X[M] = Re Z[0] - Im Z[0] (thread 0's P-butterfly element 0)
  post_split<P>(t, wave0, ulo0, uhi0, v, X);
}

// block minimum of a u64 key over the two wavefronts (slot: two LDS words per call site)
__device__ __forceinline__ unsigned long long block_min_u64(int t, unsigned long long k, unsigned long long *slot) {
  const unsigned long long w = wave_min_u64(k);
  if ((t & 63) == 0) slot[t >> 6] = w;
  __syncthreads();
  const unsigned long long a = slot[0], b = slot[1];
  return a < b ? a : b;
}

// Step 4's descent from tau1 over d' (dp): the first tau >= tau1 that is tau_max or not above d'(tau+1) — each thread over
// its 16 lags, then the block minimum.  The plain pick and every rung of the ladder end here.
__device__ __forceinline__ int descent_end(int t, int tau1, int tmax, const float *dp, unsigned long long *slot) {
  int stop = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int tau = 16 * t + 1 + j;
    if (tau >= tau1 && tau <= tmax && tau < stop) {
      if (tau == tmax || !(dp[dd_idx(tau + 1)] < dp[dd_idx(tau)])) stop = tau;
    }
  }
  return (int)block_min_u64(t, (unsigned long long)(unsigned)stop, slot);
}

// Step 5: tau + the parabolic offset on d at tau-1, tau, tau+1
__device__ __forceinline__ float refined_period(const float *dd, int tau) {
  const float dm = dd[dd_idx(tau - 1)], d0 = dd[dd_idx(tau)], dp = dd[dd_idx(tau + 1)];
  const float den = 2.0f * ((dm - 2.0f * d0) + dp);
  float delta = den > 0.f ? (dm - dp) / den : 0.f;
  delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
  return (float)tau + delta;
}

// step 6's silent frame and the ladder's empty slot
constexpr mx_f0 kSilentF0{0, 0.f, 1.f, 0.f};
constexpr mx_f0_cand kEmptyCand{0, 0.f, 1.f, 0};

// The candidate ladder of frame f (header: "Candidate ladder"), behind the plain pick of the same launch: d in dd, d' in sq,
// both complete and at rest until the frame's last barrier.  Rung 1 is the plain pick wherever something lies under theta;
// where nothing does, rungs 1..3 are empty (theta_k <= theta for them) and the plain pick is the argmin — slot 0's
// fallback when nothing lies under 2 theta either.  So rungs 0, 2 and 3 alone are searched, by the plain pick's two block
// minima each (red: a slot pair per minimum); every branch around a barrier is block-uniform.  Thread k writes slot k
// with the arithmetic of the plain record.
__device__ __forceinline__ void f0_ladder(int t, const F0Args &a, int64_t f, bool under_theta, int tau_s, bool silent,
                                          const float *dd, const float *sq, unsigned long long (*red)[2]) {
  const int tmax = a.tau_max;
  int taus[MX_F0_CANDS];
  taus[1] = under_theta ? tau_s : 0;
  static_for<0, MX_F0_CANDS>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    if (k == 1) return;
    taus[k] = k == 0 ? tau_s : 0;
    if (k > 1 && !under_theta) return;
    const float theta = a.threshold * (k == 0 ? 2.0f : k == 2 ? 0.5f : 0.25f);
    int under = 0x7fffffff;
#pragma unroll
    for (int j = 15; j >= 0; --j) {
      const int tau = 16 * t + 1 + j;
      if (tau >= a.tau_min && tau <= tmax && sq[dd_idx(tau)] < theta) under = tau;
    }
    const unsigned long long umin = block_min_u64(t, (unsigned long long)(unsigned)under, red[k ? 2 * k - 2 : 0]);
    if (umin != 0x7fffffffull) taus[k] = descent_end(t, (int)umin, tmax, sq, red[k ? 2 * k - 1 : 1]);
  });
  if (t < MX_F0_CANDS) {
    const int tk = t == 0 ? taus[0] : t == 1 ? taus[1] : t == 2 ? taus[2] : taus[3];
    bool filled = !silent && tk > 0;
#pragma unroll
    for (int j = 0; j < MX_F0_CANDS - 1; ++j) filled = filled && !(j < t && taus[j] == tk);
    mx_f0_cand c = kEmptyCand;
    if (filled) {
      const float ap = sq[dd_idx(tk)];
      if (__builtin_isfinite(ap)) {
        c.tau = tk;
        c.period = refined_period(dd, tk);
        c.aperiodicity = ap;
        c.cents = (int32_t)rintf(1200.f * log2f((float)a.sample_rate / c.period / 55.f)) + 2400;
      }
    }
    a.cands[f * MX_F0_CANDS + t] = c;
  }
}

// LADDER: the second instantiation — the plain record (where a.out is set) and, behind it, the frame's candidate ladder.
template <bool LADDER>
__global__ __launch_bounds__(FP::T) void f0_yin(const F0Args a) {
  using P = FP;
  __shared__ __attribute__((aligned(16))) float2 img[P::M];       // FFT image; then P in bin order; then d
  __shared__ __attribute__((aligned(16))) float2 ltw2[P::TW2];    // pass-2 twiddles
  __shared__ float sq[kSqLen];                                    // x^2, then its exclusive prefix sums; then d'
  __shared__ float wtot[2];                                       // a scan's first-wavefront total
  __shared__ float s_tot;                                         // sum_{j<N} x_j^2
  __shared__ unsigned s_max[2];                                   // the next frame's max |x| bits, per wavefront
  __shared__ unsigned long long red[3][2];
  float *const dd = reinterpret_cast<float *>(img);
  const int t_ = threadIdx.x;
  const bool wave0 = __builtin_amdgcn_readfirstlane(t_) < 64;
  const int lane = t_ & 63;
  cpx ulo0, uhi0;
  post_bases<P>(t_, a.ubase, ulo0, uhi0);
  cpx w3b[3];
  load_w3_bases<P>(a.tw3, t_ ? t_ : P::NS3 / 2, w3b);
  // e^{+2 pi i c/N} for the thread's points c = t + T e: e^{+2 pi i t/N} (ubase[t] = i e^{-2 pi i t/N} = (sin, cos))
  // times e^{2 pi i e/32} (compile-time)
  const cpx wb = mk(a.ubase[t_].y, a.ubase[t_].x);
  fill_ltw2<P>(t_, a.tw2, ltw2);

  int64_t f0, f1;
  block_run(a.frames_per_block, a.count, f0, f1);
  if (f0 >= f1) return;
  const float *const base = a.audio + MX_AUDIO_PAD - kF0W;
  cpx xr[P::E];
  load_raw<P, false>(t_, xr, base + (a.first_frame + f0) * (int64_t)a.hop);
  wave_absmax_bits(t_, lane, xr, s_max);
  __syncthreads();
  const float theta = a.threshold;
  const int tmin = a.tau_min, tmax = a.tau_max;

  for (int64_t f = f0; f < f1; ++f) {
    int t = t_;
    asm volatile("" : "+v"(t));
    // the level: max |x| in [1, 2) (exact)
    const int lv = __builtin_amdgcn_readfirstlane(level_exp(s_max[0] > s_max[1] ? s_max[0] : s_max[1]));
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      xr[e].x = __builtin_ldexpf(xr[e].x, -lv);
      xr[e].y = __builtin_ldexpf(xr[e].y, -lv);
    }
    // x^2 in sample order (the prefix sums read them after the first transform's barriers)
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const int c2 = 2 * (t + P::T * e);
      sq[sq_idx(c2)] = xr[e].x * xr[e].x;
      sq[sq_idx(c2 + 1)] = xr[e].y * xr[e].y;
    }
    // A = DFT(x[0:W] zero-padded): points c < W/2 are the slots e < E/2
    cpx Y[P::E], A[P::E], X[P::E];
    float nyA, nyX;
#pragma unroll
    for (int e = 0; e < P::E; ++e) Y[e] = e < P::E / 2 ? xr[e] : mk(0.f, 0.f);
    f0_forward(t, wave0, Y, A, nyA, img, ltw2, w3b, ulo0, uhi0);
    // prefix sums of x^2, first half: thread t's run of 32 and the wavefront scan of the runs' totals
    float run = 0.f;
    {
      const float *s = sq + 33 * t;
#pragma unroll
      for (int j = 0; j < 32; ++j) run += s[j];
    }
    const float incl = wave_scan_add(run);
    if (lane == 63) wtot[t >> 6] = incl;
    // X = DFT(x); the next frame's samples travel under the rest of this one
#pragma unroll
    for (int e = 0; e < P::E; ++e) Y[e] = xr[e];
    if (f + 1 < f1) load_raw<P, false>(t, xr, base + (a.first_frame + f + 1) * (int64_t)a.hop);
    f0_forward(t, wave0, Y, X, nyX, img, ltw2, w3b, ulo0, uhi0);
    {  // the exclusive prefix sums in place: sq[i] = sum_{j<i} x_j^2 (wtot[0] is visible: barriers since)
      float acc = incl - run + (wave0 ? 0.f : wtot[0]);
      float *s = sq + 33 * t;
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const float q = s[j];
        s[j] = acc;
        acc += q;
      }
      if (t == P::T - 1) s_tot = acc;
    }
    __syncthreads();  // every wave is past its last read of the image (pass 3's T2 read)
    // P = conj(A) X (= 4 DFT(a)* DFT(x)) in bin order; P[M] (real) stays in thread 0
#pragma unroll
    for (int o = 0; o < P::E; ++o) img[out_bin<P>(t, o)] = cmul(cconj(A[o]), X[o]);
    const float pM = nyA * nyX;
    __syncthreads();
    // inverse split: Z[c] = E + i O, E = P[c] + conj(P[M-c]), O = (P[c] - conj(P[M-c])) e^{2 pi i c/N}; the passes run
    // on conj(Z)
    static_for<0, P::E>([&](auto ee) {
      constexpr int e = decltype(ee)::value;
      const int c = t + P::T * e;
      const cpx pc = img[c];
      cpx pm = img[(P::M - c) & (P::M - 1)];
      if (e == 0 && t == 0) pm = mk(pM, 0.f);
      const cpx w = mulw64<-2 * e>(wb);
      const cpx E2 = mk(pc.x + pm.x, pc.y - pm.y);
      const cpx O2 = cmul(mk(pc.x - pm.x, pc.y + pm.y), w);
      Y[e] = mk(E2.x - O2.y, -(E2.y + O2.x));
    });
    cpx v[P::E];
    walk_passes<P>(t, wave0, Y, v, img, ltw2, w3b);
    __syncthreads();  // the image is free: d goes there
    // d(tau) at the thread's taus 2m, 2m+1 (m = k0 + NS3 r, r(2m) + i r(2m+1) = conj(v) / (8M)), tau <= W
    const float e0 = sq[sq_idx(kF0W)];
    const float etot = s_tot;
    {
      constexpr float sc = 1.0f / (8.0f * kF0M);
      const int kq = t ? P::NS3 - t : P::NS3 / 2;
#pragma unroll
      for (int i = 0; i < P::E; ++i) {
        const int m = i < P::R3 ? t + P::NS3 * i : kq + P::NS3 * ((i - P::R3 - 1) & (P::R3 - 1));
        const float rr[2] = {v[i].x * sc, -v[i].y * sc};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int tau = 2 * m + h;
          if (tau <= kF0W) {
            const float st = sq[sq_idx(tau)];
            const float sw = tau + kF0W < kF0N ? sq[sq_idx(tau + kF0W)] : etot;
            const float d = (e0 + (sw - st)) - 2.0f * rr[h];
            dd[dd_idx(tau)] = d > 0.f ? d : 0.f;
          }
        }
      }
    }
    __syncthreads();
    // cumulative sums of d over tau = 1..W: thread t's run tau = 16t+1 .. 16t+16
    float dv[16];
    float crun = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      dv[j] = dd[dd_idx(16 * t + 1 + j)];
      crun += dv[j];
    }
    const float cinc = wave_scan_add(crun);
    if (lane == 63) wtot[t >> 6] = cinc;
    __syncthreads();
    float cum = cinc - crun + (wave0 ? 0.f : wtot[0]);
    // d' into the prefix-sum image (its sums have been read), the first-under-theta tau and the argmin key of the run
    int under = 0x7fffffff;
    unsigned long long key = ~0ull;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int tau = 16 * t + 1 + j;
      cum += dv[j];
      const float dp = cum == 0.f ? 1.0f : dv[j] * (float)tau / cum;
      sq[dd_idx(tau)] = dp;
      if (tau >= tmin && tau <= tmax) {
        if (dp < theta && tau < under) under = tau;
        const unsigned long long k = ((unsigned long long)__float_as_uint(dp) << 32) | (unsigned)tau;
        key = k < key ? k : key;
      }
    }
    const unsigned long long umin = block_min_u64(t, (unsigned long long)(unsigned)under, red[0]);  // + barrier: d' is complete
    // the end of the descent, or the argmin where nothing lies under theta
    const int tau_s = umin != 0x7fffffffull ? descent_end(t, (int)umin, tmax, sq, red[1]) : (int)(unsigned)block_min_u64(t, key, red[2]);
    if (t == 0) {
      mx_f0 r = kSilentF0;
      if (etot != 0.f) {
        r.tau = tau_s;
        r.period = refined_period(dd, tau_s);
        r.aperiodicity = sq[dd_idx(tau_s)];
        r.rms = __builtin_ldexpf(__builtin_sqrtf(etot * (1.0f / kF0N)), lv);
      }
      if (!LADDER || a.out) a.out[f] = r;
    }
    if constexpr (LADDER) {
      __shared__ unsigned long long lred[6][2];
      f0_ladder(t, a, f, umin != 0x7fffffffull, tau_s, etot == 0.f, dd, sq, lred);
    }
    if (f + 1 < f1) wave_absmax_bits(t, lane, xr, s_max);  // the next frame's level (its samples have long arrived)
    __syncthreads();  // the images are read: the next frame may write them; s_max is written
  }
}

}  // namespace

hipError_t launch_f0(const F0Args &a0, hipStream_t s) {
  if (a0.count <= 0) return hipSuccess;
  F0Args a = a0;
  const dim3 grid = walk_grid(a.count, a.frames_per_block, kPlan4096Run), block(FP::T);
  if (a.cands) hipLaunchKernelGGL(f0_yin<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(f0_yin<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace mx
