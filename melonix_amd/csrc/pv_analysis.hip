// pv_analysis.hip — the analysis stage of the phase vocoder and its records: pv_analysis, pv_heads, and the
// constant-ratio plan pv_plan_const (the stages: pv_common.h).
#include "pv_common.h"
#include "wave_walk.h"

namespace mx {
namespace {

// arg(re + i im) in turns as an even uint32 (2^-31 turn steps; the float carries 24 bits of it); arg(0, 0) = 0.
// atan(q)/2pi on q = min/max in [0, 1] is an odd polynomial (degree 17, |error| < 2e-8 turn incl. f32 rounding — the
// resolution of the float itself at 1/8 turn), then the octant is undone; no division, no 64-bit conversion.
__device__ __forceinline__ uint32_t to_turns(float re, float im) {
  const float ax = __builtin_fabsf(re), ay = __builtin_fabsf(im);
  const float hi = __builtin_fmaxf(__builtin_fmaxf(ax, ay), 1e-30f), lo = __builtin_fminf(ax, ay);
  const float q = lo * __builtin_amdgcn_rcpf(hi);
  const float z = q * q;
  float p = 3.955824650e-04f;
  p = fma_(p, z, -2.311495831e-03f);
  p = fma_(p, z, 6.365358364e-03f);
  p = fma_(p, z, -1.154612750e-02f);
  p = fma_(p, z, 1.672621258e-02f);
  p = fma_(p, z, -2.254327014e-02f);
  p = fma_(p, z, 3.180934861e-02f);
  p = fma_(p, z, -5.305053294e-02f);
  p = fma_(p, z, 1.591549218e-01f);
  float r = p * q;                  // [0, 1/8]
  r = ay > ax ? 0.25f - r : r;      // [0, 1/4]
  r = re < 0.f ? 0.5f - r : r;      // [0, 1/2]
  r = __builtin_copysignf(r, im);   // (-1/2, 1/2]
  return (uint32_t)(int32_t)__builtin_rintf(r * 2147483648.0f) << 1;  // |r * 2^31| <= 2^30
}

// inc_f[k] = (k*Hs mod N) * 2^32/N + trunc(double(d) * (Hs/h)),  d = int32(P_f[k] - P_{f-1}[k] - (k*h mod N) * 2^32/N)
// (one binary64 product of a binary64 quotient: the same two roundings on every IEEE machine; uint32 wrap = mod 1 turn).
__device__ __forceinline__ uint32_t pv_inc(int k, uint32_t h, double hratio, uint32_t p, uint32_t prev_p) {
  constexpr uint32_t unit = (uint32_t)(4294967296ull / kPvN);
  const uint32_t expect = (((uint32_t)k * h) & (uint32_t)(kPvN - 1)) * unit;
  const int32_t d = (int32_t)(p - prev_p - expect);
  const int64_t q = (int64_t)((double)d * hratio);  // truncates toward zero
  return (((uint32_t)k * (uint32_t)kPvHs) & (uint32_t)(kPvN - 1)) * unit + (uint32_t)q;
}

// The record of one peak of a frame (h, hr: the frame's hop and stretch factor; p: the peak's bin; xc, xq: the frame's and the
// previous frame's spectrum at p; pkq: the previous frame's peak map; thrq: that frame's activity threshold)
__device__ __forceinline__ uint2 pv_make_record(uint32_t h, double hr, int p, float2 xc, float2 xq, const uint32_t *pkq, float thrq,
                                                bool prev_exists) {
  const uint32_t pc_ = to_turns(xc.x, xc.y), pp_ = to_turns(xq.x, xq.y);
  const bool cont = prev_exists && h >= 1 && cnorm2(xq) >= thrq;
  const int q = pv_owner(pkq, p);
  uint2 rec;
  rec.x = (uint32_t)p | (q != (int)kPvNoBin ? ((uint32_t)q << 11) | kRecQValid : 0u) | (cont ? kRecCont : 0u);
  rec.y = pp_ + pv_inc(p, h, hr, pc_, pp_) - pc_;
  return rec;
}

// The peaks of a map (W words, one per lane of the calling wavefront), numbered: their bins in ascending order into `list`,
// their count returned in lane 63 (exclusive scan of the words' populations through the DPP crossbar).
__device__ __forceinline__ int pv_number_peaks(uint32_t w, int lane, uint16_t *list) {
  const int c = __builtin_popcount(w);
  const int inc = wave_scan_add(c);
  uint32_t rest = w;
  int r = inc - c;
  while (rest) {
    const int b = __builtin_ctz(rest);
    rest &= rest - 1;
    list[r++] = (uint16_t)(32 * lane + b);
  }
  return inc;
}

__global__ __launch_bounds__(PV::T) void pv_analysis(const PvArgs a) {
  using P = PV;
  // the M-point image (after the transform it holds X_f in bin order, for the peak search and the row's way to HBM); the
  // pass-2 twiddle table (2 KiB, shared by both waves).  The records of a frame need its spectrum and the previous
  // frame's at its peaks only: they are made ONE FRAME LATER, from the two rows in HBM/L2 (this workgroup wrote them) —
  // the gathers are issued at the top of the next frame's transform and have all of it to arrive.  (A second image for the
  // previous spectrum costs the third wave per SIMD; gathering in the frame's own iteration leaves ~4 us of latency bare.)
  constexpr int kTw2 = ((P::TW2 + 1) / 2) * 2;
  constexpr int W = P::M / 32;  // words of a peak map
  __shared__ __attribute__((aligned(16))) float2 lds[P::M];
  __shared__ __attribute__((aligned(16))) float2 ltw2[kTw2];
  __shared__ uint32_t pkb[3][W + 2];  // the peak maps of frames f, f-1, f-2 (by frame mod 3), a zero word either side
  // the peak bins of a frame, ascending (by frame parity: the first wavefront lists frame f's while the second is still
  // making frame f - 1's records from the other list)
  __shared__ uint16_t plist[2][P::M];
  __shared__ float red[2][2];         // per wavefront: the largest squared magnitude (alternating frames)
  __shared__ uint32_t npk;
  const int t_ = threadIdx.x;
  const bool wave0 = __builtin_amdgcn_readfirstlane(t_) < 64;
  // (the eight post-split twiddles are rebuilt from their base every frame — a rotation by a constant each, stft_core.h
  // PostFly —: held for the whole walk they are the registers between two and three waves per SIMD)
  cpx ulo0, uhi0;
  post_bases<P>(t_, a.ubase, ulo0, uhi0);
  cpx w3b[3];
  load_w3_bases<P>(a.tw3, t_ ? t_ : P::NS3 / 2, w3b);
  for (int i = t_; i < P::TW2; i += P::T) ltw2[i] = a.tw2[i];
  for (int i = t_; i < 3 * (W + 2); i += P::T) (&pkb[0][0])[i] = 0u;
  const unsigned lb = xcd_block(blockIdx.x, gridDim.x);
  const int64_t f0 = (int64_t)lb * a.frames_per_block;
  const int64_t f1 = f0 + a.frames_per_block < a.frames ? f0 + a.frames_per_block : a.frames;
  if (f0 >= f1) return;
  // this workgroup's region of the record pool: its frames' records one behind the other, the first frame's (pv_heads writes
  // them) in front.  rec_run: records of the frames before the one whose offset is being fixed.
  uint2 *const rec_base = a.recs + (size_t)lb * a.rec_wg_cap;
  uint32_t rec_run = 0u;
  // The records of the workgroup's FIRST frame need the previous workgroup's last row, peak map and threshold: pv_heads
  // makes them, behind this kernel (a warm-up transform of frame f0 - 1 in front of every sixteen frames was 6 % of the
  // kernel's time and 0.8 GB of duplicate rows).
  cpx xr[P::E];
  load_raw<P, false>(t_, xr, a.audio + MX_AUDIO_PAD + (a.apos[f0] - P::N / 2));
  // this thread's window values: registers for the whole walk (the kernel runs two waves per SIMD either way; reloaded per
  // frame they were sixteen L1 round trips at the top of every transform)
  cpx hwin[P::E];
#pragma unroll
  for (int e = 0; e < P::E; ++e) hwin[e] = ld_pair<true>(a.hann_scaled, 2 * (t_ + P::T * e));
  __syncthreads();

  // pending: the frame whose peaks are listed in plist (records not yet written)
  int pend_cnt = 0;
  bool pend = false;
  float thr2_1 = 0.f, thr2_2 = 0.f;  // thresholds of frames f-1, f-2
  int m0 = (int)(f0 % 3);            // pkb index of frame f
  int cur = 0;
  for (int64_t f = f0; f < f1; ++f) {
    // as in stft_kernel: re-materialise the thread index and a zero table offset per frame, or LICM hoists every
    // frame-invariant table value and address out of the loop
    int t = t_;
    asm volatile("" : "+v"(t));
    // the pending frame's hop and stretch factor (scalar loads: requested here they return under pass 1)
    const uint32_t ph = a.hop[f > 0 ? f - 1 : 0];
    const double phr = a.hratio[f > 0 ? f - 1 : 0];
    const int m1 = m0 == 0 ? 2 : m0 - 1, m2 = m1 == 0 ? 2 : m1 - 1;  // maps of frames f-1, f-2
    cpx Y[P::E], v[P::E];
#pragma unroll
    for (int e = 0; e < P::E; ++e) Y[e] = pk_mul(xr[e], hwin[e]);
    pass1<P>(Y, v);
    __syncthreads();  // every wave is past the previous frame's peak numbering: plist and npk are complete
    if (pend) pend_cnt = (int)npk;
    // where frame f - 1's records start (f > f0; npk is its count — also for the workgroup's first frame, whose records
    // pv_heads writes): behind those of the frames before it.  A region that does not hold them voids the run.
    uint32_t rec_off = 0u;
    bool rec_fits = true;
    if (f > f0) {
      const uint32_t c1 = npk;
      rec_off = rec_run;
      rec_fits = rec_off + c1 <= a.rec_wg_cap;
      rec_run += c1;
    }
    // the pending frame's (f - 1) first record per thread: its spectrum and the one before at the peak, from their rows
    float2 ga = make_float2(0.f, 0.f), gb = make_float2(0.f, 0.f);
    int gp = 0;
    // (records are the second wavefront's first: the first one numbers the frame's peaks meanwhile)
    const int ti = (t + P::T / 2) & (P::T - 1);
    const uint16_t *pl_pend = plist[(f + 1) & 1];  // frame f - 1's list
    if (pend && ti < pend_cnt) {
      gp = pl_pend[ti];
      ga = a.xrows[(size_t)(f - 1) * P::M + gp];
      if (f >= 2) gb = a.xrows[(size_t)(f - 2) * P::M + gp];
    }
    store_t1<P>(t, v, lds);
    __syncthreads();
    cpx w2[P::R2 - 1];
    load_t1_tw2<P>(t, v, lds, ltw2, w2);
    __syncthreads();
    pass2_reg<P>(v, w2);
    store_t2<P>(t, v, lds);
    __syncthreads();
    load_t2<P>(t, v, lds);
    __syncthreads();  // every wave has its T2 read: the image is free for X_f
    cpx X[P::E];
    {
      cpx w3r[P::R3 - 1];
      root_powers7(w3b, w3r);
      if (wave0) pass3_reg<P, true>(t, v, w3r);
      else pass3_reg<P, false>(t, v, w3r);
      post_split<P>(t, wave0, ulo0, uhi0, v, X);
    }
    // X_f goes into the image in bin order (consecutive lanes hold consecutive bins) — for the peak search and, behind the
    // barrier, for its way to HBM as aligned 16-byte stores, 1 KiB per wavefront instruction; the frame's largest squared
    // magnitude through the DPP crossbar and two LDS words
    float mx2 = 0.f;
#pragma unroll
    for (int o = 0; o < P::E; ++o) {
      const float n2 = cnorm2(X[o]);
      mx2 = n2 > mx2 ? n2 : mx2;
      lds[out_bin<P>(t, o)] = X[o];
    }
    const uint32_t wmax = wave_reduce_u32<true>(__float_as_uint(mx2));  // non-negative floats order like their bit patterns
    if ((t & 63) == 0) red[cur][t >> 6] = __uint_as_float(wmax);
    if (t < W) pkb[m0][t + 1] = 0u;
    __syncthreads();
    // the samples of frame f + 1 are requested here: they travel under the peak search, the records and the numbering
    if (f + 1 < f1) load_raw<P, false>(t, xr, a.audio + MX_AUDIO_PAD + (a.apos[f + 1] - P::N / 2));
    const f32x4 *src = reinterpret_cast<const f32x4 *>(lds) + t;
    f32x4 *dst = reinterpret_cast<f32x4 *>(a.xrows + (size_t)f * P::M) + t;
#pragma unroll
    for (int i = 0; i < P::M / 2 / P::T; ++i) __builtin_nontemporal_store(src[P::T * i], &dst[P::T * i]);
    const float thr2 = kPvActiveRel2 * (red[cur][0] > red[cur][1] ? red[cur][0] : red[cur][1]);
    if (t == 0) a.fthr[f] = thr2;
    // Peaks of the row: active and not below rho times any of its four neighbours (squared magnitudes; bins outside the
    // row never stand in the way).  Thread t looks at bins 4j .. 4j+3, j = t + T i.
#pragma unroll
    for (int i = 0; i < P::M / 4 / P::T; ++i) {
      const int j = t + P::T * i;
      const f32x4 *x4 = reinterpret_cast<const f32x4 *>(lds);  // two bins per 16 bytes
      const f32x4 c0 = x4[2 * j], c1 = x4[2 * j + 1];
      const f32x4 lo = j > 0 ? x4[2 * j - 1] : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 hi = j < P::M / 4 - 1 ? x4[2 * j + 2] : f32x4{0.f, 0.f, 0.f, 0.f};
      const float neg = -1.f;
      const float v8[8] = {j > 0 ? fma_(lo.x, lo.x, lo.y * lo.y) : neg, j > 0 ? fma_(lo.z, lo.z, lo.w * lo.w) : neg,
                           fma_(c0.x, c0.x, c0.y * c0.y),               fma_(c0.z, c0.z, c0.w * c0.w),
                           fma_(c1.x, c1.x, c1.y * c1.y),               fma_(c1.z, c1.z, c1.w * c1.w),
                           j < P::M / 4 - 1 ? fma_(hi.x, hi.x, hi.y * hi.y) : neg,
                           j < P::M / 4 - 1 ? fma_(hi.z, hi.z, hi.w * hi.w) : neg};
      uint32_t nib = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        // c >= rho^2 v for each of the four neighbours <=> c >= rho^2 max(v): rounding is monotone, the decisions are the
        // same ones bit for bit (and a bin outside the row, -1, never wins the maximum over a squared magnitude)
        const float c = v8[b + 2];
        const float nb4 = __builtin_fmaxf(__builtin_fmaxf(v8[b], v8[b + 1]), __builtin_fmaxf(v8[b + 3], v8[b + 4]));
        const bool pk = c >= __builtin_fmaxf(thr2, kPvPeakMargin2 * nb4);
        nib |= pk ? (1u << b) : 0u;
      }
      if (nib) atomicOr(&pkb[m0][1 + (j >> 3)], nib << (4 * (j & 7)));
    }
    __syncthreads();  // this frame's peak map is complete
    // the pending frame's records (one per thread from the registers; a frame with more peaks than threads gathers the
    // rest here): the second wavefront's lanes first — the first one has this frame's peaks to number
    if (pend && rec_fits) {
      uint2 *rrow = rec_base + rec_off;
      const float2 *xa = a.xrows + (size_t)(f - 1) * P::M, *xb = a.xrows + (size_t)(f >= 2 ? f - 2 : 0) * P::M;
      for (int i = ti; i < pend_cnt; i += P::T) {
        if (i != ti) {
          gp = pl_pend[i];
          ga = xa[gp];
          gb = f >= 2 ? xb[gp] : make_float2(0.f, 0.f);
        }
        rrow[i] = pv_make_record(ph, phr, gp, ga, gb, &pkb[m2][1], thr2_2, f >= 2);
      }
    }
    // the first wavefront numbers this frame's peaks (exclusive scan of the words' populations through the DPP crossbar)
    // and lists their bins in ascending order
    if (wave0) {
      const uint32_t w = pkb[m0][1 + t];  // W == 64: one word per lane
      const int inc = pv_number_peaks(w, t, plist[f & 1]);
      if (t == 63) npk = (uint32_t)inc;
      a.pkmap[(size_t)f * W + t] = w;
      if (t == 63) {
        // count and place of this frame's records (rec_run: the records of the workgroup's frames before it); a frame that
        // does not fit its region is placed at the region's front — in bounds — and voids the run
        const bool fits = rec_run + (uint32_t)inc <= a.rec_wg_cap;
        a.pkcount[f] = (uint32_t)inc | ((fits ? rec_run : 0u) << kPkOffShift);
        if (!fits) *a.rec_overflow = 1u;
      }
    }
    pend = f > f0;  // (the first frame's records are pv_heads')
    thr2_2 = thr2_1;
    thr2_1 = thr2;
    m0 = m0 == 2 ? 0 : m0 + 1;
    cur ^= 1;
  }
  __syncthreads();
  pend_cnt = (int)npk;
  // the last frame's records: no next transform to hide the gathers under (a one-frame workgroup's are pv_heads')
  const bool last_fits = rec_run + (uint32_t)pend_cnt <= a.rec_wg_cap;
  if (f1 - 1 > f0 && last_fits) {
    const int64_t fl = f1 - 1;
    const int m1 = m0 == 0 ? 2 : m0 - 1, m2 = m1 == 0 ? 2 : m1 - 1;  // m1: frame fl's map, m2: frame fl - 1's
    uint2 *rrow = rec_base + rec_run;
    const float2 *xa = a.xrows + (size_t)fl * P::M, *xb = a.xrows + (size_t)(fl >= 1 ? fl - 1 : 0) * P::M;
    const uint32_t lh = a.hop[fl];
    const double lhr = a.hratio[fl];
    for (int i = t_; i < pend_cnt; i += P::T) {
      const int p = plist[fl & 1][i];
      rrow[i] = pv_make_record(lh, lhr, p, xa[p], fl >= 1 ? xb[p] : make_float2(0.f, 0.f), &pkb[m2][1], thr2_2, fl >= 1);
    }
  }
}

// The records of every analysis workgroup's first frame f (a multiple of the run length): the frame's peaks from its map,
// its spectrum and the previous frame's at the peaks from their rows, the previous frame's map and threshold — everything
// pv_analysis left in memory.  One workgroup per such frame.
__global__ __launch_bounds__(PV::T) void pv_heads(const PvArgs a) {
  MX_LATENCY_BOUND_KERNEL();
  using P = PV;
  constexpr int W = P::M / 32;
  __shared__ uint32_t pkq[W + 2];  // the previous frame's map, a zero word either side
  __shared__ uint16_t plist[P::M];
  __shared__ uint32_t npk;
  const int t = threadIdx.x;
  const int64_t f = (int64_t)blockIdx.x * a.frames_per_block;
  if (f >= a.frames) return;
  if (t < W + 2) pkq[t] = (f >= 1 && t >= 1 && t <= W) ? a.pkmap[(size_t)(f - 1) * W + (t - 1)] : 0u;
  if (t < 64) {
    const int inc = pv_number_peaks(a.pkmap[(size_t)f * W + t], t, plist);
    if (t == 63) npk = (uint32_t)inc;
  }
  __syncthreads();
  const int cnt = (int)npk;
  const uint32_t h = a.hop[f];
  const double hr = a.hratio[f];
  const float thrq = f >= 1 ? a.fthr[f - 1] : 0.f;
  uint2 *rrow = a.recs + pv_rec_start(a, f, a.pkcount[f]);  // (the front of its analysis workgroup's region)
  const float2 *xa = a.xrows + (size_t)f * P::M, *xb = a.xrows + (size_t)(f >= 1 ? f - 1 : 0) * P::M;
  for (int i = t; i < cnt; i += P::T) {
    const int p = plist[i];
    rrow[i] = pv_make_record(h, hr, p, xa[p], f >= 1 ? xb[p] : make_float2(0.f, 0.f), &pkq[1], thrq, f >= 1);
  }
}

// The constant-ratio plan, on the device (binary64 division and floor are exact IEEE operations here as on the host:
// a_f = floor(double(f*Hs) / r), h_f = a_f - a_{f-1}, Hs / h_f).  Row j is global frame fbase + j; row 0 gets hop 0.
__global__ __launch_bounds__(256) void pv_plan_const(int64_t *apos, uint32_t *hop, double *hratio, int64_t rows,
                                                     int64_t fbase, double r) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= rows) return;
  const int64_t aj = (int64_t)floor((double)((fbase + j) * kPvHs) / r);
  apos[j] = aj;
  uint32_t h = 0u;
  double q = 0.0;
  if (j > 0) {
    const int64_t d = aj - (int64_t)floor((double)((fbase + j - 1) * kPvHs) / r);
    if (d >= 1 && d <= 0x7fffffffLL) {
      h = (uint32_t)d;
      q = (double)kPvHs / (double)d;
    }
  }
  hop[j] = h;
  hratio[j] = q;
}

// The frames cut into runs of frames_per_block, one workgroup of pv_analysis per run and one of pv_heads per run's first
// frame: the default run and the number of runs.
// (8 / 12 / 16 / 24 frames per workgroup: 4.80 / 4.78 / 4.80 / 4.81 ms per 60 min in one launch — flat since the warm-up frame went)
unsigned pv_cut_runs(PvArgs &a) {
  if (a.frames_per_block <= 0) a.frames_per_block = 16;
  return (unsigned)((a.frames + a.frames_per_block - 1) / a.frames_per_block);
}
}  // namespace

hipError_t launch_pv_plan_const(int64_t *apos, uint32_t *hop, double *hratio, int64_t rows, int64_t fbase, double r,
                                hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(pv_plan_const, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, apos, hop, hratio, rows, fbase, r);
  return hipGetLastError();
}

hipError_t launch_pv_analysis(const PvArgs &a0, hipStream_t s) {
  PvArgs a = a0;
  if (a.frames - a.first <= 0) return hipSuccess;
  const unsigned fb = pv_cut_runs(a);
  hipLaunchKernelGGL(pv_analysis, dim3(fb), dim3(PV::T), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_pv_heads(const PvArgs &a0, hipStream_t s) {
  PvArgs a = a0;
  const unsigned fb = pv_cut_runs(a);
  hipLaunchKernelGGL(pv_heads, dim3(fb), dim3(PV::T), 0, s, a);
  return hipGetLastError();
}

}  // namespace mx
