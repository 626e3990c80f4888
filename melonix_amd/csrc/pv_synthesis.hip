// pv_synthesis.hip — synthesis, boundary fix-up and resampling of the phase vocoder: pv_synthesis, pv_fixup, pv_resample,
// pv_resample_frames, pv_edge_sum, and the launchers that compose the stages (the stages: pv_common.h).
#include "pcm16.h"
#include "pv_common.h"
#include "wave_walk.h"

namespace mx {
namespace {

// The phasor of a peak offset: e^{2 pi i C / 2^32} (v_sin_f32 / v_cos_f32 take their argument in turns; C = 0 gives (1, 0)
// exactly, and multiplying by it leaves a coefficient bit for bit as it was).
__device__ __forceinline__ cpx pv_phasor(uint32_t c) {
  const float turns = (float)(int32_t)c * 2.3283064365386963e-10f;  // [-1/2, 1/2)
  return mk(__builtin_amdgcn_cosf(turns), __builtin_amdgcn_sinf(turns));
}

// y[j] = sum_{k<N} Yhat[k] e^{+2 pi i jk/N} (Hermitian extension, real).  Packed z[m] = y[2m] + i y[2m+1] is
// 2*conj(DFT_M(conj Z')) with Z'[c] = (A+B)/2 + i e^{+2 pi i c/N} (A-B)/2, A = Yhat[c], B = conj(Yhat[M-c]):
// the forward passes of stft_core.h run on G[c] = conj((A+B) + i w_c (A-B)) and the frame is conj of the result.
__device__ constexpr float kW32[16][2] = {{1.000000000f, 0.000000000f}, {0.980785280f, 0.195090322f}, {0.923879533f, 0.382683432f}, {0.831469612f, 0.555570233f}, {0.707106781f, 0.707106781f}, {0.555570233f, 0.831469612f}, {0.382683432f, 0.923879533f}, {0.195090322f, 0.980785280f}, {0.000000000f, 1.000000000f}, {-0.195090322f, 0.980785280f}, {-0.382683432f, 0.923879533f}, {-0.555570233f, 0.831469612f}, {-0.707106781f, 0.707106781f}, {-0.831469612f, 0.555570233f}, {-0.923879533f, 0.382683432f}, {-0.980785280f, 0.195090322f}};  // e^{2 pi i e/32}

__global__ __launch_bounds__(PV::T) __attribute__((amdgpu_waves_per_eu(2, 2))) void pv_synthesis(const PvArgs a) {
  using P = PV;
  __shared__ __attribute__((aligned(16))) float2 lds[t1_size<P>()];
  // cd[k]: the synthesis offset C of bin k's owner peak in the frame whose coefficients are formed next (0: the bin rides
  // on no peak, or on one that restarted — it keeps its analysis phase).  Written for frame f + 1 between the barriers of
  // frame f's transform (zeroed after the first, the peaks' intervals filled in after the second), so the lock costs the
  // walk no barrier of its own.
  __shared__ __attribute__((aligned(16))) uint32_t cd[P::M];
  // the next frame's spectrum X (its row, in bin order): requested as LDS-DMA a whole frame ahead — no registers, 1 KiB per
  // wavefront instruction — instead of 32 eight-byte loads per thread that sat in 64 registers through the last pass
  __shared__ __attribute__((aligned(16))) float2 xbuf[P::M];
  const int t_ = threadIdx.x;
  const int64_t nb = pv_blocks(a.frames - a.first);
  const int64_t blk = blockIdx.x;
  const int64_t f0 = a.first + blk * kPvBlockFrames;  // local frame indices; s[0] belongs to local frame a.first
  const int64_t f1 = blk == nb - 1 ? a.frames : f0 + kPvBlockFrames;
  // The overlap-add accumulator lives in registers.  The last pass runs on the columns t and t + NS3/2 (not the forward
  // transform's t and NS3 - t: nothing is split afterwards), so this thread's sample pairs of a frame are m = t + T j,
  // j = 0..15 — a set that a shift by one hop (T pairs) maps onto itself: pair j of frame f and pair j - 1 of frame f + 1
  // are the same output samples.  acc[j]: the sum so far at this frame's pair j + 1; pair 0 leaves with every frame.
  constexpr int kOla = P::N / kPvHs;  // 16 frames reach a sample
  static_assert(kOla == 2 * P::R3 && kPvHs == 2 * P::T, "one hop = one sample pair per thread");
  cpx acc[kOla - 1];
#pragma unroll
  for (int j = 0; j < kOla - 1; ++j) acc[j] = mk(0.f, 0.f);
  // Every continuing peak of frame `fr` claims its bins in cd: from the midpoint to its lower neighbour (a tie goes to
  // the lower peak) up to the midpoint to its upper neighbour, at most kPvReach either side.  A peak is served by
  // G = 2^lg lanes (as many as the frame's peak count leaves: a sweep's handful of peaks are 65-bin intervals, music's
  // hundreds are short).  The first round's records arrive as arguments (requested a frame earlier).
  auto lanes_per_peak = [](int cnt) { return cnt <= 8 ? 4 : cnt <= 16 ? 3 : cnt <= 32 ? 2 : cnt <= 64 ? 1 : 0; };
  // (`info`: the frame's pkcount word — its peak count and where its records start)
  auto fill_cd = [&](int64_t fr, uint32_t info, int tt, uint32_t r_i, uint32_t cv, uint32_t r_m, uint32_t r_n) {
    const int cnt = (int)(info & kPkCountMask);
    const int lg = lanes_per_peak(cnt), G = 1 << lg, sub = tt & (G - 1);
    const uint2 *rrow = a.recs + pv_rec_start(a, fr, info);
    bool first = true;
    for (int i = tt >> lg; i < cnt; i += P::T >> lg) {
      if (!first) {
        const uint2 rc = rrow[i];
        r_i = rc.x;
        cv = rc.y;
        r_m = i > 0 ? rrow[i - 1].x : 0u;
        r_n = i + 1 < cnt ? rrow[i + 1].x : 0u;
      }
      first = false;
      if (!(r_i & kRecCont) || cv == 0u) continue;  // restarted (or an offset of exactly 0): nothing to write
      const int p = (int)(r_i & 2047u);
      const int pm = i > 0 ? (int)(r_m & 2047u) : -(1 << 14), pn = i + 1 < cnt ? (int)(r_n & 2047u) : (1 << 14);
      int lo = ((pm + p) >> 1) + 1, hi = (p + pn) >> 1;  // (pm + p may be negative: arithmetic shift = floor)
      lo = lo < p - kPvReach ? p - kPvReach : lo;
      hi = hi > p + kPvReach ? p + kPvReach : hi;
      lo = lo < 0 ? 0 : lo;
      hi = hi > P::M - 1 ? P::M - 1 : hi;
      for (int k = lo + sub; k <= hi; k += G) cd[k] = cv;
    }
  };
  // (a peak's record, its offset and its neighbours' records — their bins bound its interval —: all requested a frame ahead;
  // read when the interval is written they were L2 round trips in front of a barrier the other wavefront was waiting at)
  auto fetch_fill = [&](int64_t fr, uint32_t info, int tt, uint32_t &r_i, uint32_t &cv, uint32_t &r_m, uint32_t &r_n) {
    const int cnt = (int)(info & kPkCountMask);
    const int i = tt >> lanes_per_peak(cnt);
    r_i = cv = r_m = r_n = 0u;
    if (i < cnt) {
      const uint2 *rrow = a.recs + pv_rec_start(a, fr, info);
      const uint2 rc = rrow[i];
      r_i = rc.x;
      cv = rc.y;
      if (i > 0) r_m = rrow[i - 1].x;
      if (i + 1 < cnt) r_n = rrow[i + 1].x;
    }
  };
  auto zero_cd = [&](int tt) {
#pragma unroll
    for (int j = 0; j < P::M / 4 / P::T; ++j) reinterpret_cast<u32x4 *>(cd)[tt + P::T * j] = u32x4{0u, 0u, 0u, 0u};
  };
  // The row of frame fr -> xbuf: every wavefront moves 1 KiB per instruction (lane l: 16 bytes at l * 16 of the piece; the
  // LDS side of an LDS-DMA load is wave-uniform base + lane * 16), 8 pieces each.  hipcc does not know of these loads: the
  // wave that issued them waits (vmcnt(0)) in front of the barrier behind which anybody reads xbuf.
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t xbuf_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_addr(xbuf) + (uint32_t)(t_ >> 6) * 1024u));
#else
  const uint32_t xbuf_w = 0u;  // (the host pass only parses the kernel)
#endif
  auto request_row = [&](int64_t fr, int tt) {
    const char *src = reinterpret_cast<const char *>(a.xrows + (size_t)fr * P::M) + (tt >> 6) * 1024 + (tt & 63) * 16;
#pragma unroll
    for (int i = 0; i < P::M * 8 / (P::T * 16); ++i) {
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(src + i * (P::T * 16)), "s"(xbuf_w + (uint32_t)i * (P::T * 16))
                   : "memory");
    }
  };
  auto row_landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
  // this thread's window values at its sample pairs m = t + T j: registers for the whole walk
  float2 hw[P::N / kPvHs];
  {
    const float2 *w2 = reinterpret_cast<const float2 *>(a.hann);
#pragma unroll
    for (int j = 0; j < P::N / kPvHs; ++j) hw[j] = w2[t_ + P::T * j];
  }
  // (peak counts of frames f + 1, f + 2: loaded through an index the compiler cannot prove uniform, so that they stay in
  // vector registers — as wave-uniform values hipcc moves them to a scalar register the moment they are requested, behind
  // an s_waitcnt vmcnt(0) at the top of every frame)
  int lane0;
  asm volatile("v_mov_b32 %0, 0" : "=v"(lane0));
  uint32_t cnt1 = 0u, cnt2 = 0u;  // (the pkcount words of frames f + 1, f + 2)
  if (f0 < f1) {
    request_row(f0, t_);
    zero_cd(t_);
    uint32_t r_i, cv, r_m, r_n;
    const uint32_t cnt0 = a.pkcount[f0];
    fetch_fill(f0, cnt0, t_, r_i, cv, r_m, r_n);
    cnt1 = f0 + 1 < f1 ? a.pkcount[f0 + 1 + lane0] : 0u;
    __syncthreads();
    fill_cd(f0, cnt0, t_, r_i, cv, r_m, r_n);
    row_landed();
    __syncthreads();
  }
  const cpx wbase0 = a.wsplit[t_];  // e^{+2 pi i t/N}
  // The pass twiddles of this thread are powers of one root each: gamma^r (pass 2, r = 1..15) and delta^r (pass 3,
  // r = 1..7).  The powers 1, 2, 4 (, 8) stay in registers for the whole walk, the others are one packed product each per
  // frame: a table read per twiddle and frame — 22 L2 round trips in front of the two passes — was latency nothing hid.
  cpx g2b[3], g2o, g3p[3], g3q[3];
  {
    const int k = t_ & (P::R1 - 1);
    g2b[0] = a.tw2[0 * P::R1 + k];
    g2b[1] = a.tw2[1 * P::R1 + k];
    g2b[2] = a.tw2[3 * P::R1 + k];
    g2o = a.tw2[7 * P::R1 + k];
    load_w3_bases<P>(a.tw3, t_, g3p);
    load_w3_bases<P>(a.tw3, t_ + P::NS3 / 2, g3q);
  }
  for (int64_t f = f0; f < f1; ++f) {
    const int t = t_;
    // (the sixteen products wbase * e^{2 pi i e/32} are rebuilt per frame: hoisted out of the walk they cost 32 registers and
    // the kernel spills — 15.3 against 13.9 ms per hour)
    cpx wbase = wbase0;
    asm volatile("" : "+v"(wbase.x), "+v"(wbase.y));
    // the next frame's first round of records (its count came a frame ago) and the count of the frame after it
    uint32_t nr_i, ncv, nr_m, nr_n;
    fetch_fill(f + 1 < f1 ? f + 1 : f, cnt1, t, nr_i, ncv, nr_m, nr_n);
    cnt2 = f + 2 < f1 ? a.pkcount[f + 2 + lane0] : 0u;
    cpx Y[P::E], v[P::E];
    // This thread's 2 x 16 bins of the frame: c = t + T e and its mirror M - c (bin M, thread 0's mirror of c = 0, is the
    // dropped Nyquist bin: the read is clamped and the coefficient zeroed), and their offsets
    cpx rx[2 * P::E];
    uint32_t cc[2 * P::E];  // (one batch of LDS reads in front of the wave-uniform branches below, not one wait per branch)
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const int c = t + P::T * e;
      const int cm = (P::M - c) & (P::M - 1);  // (c = 0 -> 0: clamped)
      rx[2 * e] = xbuf[c];
      rx[2 * e + 1] = xbuf[cm];
      cc[2 * e] = cd[c];
      cc[2 * e + 1] = cd[cm];
    }
    // Yhat[k] = X[k] e^{2 pi i C/2^32}, C the offset of the bin's owner (0: the bin keeps its analysis phase — most bins of
    // most frames: a wavefront whose bins of four slots all ride on nothing skips their phasors; multiplying by the phasor
    // of 0 would leave them bit for bit as they are, so who skips does not matter)
#pragma unroll
    for (int e4 = 0; e4 < P::E; e4 += 4) {
      uint32_t any = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) any |= cc[2 * e4 + j];
      if (__ballot(any != 0u) != 0ull) {
#pragma unroll
        for (int j = 0; j < 8; ++j) rx[2 * e4 + j] = pk_cmul2(rx[2 * e4 + j], pv_phasor(cc[2 * e4 + j]));
      }
    }
    // G[c] = conj((A + B) + i w_c (A - B)), A = Yhat[c], B = conj(Yhat[M - c]), w_c = e^{2 pi i c/N} = e^{2 pi i t/N} e^{2 pi i e/32}
    // for c = t + T e: one value kept for the walk times a constant — and w_{c + 8T} = i w_c, so slots e and e + 8 share the
    // product.  Packed arithmetic throughout: six / five instructions per slot.
#pragma unroll
    for (int e = 0; e < P::E / 2; ++e) {
      const cpx wc = pk_rot_cs(wbase, mk(kW32[e][0], -kW32[e][1]));  // wbase * (cos + i sin)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ee = e + (P::E / 2) * h;
        cpx A = rx[2 * ee], B = rx[2 * ee + 1];  // B: Yhat[M - c] itself (its conjugate enters below)
        // (bin 0 contributes its real part only — y is the real part of the one-sided sum — and bin M, thread 0's mirror
        // of c = 0, is the dropped Nyquist bin)
        if (ee == 0 && t == 0) {
          A = mk(A.x, 0.f);
          B = mk(0.f, 0.f);
        }
        const cpx Sm = pk_add_cj(A, B), Dm = pk_sub_cj(A, B);
        const cpx q = pk_cmul2(wc, Dm);
        Y[ee] = h == 0 ? pk_cj_add_i(Sm, q) : pk_cj_sub(Sm, q);  // i (i w_c Dm) = -w_c Dm
      }
    }
    pass1<P>(Y, v);
    __syncthreads();  // (every wave has read this frame's row and offsets, and its T2 columns of the previous frame)
    if (f + 1 < f1) request_row(f + 1, t);
    store_t1<P>(t, v, lds);
    zero_cd(t);
    __syncthreads();
    load_t1<P>(t, v, lds);
    __syncthreads();
    {
      cpx w[P::R2 - 1];
      root_powers7(g2b, w);
      w[7] = g2o;
#pragma unroll
      for (int r = 0; r < 7; ++r) w[8 + r] = pk_cmul2(g2o, w[r]);
      pass2_reg<P>(v, w);
    }
    store_t2<P>(t, v, lds);
    // (here, not right behind the zeroing barrier: the records requested at the top of the frame have had two passes to arrive)
    if (f + 1 < f1) fill_cd(f + 1, cnt1, t, nr_i, ncv, nr_m, nr_n);
    cnt1 = cnt2;
    row_landed();  // (requested three barriers ago)
    __syncthreads();
    // columns t (v[0..R3)) and t + NS3/2 (v[R3..E)) of the T2 image
#pragma unroll
    for (int r = 0; r < P::R3; ++r) {
      v[r] = lds[t + P::NS3 * r];
      v[P::R3 + r] = lds[t + P::NS3 / 2 + P::NS3 * r];
    }
    // pass 3 on both columns: twiddles delta^r, delta = e^{-2 pi i col/M}, from the bases delta^1, delta^2, delta^4
    auto pass3_col = [&](const cpx (&gb)[3], int o) {
      cpx in[P::R3], w[P::R3], out[P::R3];
      w[0] = mk(1.0f, 0.0f);
      root_powers7(gb, w + 1);
#pragma unroll
      for (int r = 0; r < P::R3; ++r) in[r] = v[o + r];
      DftTw<P::R3, 1, 0, false>::run(in, w, out);
#pragma unroll
      for (int r = 0; r < P::R3; ++r) v[o + r] = out[r];
    };
    pass3_col(g3p, 0);
    pass3_col(g3q, P::R3);
    // v[r] = D[t + NS3 r], v[R3 + r] = D[t + NS3/2 + NS3 r]: pair m = t + T j is v[j / 2] (j even), v[R3 + j / 2] (j odd);
    // y[2m] = Re D[m], y[2m+1] = -Im D[m], windowed, added to what the earlier frames left at the same samples (in frame
    // order: the sums group exactly as they did in the LDS ring of rounds 1-3)
    cpx hopv = mk(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < kOla; ++j) {
      const cpx d = (j & 1) ? v[P::R3 + (j >> 1)] : v[j >> 1];
      const float2 h = hw[j];
      const cpx old = j < kOla - 1 ? acc[j] : mk(0.f, 0.f);
      const cpx sum = pk_fma_cj(d, mk(h.x, h.y), old);
      if (j == 0) hopv = sum;
      else acc[j - 1] = sum;
    }
    // the hop [f*Hs, (f+1)*Hs) has now received every frame of this workgroup that reaches it
    {
      // all 16 contributors are this workgroup's (or there are none before the signal's first frame)
      const bool final_here = (f - f0 >= kPvN / kPvHs - 1) || (blk == 0 && a.global_first);
      if (final_here) {
        reinterpret_cast<float2 *>(a.s + (f - a.first) * kPvHs)[t] = make_float2(hopv.x * kPvNorm, hopv.y * kPvNorm);
      } else {
        reinterpret_cast<float2 *>(a.halo + (size_t)blk * kPvHalo + (f - f0) * kPvHs)[t] = make_float2(hopv.x, hopv.y);
      }
    }
  }
  // what is left in the accumulator: this workgroup's share of the N - Hs samples after its last hop (raw sums; pv_fixup
  // adds the next workgroup's halo and normalises)
  static_assert(kPvHalo / 2 == (kOla - 1) * P::T, "the accumulator is the halo");
#pragma unroll
  for (int j = 0; j < kOla - 1; ++j)
    reinterpret_cast<float2 *>(a.s + (f1 - a.first) * kPvHs)[t_ + P::T * j] = make_float2(acc[j].x, acc[j].y);
}

// Boundary b (0..nb): s over [f0_b*Hs, f0_b*Hs + N - Hs) holds the left workgroup's raw sums (none at b = 0); add the
// right workgroup's halo (none at b = nb) and normalise.  Across ranks (multi-GPU) the missing side comes from the
// neighbour: prev_tail at b = 0, next_head at b = nb — the overlap-add seams of SURVEY 8e(3).
// boundary and offset both come from blockIdx.x (gridDim.y stops at 65535: 2.1 M frames, an hour at +20 semitones);
// four samples per thread (s, the halos and the seams are 16-byte aligned: arena offsets, multiples of the hop)
static_assert(kPvHalo % 4 == 0, "whole 16-byte pieces");
constexpr int kFixupPerB = (kPvHalo / 4 + 255) / 256;  // workgroups per boundary
__global__ __launch_bounds__(256) void pv_fixup(const PvArgs a) {
  const int64_t fs = a.frames - a.first;
  const int64_t nb = pv_blocks(fs);
  const int64_t b = (int64_t)(blockIdx.x / kFixupPerB);
  const int i = ((int)(blockIdx.x % kFixupPerB) * 256 + threadIdx.x) * 4;
  if (i >= kPvHalo) return;
  if ((b == 0 && a.skip_head) || (b == nb && a.skip_tail)) return;
  if (b == 0) {
    if (a.global_first) return;  // the first hops of the signal were complete when they left the accumulator
    if (a.prev_final) {  // the same samples as the previous chunk's last boundary: finished there
      *reinterpret_cast<f32x4 *>(a.s + i) = *reinterpret_cast<const f32x4 *>(a.prev_final + i);
      return;
    }
    // (left + right, the order of the interior boundaries below: of two NaN terms the sum keeps the first one's sign and payload)
    f32x4 v = *reinterpret_cast<const f32x4 *>(a.halo + i);
    if (a.prev_tail) v = *reinterpret_cast<const f32x4 *>(a.prev_tail + i) + v;
    *reinterpret_cast<f32x4 *>(a.s + i) = v * kPvNorm;
    return;
  }
  const int64_t fb = b == nb ? fs : b * kPvBlockFrames;
  f32x4 v = *reinterpret_cast<const f32x4 *>(a.s + fb * kPvHs + i);
  if (b < nb) v += *reinterpret_cast<const f32x4 *>(a.halo + (size_t)b * kPvHalo + i);
  else if (a.next_head) v += *reinterpret_cast<const f32x4 *>(a.next_head + i);
  *reinterpret_cast<f32x4 *>(a.s + fb * kPvHs + i) = v * kPvNorm;
}

// Four consecutive output samples per thread: the two outputs leave as 16- and 8-byte stores (a wavefront's 4- and 2-byte
// stores were 256 and 128 bytes per instruction).  The groups of four are cut where the f32 output's addresses are 16-byte
// aligned (the int16 output's where there is no f32 output) — whatever sample the range starts at: a chunk of a long
// signal, a rank's slice and the whole signal all store wide; the ragged ends and an output whose alignment differs from
// the other's go sample by sample.  Values do not depend on the grouping.
__host__ __device__ inline int64_t pv_resample_start(const PvArgs &a) {
  const unsigned shift = a.pcm_f32 ? (unsigned)(((uintptr_t)a.pcm_f32 >> 2) & 3u) : (unsigned)(((uintptr_t)a.pcm_i16 >> 1) & 3u);
  const int64_t e_lo = a.out_lo - a.pcm_base;  // element of pcm that receives output sample out_lo
  return e_lo - (int64_t)((uint64_t)(e_lo + shift) & 3u);
}
__global__ __launch_bounds__(256) void pv_resample(const PvArgs a) {
  const int64_t e0 = pv_resample_start(a) + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t e_lo = a.out_lo - a.pcm_base, e_hi = a.out_hi - a.pcm_base;
  if (e0 >= e_hi) return;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int64_t e = e0 + q;
    e = e < e_lo ? e_lo : (e < e_hi ? e : e_hi - 1);  // (clamped copies are computed, not stored)
    const int64_t i = e + a.pcm_base;
    const double pos = (double)i * a.ratio + (double)(kPvN / 2);
    const double fl = floor(pos);
    const int64_t m = (int64_t)fl - a.s_origin;  // s[0] is stretched sample s_origin of the whole signal
    const float tt = (float)(pos - fl);
    v[q] = (1.0f - tt) * a.s[m] + tt * a.s[m + 1];
  }
  int16_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = pcm16_clamped(v[q]);
  const bool whole = e0 >= e_lo && e0 + 4 <= e_hi;
  if (a.pcm_f32) {
    float *o = a.pcm_f32 + e0;
    if (whole && ((uintptr_t)o & 15u) == 0u) {
      *reinterpret_cast<f32x4 *>(o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e0 + q >= e_lo && e0 + q < e_hi) o[q] = v[q];
    }
  }
  if (a.pcm_i16) {
    int16_t *o = a.pcm_i16 + e0;
    if (whole && ((uintptr_t)o & 7u) == 0u) {
      *reinterpret_cast<i16x4 *>(o) = i16x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e0 + q >= e_lo && e0 + q < e_hi) o[q] = w[q];
    }
  }
}

// Marker-driven variant: the ratio is constant over a frame's hop, so frame f owns the output samples
// [i0_f, i0_{f+1}) and reads the stretched signal at u = f*Hs + (i/sr - t_f) * r_f * sr.  (One workgroup per frame of the
// range; the plan rows are indexed from the range's first frame, frame_base in the whole signal.)
__global__ __launch_bounds__(256) void pv_resample_frames(const PvArgs a) {
  const int64_t j = blockIdx.x, f = a.frame_base + j;
  const int64_t lo = a.i0[j], hi = a.i0[j + 1];
  const double tf = a.tf[j], rs = a.rf[j] * (double)a.sample_rate, sr = (double)a.sample_rate;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double pos = (double)(f * kPvHs) + ((double)i / sr - tf) * rs + (double)(kPvN / 2);
    const double fl = floor(pos);
    const int64_t m = (int64_t)fl - a.s_origin;
    const float tt = (float)(pos - fl);
    const float v = (1.0f - tt) * a.s[m] + tt * a.s[m + 1];
    if (a.pcm_f32) a.pcm_f32[i - a.pcm_base] = v;
    if (a.pcm_i16) a.pcm_i16[i - a.pcm_base] = pcm16_clamped(v);
  }
}

// dst[i] = (x[i] + y[i]) * 1/sum w^2 — the two sides of an overlap-add seam, exactly as pv_fixup adds and normalises them: x the
// left side's sums, y the right side's (the order matters where both are NaN: the sum keeps x's sign and payload)
__global__ __launch_bounds__(256) void pv_edge_sum(float *dst, const float *x, const float *y, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = x[i];
  if (y) v += y[i];
  dst[i] = v * kPvNorm;
}
}  // namespace

int64_t pv_halo_floats(int64_t frames) { return pv_blocks(frames) * (int64_t)kPvHalo; }

// The stages as the chunked pipeline launches them (capi_pv.cpp: each on a stream of its own) ...
//   launch_pv_analysis   the transforms: rows, peak maps, counts, thresholds, every frame's records but a workgroup's first
//   launch_pv_maps       those first records, the chunk maps of the recurrence, their group maps (and the range's total map)
//   launch_pv_offsets    from carry_in: the offsets every group / chunk starts from, then every peak's offset (in the records)
//   launch_pv_synthesis  rows + offsets -> the stretched signal, with the overlap-add ring (afterwards halo[0 .. N-Hs) is this
//                        rank's head seam and s[(frames-first)*Hs ..) its tail seam, both raw)
//   launch_pv_finish     boundary fix-up (with the neighbours' seams) and resampling
// ... and as one rank of a multi-GPU run sees them: stage 1 (launch_pv_analyze) = analysis + maps, with this rank's phase
// totals; stage 2 (launch_pv_synthesize) = offsets, from carry_in, + synthesis; stage 3 = finish.
hipError_t launch_pv_synthesis(const PvArgs &a, hipStream_t s) {
  if (a.frames - a.first <= 0) return hipSuccess;
  hipLaunchKernelGGL(pv_synthesis, dim3((unsigned)pv_blocks(a.frames - a.first)), dim3(PV::T), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_pv_analyze(const PvArgs &a, hipStream_t s) {
  const hipError_t e = launch_pv_analysis(a, s);
  return e == hipSuccess ? launch_pv_maps(a, s) : e;
}
hipError_t launch_pv_synthesize(const PvArgs &a, hipStream_t s) {
  const hipError_t e = launch_pv_offsets(a, s);
  return e == hipSuccess ? launch_pv_synthesis(a, s) : e;
}
hipError_t launch_pv_finish(const PvArgs &a, hipStream_t s) {
  if (a.frames - a.first <= 0) return hipSuccess;
  const int64_t nb = pv_blocks(a.frames - a.first);
  if ((nb + 1) * (int64_t)kFixupPerB > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pv_fixup, dim3((unsigned)((nb + 1) * kFixupPerB)), dim3(256), 0, s, a);
  if (a.i0)  // marker-driven: one workgroup per frame
    hipLaunchKernelGGL(pv_resample_frames, dim3((unsigned)(a.frames - a.first)), dim3(256), 0, s, a);
  else if (const hipError_t e = launch_pv_resample(a, s); e != hipSuccess) return e;
  return hipGetLastError();
}
hipError_t launch_pv_edge_sum(float *dst, const float *x, const float *y, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pv_edge_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, x, y, n);
  return hipGetLastError();
}

// the constant-ratio resampler alone, over [out_lo, out_hi) from whatever a.s / a.s_origin point at (a rank's deferred edges)
hipError_t launch_pv_resample(const PvArgs &a, hipStream_t s) {
  if (a.out_hi <= a.out_lo) return hipSuccess;
  hipLaunchKernelGGL(pv_resample, dim3((unsigned)((a.out_hi - a.pcm_base - pv_resample_start(a) + 1023) / 1024)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_pv(const PvArgs &a, hipStream_t s) {
  if (a.frames <= 0 || a.n <= 0) return hipSuccess;
  hipError_t e = launch_pv_analyze(a, s);
  if (e == hipSuccess) e = launch_pv_synthesize(a, s);
  if (e == hipSuccess) e = launch_pv_finish(a, s);
  return e;
}

}  // namespace mx
