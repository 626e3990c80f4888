// pv_common.h — BUILD-DEFINED phase-vocoder pitch shifter: what its units pv_analysis.hip,
// pv_lock.hip and pv_synthesis.hip share, and what they are.  Private to them.
//
// The reference has no phase vocoder: its pitch shift is the granular resampler of app.cpp:294-345,
// which resynth_kernels.hip reproduces bit for bit.  BASELINE.json's north_star names a phase-vocoder /
// overlap-add resynthesis, so the build defines one; its only oracle is the build's own restatement
// (oracle/pv_oracle.py, whose header is the definition: N = 4096, Hs = 256, stretch by r then resample
// by r).  PARITY UNPINNED — there is no reference arithmetic to match.
//
// Round 4: the phasor form of identity phase locking.  With every bin riding on its owner peak p,
//   Phi_f[k] = Phi_{f-1}[p] + inc_f[p] + (P_f[k] - P_f[p])   =>   |X_f[k]| e^{i Phi_f[k]} = X_f[k] * e^{i C_f[p]},
//   C_f[p] = Phi_{f-1}[p] + inc_f[p] - P_f[p]
// — the synthesis coefficient of a bin is its ANALYSIS coefficient rotated by its peak's offset.  So nothing but the
// peaks ever needs a phase: the analysis leaves the complex spectra and one 8-byte record per peak, the recurrence runs
// over the records alone, and synthesis rotates.  Against rounds 1-3 (magnitude rows, arg rows for every bin, a
// synthesis-phase row for every bin, two sweeps that each read whole rows): no atan2 outside the peaks, no Phi rows, no
// row traffic in the sweeps — 40 GB of intermediates per hour of audio become 27, of which the sweeps touch a few MB.
// The peaks' bookkeeping is the same integer arithmetic on the same values as before (uint32 turns, composable maps).
//
// Stages:
//   pv_analysis   one workgroup walks consecutive frames: Hann-windowed frame at a_f -> the LDS-resident real FFT of
//                 stft_core.h -> X/N, rows [F][N/2] complex; the frame's peaks (active, not below rho times any of its
//                 four neighbours) as a 2048-bit map and, compacted in bin order (a workgroup's frames one behind the other in its
//                 region of the record pool; pkcount[f] = count | place), one record per peak:
//                 (bin p, owner q of bin p in the PREVIOUS frame's peak map, continues?, delta) with
//                 delta = P_{f-1}[p] + inc_f[p] - P_f[p] — made one frame later from the two rows in HBM/L2 (the gathers
//                 travel under the next frame's transform)
//   pv_heads      the records of every analysis workgroup's FIRST frame (they need the previous workgroup's last row, map and
//                 threshold): from memory, behind the analysis
//   pv_lock_walk  the recurrence over the records of a chunk of the frame axis, one barrier per row, rows a few dozen
//                 records long:   C_f[p] = E_{f-1}[p] + delta  (continues)  |  restart,
//                 E_{f-1}[p] = C_{f-1}[q] where q (valid) continued itself, else 0.  A frame is therefore a map
//                 bin -> (source bin, delta) | restart, maps compose associatively, and the frame axis is scanned in
//                 chunks: composed chunk maps (dense again at the chunk's end: every bin's owner in the last row), a
//                 serial pass over them (pv_lock_chunks), then the same walk with the chunk-start offsets writes the
//                 peaks' C values, in record order
//   pv_synthesis  a workgroup walks >= 32 consecutive frames: the next frame's row arrives as LDS-DMA, requested a frame
//                 ahead; the frame's peaks claim their bins (interval fill of a per-bin offset array in LDS, between the
//                 transform's own barriers), every bin's coefficient is X_f[k] e^{2 pi i C/2^32} -> inverse real FFT (the
//                 same three passes on the conjugated, pre-split spectrum; the last one on the columns t and t + NS3/2) ->
//                 Hann window -> overlap-add in REGISTERS (a thread's sample pairs map onto themselves under a shift by one
//                 hop); after each frame the oldest hop is complete and leaves as one 1 KiB store, normalised by
//                 sum w^2 = 3N/(8 Hs).  Only the N - Hs samples either side of a workgroup boundary see two workgroups:
//                 the left one leaves its partial sums in s, the right one in a halo buffer
//   pv_fixup      adds the halo to s across each boundary (in frame order: deterministic, no atomics)
//   pv_resample   linear interpolation at i*r -> f32 / int16 PCM (pv_resample_frames: the marker-driven variant,
//                 where each frame carries its own warped time and ratio and owns a range of output samples)
// One rank of a multi-GPU run executes the same kernels on its range of frames in three stages
// (launch_pv_analyze / _synthesize / _finish): the offset carry into the rank and the two overlap-add seams come
// from its neighbours between the stages (capi.cpp mx_pv_shard_*, melonix_amd/shard.py).
#pragma once
#include "kernels.h"
#include "stft_core.h"

namespace mx {
namespace {

using PV = Plan<4096, 16>;
constexpr int kPvN = 4096, kPvM = kPvN / 2, kPvHs = 256;
constexpr float kPvActiveRel2 = 1e-6f;  // a bin is active within 60 dB of its frame's peak (squared magnitudes)
constexpr int kPvReach = 32;             // a peak owns bins at most this far away
// (1 - 2^-10)^2: near-ties are peaks on both sides, not left to rounding (compared on squared magnitudes)
constexpr float kPvPeakMargin2 = 0.9990234375f * 0.9990234375f;
constexpr uint16_t kPvNoBin = 0xFFFF;    // owner / origin: none
constexpr uint32_t kRecQValid = 1u << 22, kRecCont = 1u << 23;
// pkcount[f] packs the frame's peak count (bits 0..11: 0..2048) and where its records start INSIDE its analysis workgroup's
// region of the record pool (bits 12..: below 16 x 2048): one word per frame tells a reader how many records and where.
constexpr int kPkOffShift = 12;
constexpr uint32_t kPkCountMask = (1u << kPkOffShift) - 1u;
// first record of local frame f: its analysis workgroup's region ((f >> rec_fpb_shift) regions of rec_wg_cap entries in front)
// + the frame's offset inside it
// (64-bit: 4 M frames of full-size regions are 8.6e9 entries)
__device__ __forceinline__ size_t pv_rec_start(const PvArgs &a, int64_t f, uint32_t info) {
  return (size_t)(f >> a.rec_fpb_shift) * a.rec_wg_cap + (info >> kPkOffShift);
}
static_assert(kPlan4096E == 16, "pv kernels use the 16-points-per-thread tables of N = 4096");
static_assert(t1_size<PV>() == kPvM, "the FFT image of this plan is exactly one spectrum (XOR layout, no padding)");

// Owner of bin k in a peak map: the nearest peak at most kPvReach bins away, the lower one on a tie.  `pk` points at the
// map's word 0 inside an array that carries one zero word either side (pk[-1], pk[M/32]).
__device__ __forceinline__ int pv_owner(const uint32_t *pk, int k) {
  const int wi = k >> 5, bit = k & 31;
  const uint32_t w0 = pk[wi - 1], w1 = pk[wi], w2 = pk[wi + 1];
  const uint64_t below = ((uint64_t)w1 << 32) | w0, above = ((uint64_t)w2 << 32) | w1;
  const uint64_t lm_ = below & (~0ull >> (31 - bit));  // peaks at or below k (bit 32 + `bit` is k itself)
  const uint64_t rm_ = above & (~0ull << bit);         // peaks at or above k
  const int dl = lm_ ? (32 + bit) - (63 - __builtin_clzll(lm_)) : 1 << 20;
  const int dr = rm_ ? __builtin_ctzll(rm_) - bit : 1 << 20;
  const int dmin = dl <= dr ? dl : dr;
  return dmin <= kPvReach ? (dl <= dr ? k - dl : k + dr) : (int)kPvNoBin;
}

// (pv_heads, pv_lock_walk and pv_lock_chunks are chains of dependent memory and LDS round trips, a few instructions between
// them: in the chunked pipeline they run beside a transform kernel whose waves would win most issue cycles by age — they raise
// their wave priority, MX_LATENCY_BOUND_KERNEL.  They are a few hundred waves: the transform does not notice.)
#define MX_LATENCY_BOUND_KERNEL() __builtin_amdgcn_s_setprio(3)
__host__ __device__ inline int64_t pv_chunks(const PvArgs &a) { return (a.frames - a.first + a.scan_chunk - 1) / a.scan_chunk; }

constexpr int kPvBlockFrames = 32;       // frames per synthesis workgroup (the last one takes the remainder too)
constexpr int kPvHalo = kPvN - kPvHs;    // samples either side of a workgroup boundary that two workgroups feed
constexpr float kPvNorm = 1.0f / (3.0f * kPvN / (8.0f * kPvHs));
static_assert(kPvBlockFrames >= kPvN / kPvHs, "a workgroup must cover a full overlap depth");
__host__ __device__ constexpr int64_t pv_blocks(int64_t frames) {
  return frames / kPvBlockFrames > 0 ? frames / kPvBlockFrames : 1;
}

}  // namespace

// the records of every analysis workgroup's first frame (pv_analysis.hip), for launch_pv_maps (pv_lock.hip)
hipError_t launch_pv_heads(const PvArgs &a, hipStream_t s);

}  // namespace mx
