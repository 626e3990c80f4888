// kernels.h — internal launch interface between the C-ABI layer (capi_*.cpp) and
// the gfx950 kernels (*.hip).  Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/melonix_amd.h"

namespace mx {

enum StftMode {
  kBulkAligned = 0,  // uniform hop, even hop: 64-bit sample/weight loads
  kBulkAny = 1,      // uniform hop, odd hop
  kRanges = 2,       // per-frame (start,end) list
};

struct StftArgs {
  const float *audio;  // padded image: [MX_AUDIO_PAD zeros][n][MX_AUDIO_PAD zeros]
  int64_t n;
  const float *wtab;      // bulk: N forward weights, pre-scaled by 1/(2N)
  const float *wext;      // ranges: d-indexed weights, pre-scaled by 1/(2N) (stft_tables.h)
  float decay;            // exp(-2.5e-4*hop): per-hop decay of the sliding window
  const float2 *tw2;      // pass-2 twiddles
  const float2 *tw3;      // pass-3 twiddles
  const float2 *ubase;    // post-split bases
  const int32_t *ranges;  // ranges mode: count x {start,end} (device)
  int hop;
  int64_t first_frame;
  int64_t count;
  int kmin, kmax;
  float *mags;       // count x N/2, may be null
  mx_pitch *pitch;   // count, may be null
  uint8_t *rgb;      // count x N/2 x 3 (fused colormap), may be null
  float cmap_k;
  int frames_per_block;
};

hipError_t launch_stft(int N, int mode, const StftArgs &a, hipStream_t s);
// Points per thread of the plan launch_stft uses for N (selects the twiddle tables to upload).
constexpr int kPlan4096E = 16;
int stft_points_per_thread(int N);
// Longest run of consecutive frames worth giving one workgroup for (N, mode, hop): the kernels that carry a register
// image from frame to frame amortise their first frame's direct load over the run.
int stft_frames_per_block_cap(int N, int mode, int hop);

struct ResynthArgs {
  const float *audio;  // padded image
  const mx_step *steps;
  int64_t nsteps;
  int64_t nsamples;    // total incl. trailing zeros
  float *pcm_f32;      // may be null
  int16_t *pcm_i16;    // may be null
};
hipError_t launch_resynth(const ResynthArgs &a, hipStream_t s);

// Build-defined phase-vocoder pitch shifter (pv_common.h and its units pv_*.hip; no reference counterpart).
struct PvArgs {
  const float *audio;  // padded image (zeros in the pads)
  int64_t n;
  double ratio;            // r = 2^(semitones/12)
  const int64_t *apos;     // analysis centres a_f = floor(f*Hs/r), frames entries
  const uint32_t *hop;     // a_f - a_{f-1}; 0 for local row 0 of the whole signal and where a plan does not advance
  const double *hratio;    // Hs / hop (binary64 quotient), 0 where hop is 0
  int64_t frames;
  const float *hann_scaled;  // periodic Hann * 1/(2N): the analysis window with the transform's folded scale
  const float *hann;         // periodic Hann (synthesis window)
  const float2 *wsplit;      // e^{+2 pi i c/N}, c = 0..N/2-1 (pre-split of the inverse transform)
  const float2 *tw2, *tw3, *ubase;  // Plan<4096,16> tables
  // Per frame (row) the analysis leaves: the one-sided spectrum X/N, complex (what synthesis rotates), the frame's spectral
  // peaks as a 2048-bit map, and one 8-byte record per peak, in bin order — everything the phase recurrence needs of the
  // frame (the recurrence runs over peaks only; every other bin rides on its owner peak's phasor):
  //   rec.x = p | q << 11 | qvalid << 22 | cont << 23   p: the peak's bin; q: the peak of the PREVIOUS frame that owns bin p
  //                                                     (nearest within reach); cont: p carried signal in both frames and h >= 1
  //   rec.y = delta = P_{f-1}[p] + inc_f[p] - P_f[p]    (uint32 turns; inc: pv_inc)
  // so that the peak's synthesis offset is  C_f[p] = E_{f-1}[p] + delta  (cont) with E_{f-1}[p] = C_{f-1}[q] where q
  // continued itself, else 0; a peak that does not continue restarts (offset 0: its bins keep their analysis phases).
  float2 *xrows;       // [frames][N/2]
  uint32_t *pkmap;     // [frames][N/64] bit k: bin k is a spectral peak of the frame
  uint32_t *pkcount;   // [frames] bits 0..11: number of peaks (= records) of the frame; bits 12..: where they start inside the
                       // frame's analysis workgroup's region of the record pool (below)
  float *fthr;         // [frames] the frame's activity threshold (squared magnitude): what the next frame's records compare with
  uint2 *recs;         // the frames' records, in the pool; the second sweep REPLACES rec.y by C_f of
                       // the peak (0 = restarted): delta has no reader after it.  Every analysis workgroup (frames_per_block
                       // consecutive frames) packs its frames' records one behind the other into a region of rec_wg_cap entries
                       // of its own (no atomics: the layout is a function of the signal).  A region that does not hold its
                       // frames (rec_wg_cap < frames_per_block * N/2 is a bet on the signal: an impulse makes every bin a peak)
                       // raises *rec_overflow: the caller discards the run and repeats it with full-sized regions
  uint32_t rec_wg_cap; // records per analysis workgroup's region
  int rec_fpb_shift;   // log2(frames_per_block of the analysis launch): local frame f lies in region f >> rec_fpb_shift
  uint32_t *rec_overflow;  // [1] set to 1 by an analysis workgroup whose region is too small (the run's results are void)
  uint32_t *chunk_sums;  // [ceil(frames/scan_chunk)][N/2] a chunk's composed map: delta (or restart value) ...
  uint16_t *chunk_org;   // ... and source bin at the chunk's start (0xFFFF: restart); then the chunk-start offsets
  uint32_t *group_sums;  // [ceil(chunks/32)][N/2] the same for groups of 32 chunks (the composition is two-level)
  uint16_t *group_org;
  int scan_chunk;
  float *halo;        // pv_halo_floats(frames): partial sums right of each synthesis-workgroup boundary
  float *s;           // stretched signal, s_len = frames*Hs + N, index 0 = stretched time -N/2
  int64_t s_len;
  float *pcm_f32;     // output sample i of the whole signal is pcm[i - pcm_base]; may be null
  int16_t *pcm_i16;   // likewise
  int64_t pcm_base;
  int frames_per_block;
  // multi-GPU (one rank's part of the frame axis; all zero / null for a whole-signal run)
  int64_t first;             // local frames [first, frames) are this rank's; first = 1: row 0 is the frame before them
  int global_first;          // this rank holds the signal's frame 0
  const uint32_t *carry_in;  // [N/2] synthesis phase at the end of the previous rank's / chunk's last frame (null: zero)
  uint32_t *carry_out;       // [N/2] out: the same row at the end of THIS range's last frame (null: not wanted)
  uint32_t *tot_sums;        // [N/2] out: this rank's total map over its frames (null: not wanted): delta / value ...
  uint16_t *tot_org;         // ... and source bin at the rank's start (0xFFFF: restart)
  const float *prev_tail;    // [N-Hs] the previous rank's tail seam (raw sums), null on the first rank
  const float *next_head;    // [N-Hs] the next rank's head seam, null on the last rank
  const float *prev_final;   // [N-Hs] the previous chunk's FINISHED samples across boundary 0 (one GPU walking the signal chunk by
                             // chunk: the previous chunk's fix-up already added the two sides and normalised); overrides prev_tail
  int skip_head, skip_tail;  // pv_fixup leaves boundary 0 / the last boundary alone (a rank's edges wait for its neighbours' seams)
  int64_t out_lo, out_hi;    // output samples [out_lo, out_hi) of the whole signal are resampled here
  int64_t s_origin;          // stretched sample index (incl. the N/2 offset) of s[0]
  // marker-driven plan (null for a constant ratio): per frame warped time, ratio and first output sample
  // (indexed like the frames this range synthesises: entry 0 is local frame `first`)
  const double *tf, *rf;
  const int64_t *i0;         // one entry more than frames
  int64_t frame_base;        // index in the whole signal of local frame `first`
  int sample_rate;
};
// The launch side of every kernel that walks runs of consecutive frames (f0_yin, chroma_frames, onset_flux_kernel,
// sib_features_kernel): `run` frames per workgroup — the caller's, or `fallback` where that is <= 0 —, doubled until the blocks
// fit the grid's x extent; -> the grid.  No output depends on the run.
inline dim3 walk_grid(int64_t count, int &run, int fallback) {
  if (run <= 0) run = fallback;
  while ((count + run - 1) / run > (1ll << 30)) run *= 2;
  return dim3((unsigned)((count + run - 1) / run));
}
constexpr int kPlan4096Run = 8;  // the fallback of the Plan<4096,16> walkers (f0_yin, chroma_frames)
// ... and of the one-wavefront walkers of the 1024-point transform: long runs where there are frames enough to fill the device
// with them (an onset run pays `lag` frames at its head)
inline int onset_default_run(int64_t count) {
  const int64_t want = count / 4096;
  return (int)(want < 1 ? 1 : want > 32 ? 32 : want);
}

hipError_t launch_pv(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_analyze(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_synthesize(const PvArgs &a, hipStream_t s);
// the same stages in the pieces the chunked pipeline puts on streams of their own (pv_synthesis.hip: launch_pv_analyze =
// analysis + maps, launch_pv_synthesize = offsets + synthesis)
hipError_t launch_pv_analysis(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_maps(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_offsets(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_synthesis(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_finish(const PvArgs &a, hipStream_t s);
int64_t pv_halo_floats(int64_t frames);
// the composition, in order, of n maps -> one; sums_stride / org_stride: elements between consecutive maps' rows (0: dense, N/2)
hipError_t launch_pv_compose_maps(const uint32_t *sums, const uint16_t *org, int64_t n, uint32_t *out_sums, uint16_t *out_org, hipStream_t s,
                                  int sums_stride = 0, int org_stride = 0);
hipError_t launch_pv_resample(const PvArgs &a, hipStream_t s);
hipError_t launch_pv_edge_sum(float *dst, const float *x, const float *y, int n, hipStream_t s);
// constant-ratio analysis plan written on the device: rows of apos / hop / hratio for global frames fbase, fbase+1, ...
hipError_t launch_pv_plan_const(int64_t *apos, uint32_t *hop, double *hratio, int64_t rows, int64_t fbase, double r,
                                hipStream_t s);

// Build-defined YIN f0 tracker (f0_kernels.hip; the reference has no detector).  Frame first_frame + f (f < count) is
// centred on sample (first_frame + f) * hop; out[f] its record.  tau_min / tau_max: the search range, checked by the caller.
struct F0Args {
  const float *audio;  // padded image (zeros in the pads)
  int hop;
  int64_t first_frame;
  int64_t count;
  int tau_min, tau_max;
  float threshold;
  const float2 *tw2, *tw3, *ubase;  // Plan<4096,16> tables
  mx_f0 *out;
  int frames_per_block;  // 0: the default
  // the candidate ladder (f0_yin's second instantiation): set, a frame's MX_F0_CANDS slots go to cands[4 f ..] and `out` may
  // be null; null: the plain tracker.  sample_rate: the ladder's cents
  mx_f0_cand *cands;
  int sample_rate;
};
hipError_t launch_f0(const F0Args &a, hipStream_t s);

// Build-defined Viterbi decode over the ladder (f0_decode.hip).  Costs already in Q16 (q() of the header).  Scratch, all of
// the caller's, of the byte counts f0_decode_scratch(count, chunk) gives; chunk: frames per chunk, >= 1.
struct F0DecodeArgs {
  const mx_f0 *track;
  const mx_f0_cand *cands;
  int64_t count;
  int64_t q_unvoiced, q_jump, q_switch;
  int32_t max_jump_cents;
  int64_t chunk;
  uint16_t *bp;
  int64_t *prod;
  uint16_t *map;
  mx_f0 *out;      // may alias track
  uint8_t *state;  // may be null
};
int64_t f0_decode_default_chunk(int64_t count);
struct F0DecodeScratch {
  size_t bp, prod, map;  // bytes
};
F0DecodeScratch f0_decode_scratch(int64_t count, int64_t chunk);
hipError_t launch_f0_decode(const F0DecodeArgs &a, hipStream_t s);
// Build-defined PSOLA overlap-add (psola_kernels.hip; records: psola_plan.cpp, definition: include/melonix_amd.h).  The
// records are not validated on the device: bad ones give wrong samples, no access outside the padded audio or the outputs.
// Rec: mx_psola_grain, or mx_psola_fgrain (the formant shift: the same walk, another source address per sample).
template <class Rec>
struct PsolaArgsT {
  const float *audio;  // padded image (zeros in the pads)
  int64_t n;
  const Rec *grains;
  int64_t ngrains;
  int64_t nsamples;
  float *pcm_f32;    // may be null
  int16_t *pcm_i16;  // may be null
};
using PsolaArgs = PsolaArgsT<mx_psola_grain>;
using PsolaFormantArgs = PsolaArgsT<mx_psola_fgrain>;
hipError_t launch_psola(const PsolaArgs &a, hipStream_t s);
hipError_t launch_psola(const PsolaFormantArgs &a, hipStream_t s);
// Build-defined onset strength (onset_kernels.hip; definition: include/melonix_amd.h).  Frame first_frame + f (f < count) is
// centred on sample (first_frame + f) * hop; flux[f] its value.  lag in [1, 4], 1 <= kmin <= kmax <= 511: checked by the caller.
struct OnsetArgs {
  const float *audio;  // padded image (zeros in the pads)
  int hop;
  int64_t first_frame;
  int64_t count;
  int lag, kmin, kmax;
  float compress;
  const float2 *tw;  // W1024^j = e^{-2 pi i j/1024}, j < 1024
  float *flux;
  int run;  // consecutive frames per wavefront; 0: the default.  The output does not depend on it
};
hipError_t launch_onset_flux(const OnsetArgs &a, hipStream_t s);
// Build-defined sibilant features (sibilant_kernels.hip; definition: include/melonix_amd.h, arithmetic: sibilant_core.h on
// onset_core.h's transform).  Frames as OnsetArgs; out[f] the record of frame first_frame + f.  1 <= ks <= 512: checked by the caller.
struct SibArgs {
  const float *audio;  // padded image (zeros in the pads)
  int hop;
  int64_t first_frame;
  int64_t count;
  int ks;
  const float2 *tw;  // the onset transform's table
  mx_sib_feat *out;
  int run;  // consecutive frames per wavefront; 0: onset_default_run's.  The output does not depend on it
};
hipError_t launch_sib_features(const SibArgs &a, hipStream_t s);
// Build-defined source gain (gain_kernels.hip; definition: include/melonix_amd.h).  dst: samples [0, n) of the new object
// (16-byte aligned, as src).  The points are not validated on the device: bad ones give wrong samples, no store outside [0, n).
hipError_t launch_audio_gain(const float *src, float *dst, int64_t n, const mx_gain_point *pts, int64_t npts, hipStream_t s);
// Build-defined loudness records (loudness_kernels.hip; definition: include/melonix_amd.h, arithmetic: loudness_core.h).  Groups
// [first_group, first_group + ngroups) of the take, all inside it, S and W the geometry of the sample rate: checked by the
// caller.  out: the records of step G*first_group on, 16-byte aligned; only records of steps that exist are written.
struct LoudnessArgs {
  const float *image;  // padded image (the samples before the file are taken as zeros whatever the pad holds)
  int64_t n;
  int S, W;
  int64_t first_group, ngroups;
  double coeffs[10];  // mx_loudness_coeffs' order
  mx_loud_step *out;
};
hipError_t launch_loudness_steps(const LoudnessArgs &a, hipStream_t s);
// Build-defined true-peak records (truepeak_kernels.hip; definition: include/melonix_amd.h, arithmetic: truepeak_core.h).  Steps
// [first_step, first_step + nsteps) of the take, all inside it, S and L the geometry of the sample rate: checked by the caller.
// out: the record of step first_step on, 8-byte aligned.
struct TruePeakArgs {
  const float *image;  // padded image (the samples outside the file are taken as zeros whatever the pads hold)
  int64_t n;
  int S, L;
  int64_t first_step, nsteps;
  mx_tp_step *out;
};
hipError_t launch_true_peak_steps(const TruePeakArgs &a, hipStream_t s);
// Build-defined look-ahead limiter (the same unit).  dst: samples [0, n) of the new object (16-byte aligned, as the image);
// pcm16: n int16 or null.  ceiling a normal binary32 in (0, 1], lookahead in [1, 1024]: checked by the caller.  No store
// outside [0, n) of either output.
struct LimitArgs {
  const float *image;  // padded image, as above
  int64_t n;
  int L;
  float ceiling;
  int lookahead;
  float *dst;
  int16_t *pcm16;
};
hipError_t launch_audio_limit(const LimitArgs &a, hipStream_t s);
// Build-defined sample-rate conversion (resample_kernels.hip; definition: include/melonix_amd.h, arithmetic: resample_core.h).
// Outputs [first_out, first_out + count) of the converted take, all inside [0, m), plan a plan of rs::plan_for with taps > 0:
// checked by the caller.  table: the plan's taps with a row per tap index (resample_table_by_tap), in HBM.  out: 4-byte aligned;
// no store outside out[0 .. count).
struct ResampleArgs {
  const float *image;  // padded image (the samples outside the file are taken as zeros whatever the pads hold)
  int64_t n;
  mx_resample_plan plan;
  const float *table;
  int64_t first_out, count;
  float *out;
};
hipError_t launch_resample(const ResampleArgs &a, hipStream_t s);
// Build-defined noise reduction (denoise_kernels.hip; definition: include/melonix_amd.h, arithmetic: denoise_core.h on
// onset_core.h's transform).  Outputs [first, first + count) of the cleaned take, all inside [0, n): checked by the caller.
// print: the 513 values, in HBM; sens, floor: mx_denoise_factors'.  f32 (4-byte aligned) and i16 (2-byte aligned), each or null:
// no store outside [0 .. count) of either.
struct DenoiseArgs {
  const float *image;  // padded image (the samples outside the file are taken as zeros whatever the pads hold)
  int64_t n;
  const float2 *tw;  // the onset transform's table
  const float *print;
  float sens, floor;
  int64_t first, count;
  float *f32;
  int16_t *i16;
  int run;  // output blocks of 256 samples per wavefront; 0: the default.  The output does not depend on it
};
hipError_t launch_denoise(const DenoiseArgs &a, hipStream_t s);
// The power rows of frames [first_frame, first_frame + count) of the same framing: rows[513 f + k] = (|X_k| / 512)^2; and the
// print of `count` rows (1 .. 8192: checked by the caller): their binary64 sum in ascending frame order / count, to binary32.
struct NoiseRowsArgs {
  const float *image;
  int64_t n;
  const float2 *tw;
  int64_t first_frame, count;
  float *rows;
  int run;  // consecutive frames per wavefront; 0: onset_default_run's
};
hipError_t launch_noise_rows(const NoiseRowsArgs &a, hipStream_t s);
hipError_t launch_noise_print(const float *rows, int64_t count, float *print, hipStream_t s);
// Build-defined dynamics compressor (compress_kernels.hip; definition: include/melonix_amd.h, arithmetic: compress_core.h).
// Peaks: p_b of steps [first_step, first_step + nsteps), any steps (0 outside the file's) -> out[0 .. nsteps).
struct CompressPeaksArgs {
  const float *image;  // padded image (the samples outside the file do not exist whatever the pads hold)
  int64_t n;
  int D;
  int64_t first_step, nsteps;
  float *out;
};
hipError_t launch_compress_peaks(const CompressPeaksArgs &a, hipStream_t s);
// Curve: groups [g0, g0 + groups) walk their steps [g Gc - W, min((g + 1) Gc, total)) over peaks[b - peaks_first] — every such step
// is there: the caller's sizing — and store s_b to out[b - out_first] for their own steps inside [out_first, out_end).
struct CompressCurveArgs {
  const float *peaks;
  int64_t peaks_first;
  const int32_t *table;  // T[0 .. 2049), in HBM
  int32_t c_att, c_rel, W;
  int64_t g0, groups, total;
  int32_t *out;
  int64_t out_first, out_end;
};
hipError_t launch_compress_curve(const CompressCurveArgs &a, hipStream_t s);
// Apply: outputs [first, first + count), all inside [0, n): checked by the caller.  curve[u - curve_first] = s_u for every
// u >= 0 the range reads (cp::gain_lo .. cp::gain_hi).  f32 (4-byte aligned) and i16 (2-byte aligned), each or null: no store
// outside [0 .. count) of either.
struct CompressApplyArgs {
  const float *image;
  int64_t n;
  int D, K;
  float makeup;
  const int32_t *curve;
  int64_t curve_first;
  int64_t first, count;
  float *f32;
  int16_t *i16;
};
hipError_t launch_compress_apply(const CompressApplyArgs &a, hipStream_t s);
// Build-defined tempo estimation (tempo_kernels.hip; definition: include/melonix_amd.h, arithmetic: tempo_core.h).  Smoothing:
// count <= INT32_MAX, width in [0, 32], d_out not overlapping d_flux.  Comb: one record per job, count >= 1; a job outside its
// range (the caller's check) gives a wrong record and nothing worse.
namespace tempo { struct SmoothWeights; }
hipError_t launch_tempo_smooth(const float *d_flux, int64_t count, int width, const tempo::SmoothWeights &w, float *d_out,
                               hipStream_t s);
hipError_t launch_tempo_comb(const float *d_curve, int64_t count, const mx_comb_job *d_jobs, int64_t njobs, mx_comb *d_out,
                             hipStream_t s);
// spec-cache.cpp:77-96 colormap: nbins_total magnitudes -> 3*nbins_total bytes (both device).
hipError_t launch_colormap(const float *mags, uint8_t *rgb, int64_t nbins_total, float k, hipStream_t s);

// App::calcPicks (app.cpp:347-378): all levels, level after level, into d_out ({min,max} pairs; n pairs
// of capacity always suffice); counts[l] = pairs in level l (host array of >= 64), *nlevels = levels.
hipError_t launch_picks(const float *audio_padded, int64_t n, float *d_out, int64_t *counts, int *nlevels, hipStream_t s);

// Zero-crossing predicate bitmaps for grain segmentation (app.cpp:167-181, 202-216).
hipError_t launch_zc_bitmaps(const float *audio_padded, int64_t n, uint64_t *zc7, uint64_t *zc3,
                             hipStream_t s);

// The grain chain of App::preproc on the device (grain_chain.hip): phase 1 ranks the look-around-3 bits (read header word 2
// = node count back), phase 2 builds the chain; header word 1 = grain count, table = starts / lens / first samples.
size_t grain_rank_scratch_bytes(int64_t n);
hipError_t launch_grain_rank(const float *audio_padded, int64_t n, const uint64_t *zc7, const uint64_t *zc3, void *rank_scratch,
                             hipStream_t s);
void grain_chain_sizes(int64_t n, uint32_t nodes, int *levels_out, uint32_t *out_cap_out, size_t *bytes_out);
hipError_t launch_grain_chain(const float *audio_padded, int64_t n, const uint64_t *zc7, const uint64_t *zc3, void *rank_scratch,
                              uint32_t nodes, void *chain_scratch, int32_t **d_starts, int32_t **d_lens, float **d_firsts,
                              hipStream_t s);

}  // namespace mx
