/*
 * melonix_amd.h — C-ABI boundary of the MI355X-native melonix hot path.
 *
 * This is the drop-in boundary: plain C types, opaque handles, caller-allocated
 * outputs, int status codes (0 = ok, negative = error; text via mx_last_error()).
 * No C++ types, no exceptions and no torch types cross it.  The C++ facade in
 * melonix_amd/cpp/ (Spec, SpecCache, saveWav — the reference's own class
 * surface) and every parity test / bench call through these entry points.
 *
 * Each entry point names the reference interface it replaces; file:line are
 * relative to the reference tree (mika314/melonix @ 2025-05-23).
 *
 * Device layout of an mx_audio (HBM): [MX_AUDIO_PAD zeros][n samples f32][MX_AUDIO_PAD zeros]
 * so that a frame [end-N, end) that straddles either end of the file reads
 * zeros exactly like spec.cpp:50-54 without per-sample bounds checks.
 */
#ifndef MELONIX_AMD_H
#define MELONIX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_ERR_INVALID (-1)  /* bad argument */
#define MX_ERR_DEVICE (-2)   /* HIP runtime error / no MI355X visible */
#define MX_ERR_NOMEM (-3)
#define MX_ERR_IO (-4)

#define MX_AUDIO_PAD 32768 /* samples of zero padding either side (>= largest N) */

typedef struct mx_ctx mx_ctx;     /* one per GPU / per process rank */
typedef struct mx_audio mx_audio; /* device-resident mono f32 audio */

/* Per-frame pitch record (build-defined op, SURVEY §8 a-6: the reference has no
 * detector; note law from app.cpp:499-516).  A frame that holds a sample that is Inf or NaN has a row without a finite
 * magnitude; its pitch record has kmin <= bin <= kmax and a mag that is not finite, and that record is identical whatever
 * frames_per_block or launch split computes it.  Rows and records of frames that do not hold the sample are unaffected. */
typedef struct mx_pitch {
  int32_t bin; /* argmax_k mag[k], k in [kmin,kmax], ties -> lowest k */
  float mag;   /* mag[bin] */
} mx_pitch;

/* marker.hpp:4-9 */
typedef struct mx_marker {
  int32_t sample;
  double note;
  double dTime;
  double pitchBend;
} mx_marker;

/* One App::process() call of the export loop (app.cpp:294-345), precomputed. */
typedef struct mx_step {
  double cursor;       /* warped time at entry (app.cpp:1201-1206) */
  int32_t grain_start; /* key of the chosen grain = first source sample (app.cpp:298-301) */
  int32_t grain_len;   /* grain.size() */
  float rate;          /* powf(2, pitchBend/12) (app.cpp:297) */
  float next_first;    /* nextGrainFirstSample (app.cpp:312-329) */
  int32_t sz;          /* samples this step emits (app.cpp:332-343) */
  int32_t _pad;
  int64_t out_offset;  /* exclusive prefix sum of sz = position in the PCM stream */
} mx_step;

/* ---- context ------------------------------------------------------------ */

/* device: HIP ordinal.  Fails with MX_ERR_DEVICE when no gfx950 device is usable. */
int mx_ctx_create(int device, mx_ctx **out);
void mx_ctx_destroy(mx_ctx *ctx);
/* A new context launches on its own non-blocking stream.  mx_ctx_set_stream makes it launch on a
 * caller-owned hipStream_t instead (e.g. torch's current stream; NULL = the HIP null stream);
 * mx_ctx_use_own_stream switches back. */
int mx_ctx_set_stream(mx_ctx *ctx, void *hip_stream);
int mx_ctx_use_own_stream(mx_ctx *ctx);
int mx_ctx_synchronize(mx_ctx *ctx);
/* The context keeps its work buffers between calls (device staging of the host-pointer entry points, the phase
 * vocoder's budgeted arena and its automatic budget, the host landing zone of mx_grains_dev); this releases them.
 * mx_ctx_destroy does so too. */
int mx_ctx_release_scratch(mx_ctx *ctx);
/* Run length: consecutive frames one workgroup of a bulk (uniform-hop) launch walks.  The sliding-window kernels
 * restart their window from the exact weights at the head of every run, so a row's last bits depend on where the runs
 * start.  The default is a function of the launch's frame count (a power of two, at most 32; short launches use short
 * runs so that every CU gets work): mx_stft_run_length returns it (> 0; < 0 = error code).  A job that computes one
 * signal in several launches — the frame shards of a multi-GPU run — gets the rows of the single launch bit for bit by
 * starting every launch on a multiple of 32 frames and pinning its run length to the whole signal's:
 * mx_ctx_set_frames_per_block(ctx, mx_stft_run_length(N, hop, total_frames)) (0 = back to the default).  The pin is
 * per CONTEXT, not per (N, hop): it applies to every bulk launch of that context at any size until it is set back to 0
 * (a job that mixes sizes re-pins between them); ranges-mode launches (mx_stft_ranges*) ignore it. */
int mx_stft_run_length(int N, int hop, int64_t count);
int mx_ctx_set_frames_per_block(mx_ctx *ctx, int frames);
/* Page-locked host memory for the buffers the host-pointer entry points fill (magnitude / texel rows, PCM): a
 * device->host copy into it is a direct DMA at PCIe rate, a copy into fresh pageable memory is several times slower
 * (staging + page faults).  The reference has no counterpart (its rows never leave the CPU, spec.cpp:61-65); the
 * facade's Spec worker lands every batch in such a buffer and recycles it.  Free with mx_pinned_free. */
int mx_pinned_alloc(mx_ctx *ctx, size_t bytes, void **out);
void mx_pinned_free(mx_ctx *ctx, void *p);
/* ERRORS.  Every entry point reports failure through its return value — a negative status (int / int64_t entry points), NaN (the
 * double / float time maps), MX_ERR_* as the int of mx_time2sample — and a thread-local description of the last error returned on
 * this thread; nothing is ever thrown across this boundary (every entry point's body runs inside a catch-all: std::bad_alloc ->
 * MX_ERR_NOMEM, any other exception -> MX_ERR_INVALID), and a failed call leaves its output pointers and handles untouched.
 * The reference signals no errors at all (spec.cpp / app.cpp:628-666 degrade to empty results); the facade maps a failed call to
 * an empty vector / a black column the same way. */
const char *mx_last_error(void);
/* "melonix_amd <version> gfx950" */
const char *mx_version(void);

/* ---- audio ---------------------------------------------------------------
 * Replaces Spec::Spec(std::span<float> wav) borrowing App::wavData
 * (spec.cpp:10-16, app.cpp:251): the samples are copied to HBM once.
 * MX_ERR_INVALID for n > 0x7fffffff - 2 * MX_AUDIO_PAD (2 147 418 111): the padded image's last element is then the last
 * int32 index, and every kernel indexes the image in int32. */
int mx_audio_upload(mx_ctx *ctx, const float *host_wav, int64_t n, mx_audio **out);
/* Zero-copy: wrap a device buffer already laid out [PAD zeros][n][PAD zeros]
 * (d_padded points at the first pad sample, 16-byte aligned).  The caller keeps ownership.
 * MX_ERR_INVALID, with *out untouched, for n > 0x7fffffff - 2 * MX_AUDIO_PAD: mx_audio_upload's bound and message. */
int mx_audio_wrap_device(mx_ctx *ctx, const float *d_padded, int64_t n, mx_audio **out);
int64_t mx_audio_length(const mx_audio *a);
int mx_audio_free(mx_ctx *ctx, mx_audio *a);

/* ---- STFT magnitude spectrogram + pitch pick -------------------------------
 * Replaces Spec::internalGetSpec (spec.cpp:44-66) with SpectrSize (spec.cpp:8)
 * generalised to N in {4096, 16384, 32768}: frame = samples [end-N, end),
 * one-sided exponential window expf(-2.5e-4f*(start-i)) left of `start`,
 * zeros outside the file, |DFT|/N for bins 0..N/2-1.
 *
 * kmin/kmax: pitch-pick band (inclusive, clamped to [0, N/2-1]); pass -1,-1
 * for the default band (notes 24..84 = 55..1760 Hz) at 48 kHz; for any other
 * sample rate pass the bins mx_pitch_band() returns.
 */

/* Default pitch band for (N, sampleRate): kmin=ceil(55*N/sr), kmax=floor(1760*N/sr). */
void mx_pitch_band(int N, int sampleRate, int *kmin, int *kmax);

/* The editor's note <-> frequency law (app.cpp:498-499: f(note) = 55 * 2^((note-24)/12) Hz; bin k of an
 * N-point frame sits at k*sampleRate/N Hz).  mx_bin_note turns a pitch record's bin into the value a
 * Marker::note (marker.hpp:6) holds: 24 + 12*log2(k*sampleRate/N/55); -HUGE_VAL for k <= 0.
 * mx_note_bin is its inverse (fractional bin).  Host, double. */
double mx_bin_note(int bin, int N, int sampleRate);
double mx_note_bin(double note, int N, int sampleRate);

/* Arbitrary (start,end) pairs — the drop-in mode: one call drains a whole
 * batch of Spec::getSpec jobs (spec.cpp:18-42, 68-97).  ranges = count x {start,end}
 * (host).  mags_out = count x N/2 f32 (host, may be NULL); pitch_out = count
 * records (host, may be NULL).  Blocks until the results are in host memory. */
int mx_stft_ranges(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count,
                   int kmin, int kmax, float *mags_out, mx_pitch *pitch_out);

/* Uniform hop — the bulk mode: frame h in [first_frame, first_frame+count) is
 * (start,end) = (h*hop, (h+1)*hop), i.e. the UI's column indexing
 * (spec-cache.cpp:12,63-65) with an identity time map and `hop` samples per pixel.
 * Host outputs as above; blocks. */
int mx_stft_hop(mx_ctx *ctx, const mx_audio *a, int N, int hop, int64_t first_frame, int64_t count,
                int kmin, int kmax, float *mags_out, mx_pitch *pitch_out);

/* Same, outputs stay in HBM (d_mags: count x N/2 f32, d_pitch: count records;
 * either may be NULL).  Asynchronous on the ctx stream. */
int mx_stft_hop_dev(mx_ctx *ctx, const mx_audio *a, int N, int hop, int64_t first_frame,
                    int64_t count, int kmin, int kmax, float *d_mags, mx_pitch *d_pitch);
int mx_stft_ranges_dev(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *d_ranges,
                       int64_t count, int kmin, int kmax, float *d_mags, mx_pitch *d_pitch);

/* Fused colormap (SpecCache::populateTex, spec-cache.cpp:77-96): the STFT
 * kernel's epilogue applies  magnitude * k -> clamp -> 3-segment RGB8  to the
 * row it has just produced, so texture rows leave the device as 3 bytes per bin
 * from ONE launch.  rgb = count x N/2 x 3 bytes.  The *_mags variant returns the
 * magnitude rows of the same launch as well (mags_out / d_mags may be NULL):
 * that is what a Spec worker feeding both getSpec and a SpecCache wants. */
int mx_stft_ranges_rgb(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count,
                       float k, uint8_t *rgb_out);
int mx_stft_ranges_rgb_mags(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges,
                            int64_t count, float k, float *mags_out, uint8_t *rgb_out);
int mx_stft_ranges_rgb_dev(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *d_ranges,
                           int64_t count, float k, float *d_mags, uint8_t *d_rgb);
/* The colormap alone on device-resident magnitude rows (nbins_total a multiple
 * of 4), e.g. to re-colour cached rows after the user changed k (app.cpp:75). */
int mx_colormap_dev(mx_ctx *ctx, const float *d_mags, int64_t nbins_total, float k, uint8_t *d_rgb);

/* Device-resident magnitude rows — the device-side row cache of a Spec worker (the reference keeps its
 * rows in host memory, spec.cpp:18-42).  mx_stft_ranges_keep is mx_stft_ranges_rgb_mags whose magnitude rows STAY in HBM
 * (*rows_out, count rows; release with mx_rows_free) whatever comes back to the host: rgb_out (k != 0) and mags_out
 * may each be NULL.  mx_rows_fetch copies rows [first, first+count) of a kept batch to the host; mx_rows_colormap returns
 * their texel rows for a scale k by running the colormap alone (no transform) — what a changed brightness (app.cpp:75)
 * or a late getSpec of a texel-only column costs instead of a second STFT. */
typedef struct mx_rows mx_rows;
int mx_stft_ranges_keep(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count, float k,
                        float *mags_out, uint8_t *rgb_out, mx_rows **rows_out);
int64_t mx_rows_count(const mx_rows *rows);
void mx_rows_free(mx_ctx *ctx, mx_rows *rows);
int mx_rows_fetch(mx_ctx *ctx, const mx_rows *rows, int64_t first, int64_t count, float *mags_out);
int mx_rows_colormap(mx_ctx *ctx, const mx_rows *rows, int64_t first, int64_t count, float k, uint8_t *rgb_out);

/* Number of frames of the bulk indexing: ceil(n / hop). */
int64_t mx_frame_count(int64_t n, int hop);

/* ---- time maps (host, cold-cache pure functions of the marker list) -------
 * Replace App::sample2Time / time2Sample / time2PitchBend / duration
 * (app.cpp:1020-1122).  markers must be sorted by sample. */
double mx_sample2time(const mx_marker *markers, int nmarkers, int sampleRate, int val);
int mx_time2sample(const mx_marker *markers, int nmarkers, int sampleRate, double val);
double mx_duration(const mx_marker *markers, int nmarkers, int sampleRate, int64_t nsamples);
float mx_time2pitchbend(const mx_marker *markers, int nmarkers, int sampleRate, int64_t nsamples,
                        double val);
/* SpecCache::getTex key + populateTex range (spec-cache.cpp:12, 63-65). */
void mx_column_range(const mx_marker *markers, int nmarkers, int sampleRate, double time,
                     int screenWidth, double rangeTime, int *key, int *start, int *end);

/* ---- grains + resynthesis schedule ------------------------------------------
 * mx_grains replaces the grain scan of App::preproc (app.cpp:153-235).
 * starts/lens are library-allocated (free with mx_free). */
int mx_grains(const float *host_wav, int64_t n, int32_t **starts, int32_t **lens, int64_t *count);
/* Device version: zero-crossing predicates evaluated on the GPU from the
 * resident audio; same outputs. */
int mx_grains_dev(mx_ctx *ctx, const mx_audio *a, int32_t **starts, int32_t **lens, int64_t *count);
/* The same chain as a grain TABLE: additionally firsts[g] = wav[starts[g]], the only samples the export loop reads
 * (App::process's nextGrainFirstSample, app.cpp:323-328) — with it mx_schedule_build_table needs no host copy of
 * the audio.  The chain itself is built on the device (ranks of the crossings, successor of every crossing, binary
 * lifting, expansion from start 0): only the table comes back.  firsts may be NULL. */
int mx_grain_table_dev(mx_ctx *ctx, const mx_audio *a, int32_t **starts, int32_t **lens, float **firsts, int64_t *count);

/* Replays the cursor recurrence of App::exportWav / App::process
 * (app.cpp:1200-1207, 294-331) on the host: one mx_step per process() call that
 * finds a grain.  *nsamples = sum(sz) + 1500 (the terminating call appends
 * preferredGrainSize zeros, app.cpp:303-309).  steps is library-allocated. */
int mx_schedule_build(const float *host_wav, int64_t n, int sampleRate, const int32_t *grain_starts,
                      const int32_t *grain_lens, int64_t ngrains, const mx_marker *markers,
                      int nmarkers, mx_step **steps, int64_t *nsteps, int64_t *nsamples);
/* The same chain of process() calls from any warped time: App::playback's refill loop
 * (app.cpp:272-274, `while (restWav.size() < need) tmpCursor += process(tmpCursor, restWav)` from an
 * empty restWav).  need >= 0: stop once *nsamples >= need; a call that finds no grain left adds 1500
 * zeros and leaves the cursor where it is, as often as the loop asks (the zeros are the tail of the
 * PCM, not steps).  need < 0: run to the end as mx_schedule_build does, from cursor0.
 * *cursor_end (may be NULL): the loop's cursor on exit = where the next refill continues. */
int mx_schedule_build_from(const float *host_wav, int64_t n, int sampleRate, const int32_t *grain_starts,
                           const int32_t *grain_lens, int64_t ngrains, const mx_marker *markers,
                           int nmarkers, double cursor0, int64_t need, mx_step **steps,
                           int64_t *nsteps, int64_t *nsamples, double *cursor_end);
/* mx_schedule_build_from on a grain table (mx_grain_table_dev) instead of the audio itself. */
int mx_schedule_build_table(int64_t n, int sampleRate, const int32_t *grain_starts, const int32_t *grain_lens,
                            const float *grain_firsts, int64_t ngrains, const mx_marker *markers, int nmarkers,
                            double cursor0, int64_t need, mx_step **steps, int64_t *nsteps, int64_t *nsamples,
                            double *cursor_end);
void mx_free(void *p);

/* PCM conversions.  The two float -> int16 conversions of the library, each defined for EVERY binary32 value
 * (melonix_amd/csrc/pcm16.h writes them once, for the device and the host):
 *   reference form  mx_resynth, mx_resynth_dev, mx_resynth_to_wav, mx_export_wav: what the compiled reference's
 *                   static_cast<int16_t>(v * 32767.) (app.cpp:1212) gives.  With d = (double)v * 32767.:
 *                     |d| < 2^31 (that is |v| <= 65538)   the low 16 bits of trunc(d), as a two's-complement int16
 *                                                         (1.5 -> -16386, 2 -> -2, 65537 -> 32767, 65538 -> -2);
 *                     otherwise, +-Inf and NaN included   0.
 *   clamped form    the phase vocoder and PSOLA, its formant and contour renders included:
 *                     NaN -> 0;  otherwise (int16)(clamp(v, -1, 1) * 32767.), the product in binary64, truncated toward
 *                     zero.  So +-Inf -> +-32767.
 *
 * Gather-lerp resampler + float->int16 (app.cpp:332-343, 1209-1212; the reference form above) over a
 * precomputed schedule.  pcm_f32_out / pcm_i16_out: nsamples each (host, either
 * may be NULL).  Bit-exact vs the reference arithmetic (no FMA contraction). */
int mx_resynth(mx_ctx *ctx, const mx_audio *a, const mx_step *steps, int64_t nsteps,
               int64_t nsamples, float *pcm_f32_out, int16_t *pcm_i16_out);
/* Device-resident variant: d_steps / outputs in HBM, asynchronous.
 * PRECONDITION (not checked on the device — mx_resynth, the host-pointer entry point, does check it): the steps are
 * in output order and contiguous, out_offset[0] == 0 and out_offset[i+1] == out_offset[i] + sz[i], as every
 * mx_schedule_build* call produces them (a rank's slice of a schedule rebased to its own buffer, shard_schedule in
 * melonix_amd/shard.py, qualifies).  Then every one of the nsamples outputs is written: step i fills its sz[i]
 * samples, and the samples past the LAST step record's run (the zeros of the terminating process() calls,
 * app.cpp:303-309) are cleared on the device.  With gaps or reordered records the gaps keep their previous contents. */
int mx_resynth_dev(mx_ctx *ctx, const mx_audio *a, const mx_step *d_steps, int64_t nsteps,
                   int64_t nsamples, float *d_pcm_f32, int16_t *d_pcm_i16);

/* The tail of App::exportWav (app.cpp:1209-1214) for a schedule that is already built and audio that is already
 * on the device: resynthesis to int16 and saveWav, with the PCM streamed device -> pinned pieces -> file (it never
 * exists as one host buffer).  File bytes = mx_resynth's int16 output through mx_save_wav. */
int mx_resynth_to_wav(mx_ctx *ctx, const mx_audio *a, const mx_step *steps, int64_t nsteps,
                      int64_t nsamples, const char *path, int sampleRate, int strict_reference_header);

/* Whole App::exportWav (app.cpp:1194-1215): grains -> schedule -> GPU resynth
 * -> int16 -> saveWav.  strict_reference_header!=0 reproduces save-wav.cpp:43. */
int mx_export_wav(mx_ctx *ctx, const float *host_wav, int64_t n, int sampleRate,
                  const mx_marker *markers, int nmarkers, const char *path,
                  int strict_reference_header);

/* ---- phase-vocoder pitch shift (BUILD-DEFINED) ------------------------------------
 * The reference has no phase vocoder (its pitch shift is the granular resampler above); BASELINE.json's
 * north_star names one, so the build defines it: N = 4096, synthesis hop 256, periodic Hann analysis and
 * synthesis windows, time-stretch by r = 2^(semitones/12) with integer phase propagation and identity phase
 * locking (spectral peaks carry the phase, every other bin rides on its nearest peak), overlap-add,
 * linear resampling by r back to the input length (definition: oracle/pv_oracle.py).  Constant shift over
 * the whole file; output has mx_audio_length(a) samples.  int16: the clamped form of "PCM conversions".
 * Parity is unpinned by construction: the only oracle is the build's own CPU restatement.
 * Samples that are not finite.  A frame that holds a NaN or an Inf sample — frame f holds the 4096 samples around a_f — has a
 * spectrum without a finite peak to lock to, and the 4096 stretched samples it covers, [f Hs - N/2, f Hs + N/2), are not
 * finite; so is every output either of whose two taps lies there (a NaN times a weight of 0 is NaN).  The recurrence only
 * runs forward: every output before the first such one keeps the bytes it has without the bad sample.  Behind the last one
 * every output is finite again; behind a NaN the first clean frame restarts every bin from its analysis phase (no bin of
 * the frame before it is active: NaN >= threshold is false), exactly as the oracle does, and the usual tolerance holds
 * from there on.  Chunked, sharded and device forms give the resident form's bytes, the NaNs' signs and payloads
 * included: an overlap-add seam is summed left side + right side in every form.  int16 of such outputs: "PCM conversions". */
int mx_pv_pitch_shift(mx_ctx *ctx, const mx_audio *a, double semitones, float *pcm_f32_out,
                      int16_t *pcm_i16_out);
/* Same, outputs stay in HBM (either may be NULL); blocks until done.
 * WORK ARENA: one device allocation with a BUDGET, made at the first call, kept by the context for the next one (regrown
 * only when a call needs another shape) and released by mx_ctx_release_scratch / mx_ctx_destroy.
 *   budget   mx_pv_set_arena_budget(ctx, bytes); 0 (the default) = the environment variable MELONIX_PV_ARENA_MB if set,
 *            else a quarter of what hipMemGetInfo reports free when the context first needs an arena (taken once, kept
 *            until mx_ctx_release_scratch).  mx_pv_arena_budget: the budget in force.  An arena above a newly set budget
 *            is given back at once.
 *   resident a call whose frames fit the budget (22 KiB per frame: spectra 16 KiB, peak records 4 KiB, the stretched signal,
 *            maps and plan rows; 17.9 GB for an hour at +3 semitones) is ONE chunk: analysis, phase recurrence and synthesis
 *            each run once over the whole call, and a rank of a multi-GPU run (below) analyses its frames once.
 *   chunked  what does not fit (8 h on one GPU) is walked in chunks — the longest multiple of 32 frames of which two
 *            slots of spectra + records and a ring of four stretched-signal buffers (47 KiB per frame of a chunk) fit
 *            the budget.  Chunks meet on multiples of 32 frames — the synthesis workgroups — and hand each other the
 *            phase row and the overlap-add seam the way the ranks of a multi-GPU run do: the output is bit-identical
 *            whatever the chunk length, resident included.  While a chunked call runs, two internal streams carry the
 *            phase recurrence and the fix-up / resampling beside the transforms; both are joined before the call returns.
 *   records  the peak records are packed (room for 512 peaks per frame on average over an analysis workgroup's 8 or 16
 *            frames; a frame can have 2048).  A signal with more (an impulse train) makes the call repeat itself once,
 *            transparently, on an arena with full-size record regions (34 / 71 KiB per frame), which the context then keeps
 *            until mx_ctx_release_scratch; the samples are the same either way.  MELONIX_PV_FULL_RECORDS=1 starts there.
 *   MX_ERR_NOMEM (checked against hipMemGetInfo before allocating) if the device cannot give the arena, or if the
 *            budget is below what the smallest chunks need (two slots of 32 frames: 3.5 MiB).
 * mx_pv_set_chunk_frames(frames > 0) overrides the policy with two-slot chunks of exactly that length (rounded up to a
 * multiple of 32; 0 = back to the budget; the environment variable MELONIX_PV_CHUNK_FRAMES likewise): a test that wants
 * many chunk boundaries in a short signal.  mx_pv_arena_bytes: what the context holds right now (0 before the first
 * call).  mx_pv_last_chunks: the number of chunks the last run over this arena took (1 = resident). */
int mx_pv_set_chunk_frames(mx_ctx *ctx, int64_t frames);
int mx_pv_set_arena_budget(mx_ctx *ctx, int64_t bytes);
int64_t mx_pv_arena_budget(mx_ctx *ctx);
int64_t mx_pv_arena_bytes(mx_ctx *ctx);
int64_t mx_pv_last_chunks(mx_ctx *ctx);
int mx_pv_pitch_shift_dev(mx_ctx *ctx, const mx_audio *a, double semitones, float *d_pcm_f32,
                          int16_t *d_pcm_i16);

/* The same vocoder steered by the editor's markers the way App::exportWav is (app.cpp:1194-1207, 296-301): the
 * output runs over warped time t in [0, duration()); around warped time t the source is read at time2Sample(t)
 * and shifted by 2^(time2PitchBend(t)/12), the bend taken constant over a frame's hop (definition:
 * oracle/pv_oracle.py marker_plan / render).  Still build-defined, parity unpinned.
 * mx_pv_render_length: the number of output samples (those with i/sampleRate < duration()), < 0 on error. */
int64_t mx_pv_render_length(int64_t n, int sampleRate, const mx_marker *markers, int nmarkers);
/* The frame plan itself (library-allocated, free each with mx_free): per frame the analysis centre, warped time and
 * ratio, and i0[f] = first output sample of frame f (frames + 1 entries, the last = *nsamples). */
int mx_pv_plan(int64_t n, int sampleRate, const mx_marker *markers, int nmarkers, int64_t **apos, double **tf,
               double **rf, int64_t **i0, int64_t *frames, int64_t *nsamples);
int mx_pv_render(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_marker *markers, int nmarkers,
                 float *pcm_f32_out, int16_t *pcm_i16_out);
int mx_pv_render_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_marker *markers, int nmarkers,
                     float *d_pcm_f32, int16_t *d_pcm_i16);

/* One rank of a multi-GPU phase-vocoder run (the overlap-add seams).  Every rank holds the whole
 * input and takes a contiguous range of frames (boundaries on multiples of 32 frames, so the sums group exactly
 * as in a single-GPU run and the concatenated outputs are bit-identical to mx_pv_pitch_shift's).  The caller does
 * the two small exchanges between the stages with its own collective (melonix_amd/shard.py: RCCL / gloo
 * all-gathers): the per-rank phase totals after stage 1, the seams after stage 2.  A rank works inside the same budgeted
 * arena as a single GPU (above): a range that fits the budget stays RESIDENT between the stages and is analysed once
 * (stage 1 = analysis + maps, stage 2 = offsets + synthesis from the rows stage 1 left); only a range beyond the budget is
 * walked in chunks, and then analysed twice (stage 1 keeps the maps only, stage 2 analyses again with the carry).  Every
 * rank needs at least 32 frames of its own.
 * Two forms.  Host pointers (mx_pv_shard_analyze / _synthesize / _finish): the exchanged rows travel through host memory
 * and the rank's outputs wait in library-owned device buffers (6 bytes per output sample) until stage 3 downloads them.
 * Device pointers (the _dev forms): everything a rank exchanges stays in HBM, laid out as the two all-gathers move it — each
 * stage writes the rank's entry of the next all-gather's send buffer and reads the previous all-gather's receive buffer
 * as it is — and the PCM goes straight into the caller's device buffers.
 *   mx_pv_shard_frames      the rank's frame range and the output samples [out_lo, out_hi) it will deliver
 *   mx_pv_shard_analyze     stage 1; tot_sums_out[2048] / tot_org_out[2048]: this rank's frames as one map of the
 *                           phase row: bin k ends at value[org[k]] + sums[k] (mod 2^32), or at sums[k] where
 *                           org[k] = 0xFFFF (the bin restarted inside the rank)
 *   mx_pv_shard_synthesize  stage 2; carry_in[2048]: the phase row the rank starts from = the maps of all lower
 *                           ranks applied in order to a zero row (NULL on rank 0);
 *                           head_out / tail_out[3840]: raw partial sums either side of the rank's frames
 *   mx_pv_shard_finish      stage 3; prev_tail = rank-1's tail_out (NULL on rank 0), next_head = rank+1's head_out
 *                           (NULL on the last rank); out_hi-out_lo samples each (host, either may be NULL)
 *   mx_pv_shard_analyze_dev     stage 1; d_map_out: 12 KiB on the device = 2048 uint32 sums then 2048 uint16 source bins
 *   mx_pv_shard_synthesize_dev  stage 2; d_maps_all: [world] x 12 KiB, the all-gathered stage-1 entries (the maps of the
 *                               ranks below are folded into the rank's carry on the device); d_pcm_f32 / d_pcm_i16:
 *                               out_hi - out_lo samples each on the device (either may be NULL), complete but for the
 *                               rank's edges; d_seams_out: 30 KiB = head then tail, 3840 floats each
 *   mx_pv_shard_finish_dev      stage 3; d_seams_all: [world] x 30 KiB, the all-gathered stage-2 entries; fills the edges
 *                               of the PCM buffers given to stage 2
 * Every stage blocks until its device work is done. */
int mx_pv_shard_frames(int64_t n, double semitones, int rank, int world, int64_t *frame_lo, int64_t *frame_hi,
                       int64_t *out_lo, int64_t *out_hi);
int mx_pv_shard_analyze(mx_ctx *ctx, const mx_audio *a, double semitones, int rank, int world,
                        uint32_t *tot_sums_out, uint16_t *tot_org_out);
int mx_pv_shard_synthesize(mx_ctx *ctx, const uint32_t *carry_in, float *head_out, float *tail_out);
int mx_pv_shard_finish(mx_ctx *ctx, const float *prev_tail, const float *next_head, float *pcm_f32_out,
                       int16_t *pcm_i16_out);
int mx_pv_shard_analyze_dev(mx_ctx *ctx, const mx_audio *a, double semitones, int rank, int world, void *d_map_out);
int mx_pv_shard_synthesize_dev(mx_ctx *ctx, const void *d_maps_all, float *d_pcm_f32, int16_t *d_pcm_i16,
                               void *d_seams_out);
int mx_pv_shard_finish_dev(mx_ctx *ctx, const void *d_seams_all);

/* ---- waveform min/max pyramid ---------------------------------------------------
 * Replaces App::calcPicks (app.cpp:347-378): level l = floor(n / 2^(l+1)) {min,max} pairs over blocks
 * of 2^(l+1) samples, for every l with n > 2^(l+1).  picks_out (host, caller-allocated, 2*n floats
 * always suffice) receives the levels one after the other as interleaved {min,max}; counts_out
 * (>= 64 entries) the pairs per level; *nlevels the number of levels. */
int mx_minmax_pyramid(mx_ctx *ctx, const mx_audio *a, float *picks_out, int64_t *counts_out, int *nlevels);
/* Same, the pairs stay in HBM (d_picks: 2*n floats of capacity); counts_out / nlevels are host. */
int mx_minmax_pyramid_dev(mx_ctx *ctx, const mx_audio *a, float *d_picks, int64_t *counts_out, int *nlevels);
/* Replaces App::getMinMaxFromRange (app.cpp:380-426) over such a pyramid (host), quirks included. */
void mx_minmax_range(const float *host_wav, int64_t n, const float *picks, const int64_t *counts, int nlevels,
                     int start, int end, float *mn, float *mx);

/* ---- YIN f0 tracking, notes, pitch-correction markers (BUILD-DEFINED) ---------------------------------
 * The reference has no f0 estimator (Marker::note comes from the mouse, app.cpp:923,937); the build defines one, and
 * parity is against that definition (restated in f64 by tests/yin_ref.py).  N = 4096, W = N/2.  Frame h is centred on
 * sample h*hop and reads x_j = audio[h*hop - W + j], j < N (zeros outside the file).  Per frame:
 *   d(tau) = sum_{j<W} (x_j - x_{j+tau})^2 (tau <= W, >= 0), d'(tau) = d(tau) * tau / sum_{j=1..tau} d(j) (1 where 0);
 *   search range tau_min = max(2, floor(sr/fmax)) .. tau_max = min(W-1, ceil(sr/fmin));
 *   tau* = the first tau in range with d' < threshold, then forward while d'(tau+1) < d'(tau) (tau+1 <= tau_max);
 *   none under threshold: the argmin of d' over the range (lowest tau on ties);
 *   period = tau* + parabolic offset on d at tau*-1, tau*, tau*+1 (clamped to +-1/2, 0 if the curvature is <= 0).
 * A frame is silent exactly when its samples are all zero.  The level does not change tau, period or aperiodicity: the
 * kernel scales each frame by a power of two to a fixed binade first (records are bit for bit the same for 2^k x
 * wherever 2^k x is exact in f32, subnormal samples included), and rms scales with it.  A frame that holds a NaN or an Inf
 * sample is never voiced — its aperiodicity is not below the threshold —, its record is the same whatever the launch split,
 * and every other frame keeps the bytes it has without the bad sample.
 * Defaults fmin = 55, fmax = 1760 Hz (notes 24..84), threshold 0.15.  Note law (mx_bin_note's):
 * note = 24 + 12*log2(sr / period / 55). */
typedef struct mx_f0 {
  int32_t tau;        /* tau* (0: silent, or unvoiced in a decoded track) */
  float period;       /* tau* + parabolic offset, samples (0: silent) */
  float aperiodicity; /* d'(tau*) (1: silent) */
  float rms;          /* sqrt(sum x_j^2 / N) over the frame (0: silent) */
} mx_f0;

/* Frames [first_frame, first_frame + count) of the bulk indexing (first_frame + count <= mx_frame_count(n, hop)).
 * Host output, blocks.  MX_ERR_INVALID for sr <= 0, hop outside [1, 16384], fmin <= 0, fmax <= 0, an empty search range
 * or frames outside the file. */
int mx_f0_track(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                float fmin, float fmax, float threshold, mx_f0 *out);
/* Same, the records stay in HBM (count x 16 bytes).  Asynchronous on the context's stream. */
int mx_f0_track_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                    float fmin, float fmax, float threshold, mx_f0 *d_out);

/* ---- Candidate ladder and Viterbi f0 decoding (BUILD-DEFINED, like the tracker; restated by tests/f0_decode_ref.py) ----
 * One YIN pick per frame looks at no other frame: where a subharmonic or a strong partial lifts d' at the true period
 * just above the threshold, "the first dip under theta" lands an octave away for a few frames.  The ladder keeps several
 * period candidates per frame and the decoder picks one path through the whole take.
 *
 * Candidate ladder.  Per frame, with d' and the search range of the YIN section above:
 *   rungs     theta_k = threshold * {2, 1, 1/2, 1/4}, k = 0..3, formed in f32;
 *   rung k    the tracker's tau* rule with theta_k: the first tau in range with d' < theta_k, then forward while
 *             d'(tau+1) < d'(tau) and tau+1 <= tau_max; no tau under theta_k: the rung is empty;
 *   fallback  rung 0 empty: slot 0 takes the argmin of d' over the range (lowest tau on ties), YIN's own fallback;
 *   a rung whose tau equals an earlier rung's is empty; a slot whose d' is not finite is empty; a silent frame (all
 *   samples zero) has four empty slots.
 *   Empty slot: {0, 0.f, 1.f, 0}.  Filled slot: period and aperiodicity by the tracker's arithmetic at that tau, and
 *   cents = (int32_t)rintf(1200.f * log2f((float)sr / period / 55.f)) + 2400 (100 x the note of mx_bin_note's law).
 * Wherever the plain record has aperiodicity < threshold, some slot has its tau and the same period and aperiodicity
 * bits.  Like the plain record a frame's slots depend on nothing but its samples: the same bytes whatever the launch split. */
#define MX_F0_CANDS 4
typedef struct mx_f0_cand {
  int32_t tau;        /* the rung's tau (0: empty slot) */
  float period;       /* tau + parabolic offset, samples (0: empty) */
  float aperiodicity; /* d'(tau) (1: empty) */
  int32_t cents;      /* 100 x note, rounded (0: empty) */
} mx_f0_cand;

/* Frames [first_frame, first_frame + count): MX_F0_CANDS records per frame, slot-major within the frame (frame f's slot k
 * at d_cands[4 f + k]), in HBM.  d_track may be NULL; otherwise it receives exactly mx_f0_track_dev's bytes, from the same
 * launch.  Asynchronous on the context's stream.  Argument checks: mx_f0_track's. */
int mx_f0_candidates_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                         float fmin, float fmax, float threshold, mx_f0 *d_track, mx_f0_cand *d_cands);
/* Same, host pointers (track may be NULL), through the context's staging buffers.  Blocks. */
int mx_f0_candidates(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                     float fmin, float fmax, float threshold, mx_f0 *track, mx_f0_cand *cands);

/* Decoder: the cheapest path through the frames' states.  All arithmetic in int64; Q = 65536, q(x) = (int64)rint(x * Q) on
 * the f32 value, INF = 2^56.  States j = 0..3: the frame's slots (a slot is empty when its tau is <= 0); j = 4: unvoiced.
 *   O_f(j)     min(q(aperiodicity), 2Q) for a filled slot (at least 0; 2Q for a NaN), INF for an empty one,
 *              q(unvoiced_cost) for j = 4;
 *   T_f(i, j)  between frames f-1 and f: 0 for 4 -> 4; q(switch_cost) between 4 and a slot, either way; between two filled
 *              slots q(jump_cost) * min(|cents_j - cents_i|, max_jump_cents) / 100 (integer division); 0 where either
 *              slot is empty;
 *   V_0(j) = O_0(j); V_f(j) = min_i (V_{f-1}(i) + T_f(i, j)) + O_f(j), bp_f(j) the lowest i attaining the minimum;
 *   the end state is the lowest j attaining min V_{F-1}, s_{f-1} = bp_f(s_f).  The path never enters an empty slot: the
 *   all-unvoiced path costs at most count * 16 * Q < INF.
 * Output record of frame f: the chosen slot's {tau, period, aperiodicity} with rms from track[f]; {0, 0.f, 1.f,
 * track[f].rms} where the path is unvoiced.  Output state: one uint8_t per frame, 0..4.
 * The device walks the take in chunks (min-plus products per chunk, one pass over the chunks, a re-walk per chunk; the
 * maps bp the same way backwards): no kernel takes more than max(chunk, count / chunk) dependent steps, and integers make
 * every V_f, hence the path, independent of the chunk length.
 * Defaults {0.3, 0.1, 0.5, 1200}.  Nobody has tuned them on recorded voices: they are values for which the f64 reference
 * decodes tests/f0_decode_ref.py's GLITCH signal (a steady 220 Hz tone with subharmonic and second-partial bursts: 18
 * plain frames an octave down, 5 notes) cleanly: no frame off, 1 note.  At switch_cost 0.1 the path escapes through the
 * unvoiced state instead and 28 of the 359 frames 8..F-9 come out wrong. */
typedef struct mx_f0_decode_params {
  float unvoiced_cost, jump_cost, switch_cost; /* each finite, in [0, 16] */
  int32_t max_jump_cents;                      /* in [0, 12000] */
} mx_f0_decode_params;
/* {0.3f, 0.1f, 0.5f, 1200} */
void mx_f0_decode_params_default(mx_f0_decode_params *p);
/* count frames: d_track (rms), d_cands (4 per frame) -> d_out (may alias d_track) and d_state (may be NULL), all in HBM.
 * p NULL: the defaults.  Asynchronous on the context's stream.  Work memory (2 bytes per frame and 202 per chunk) belongs
 * to the context, kept between calls, released by mx_ctx_release_scratch; MX_ERR_NOMEM when it cannot be had.
 * MX_ERR_INVALID for a cost outside [0, 16] or not finite, or max_jump_cents outside [0, 12000]. */
int mx_f0_decode_dev(mx_ctx *ctx, const mx_f0 *d_track, const mx_f0_cand *d_cands, int64_t count,
                     const mx_f0_decode_params *p, mx_f0 *d_out, uint8_t *d_state);
/* Same, host pointers (state may be NULL; out may alias track).  Blocks. */
int mx_f0_decode(mx_ctx *ctx, const mx_f0 *track, const mx_f0_cand *cands, int64_t count, const mx_f0_decode_params *p,
                 mx_f0 *out, uint8_t *state);
/* Candidates and decode in one call: the decoded track of frames [first_frame, first_frame + count), host output. */
int mx_f0_track_decoded(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                        float fmin, float fmax, float threshold, const mx_f0_decode_params *p, mx_f0 *out);
/* Frames per chunk of the decode (0: the default, about sqrt(count) / 3).  For tests, like mx_pv_set_chunk_frames: the output
 * does not depend on it. */
int mx_f0_decode_set_chunk(mx_ctx *ctx, int64_t frames);

/* Notes (host, double).  A frame is voiced when tau > 0, aperiodicity < threshold and rms >= rms_floor.  A note is a
 * maximal run of voiced frames; a new run starts before frame f when |m_f - m_{f-1}| > max_jump or
 * |m_f - median(m over the run so far)| > max_dev (m = the frame's note; the median of an even count is the mean of the
 * two middle values).  Runs shorter than min_frames (>= 2) are dropped. */
typedef struct mx_note_params {
  float threshold, rms_floor;
  double max_jump, max_dev;
  int32_t min_frames;
} mx_note_params;
typedef struct mx_note {
  int32_t start_sample, end_sample; /* centres of the run's first and last frames */
  int32_t first_frame, frames;      /* frame index of the run's first frame (track[0] is frame first_frame), run length */
  double note;                      /* the run's median note */
  float aperiodicity;               /* the run's mean */
  float spread;                     /* max |m_f - note| */
} mx_note;
/* {0.15, 1e-3, 0.5, 0.75, 8} */
void mx_note_params_default(mx_note_params *p);
/* track: count records of frames first_frame .. first_frame+count-1 (hop samples apart).  *notes is library-allocated
 * (free with mx_free; NULL when there are none). */
int mx_detect_notes(const mx_f0 *track, int64_t count, int sampleRate, int hop, int64_t first_frame,
                    const mx_note_params *params, mx_note **notes, int64_t *nnotes);
/* Correction markers: each note moves to T, the nearest integer note whose pitch class T mod 12 (A = 0) is set in
 * scale_mask (bits 0..11; 0 = all twelve), ties to the lower note; bend b = strength * (T - note), strength in [0, 1].
 * out (2*count markers): {start_sample, note, 0, b}, {end_sample, note, 0, b} per note — strictly increasing samples,
 * dTime 0 (the time map stays the identity).  The notes must be in order and not overlap. */
int mx_correction_markers(const mx_note *notes, int64_t count, double strength, int scale_mask, mx_marker *out);

/* ---- Formant-preserving PSOLA rendering driven by the f0 track (BUILD-DEFINED; restated in f64 by tests/psola_ref.py) ----
 * The granular resampler and the phase vocoder both move the spectral envelope with the pitch.  Time-domain
 * pitch-synchronous overlap-add does not: two-period Hann grains are cut from the source at the spacing the f0 track gives
 * and laid down again at that spacing divided by the pitch ratio; each grain keeps its shape, so the formants stay.  It wants
 * a monophonic, tracked take.  Markers steer it as they steer mx_pv_render (same time map, same bend, same output length).
 *
 * Inputs: the audio (n samples at sr); a track of count = mx_frame_count(n, hop) mx_f0 records, frame h centred on h*hop,
 * plain or decoded; the parameters below; the markers, sorted.  All planning arithmetic is host binary64, no contraction.
 *   voicing   frame h is voiced by mx_detect_notes' rule (tau > 0, aperiodicity < threshold, rms >= rms_floor) and, in
 *             addition, a finite period in [2, MX_PSOLA_MAX_HALF]; any other record is unvoiced.
 *   P(x)      for a source position x, from frame h = clamp(floor(x/hop + 1/2), 0, count-1): (double)period_h if the frame
 *             is voiced, else unvoiced_period U; voiced(x) is read the same way.
 *   analysis  a_0 = 0, p_m = P(a_m), v_m = voiced(a_m), a_{m+1} = a_m + p_m, while a_m - p_m < n (the last window reaches
 *             past the end of the file: the tail keeps its full window sum).
 *   synthesis L = mx_pv_render_length(n, sr, markers).  s_0 = 0; src_k = max(time2sample(s_k/sr), 0); m(k) = the analysis
 *             mark nearest to src_k (the last mark beyond it; ties: the HIGHER index — time2sample truncates, and at a
 *             period of 2 the identity map lands halfway between two marks); H_k = p_{m(k)};
 *             r_k = clamp(2^((double)time2pitchbend(s_k/sr) / 12), 1/2, 2) if v_{m(k)}, else 1 (unvoiced sound keeps its
 *             spacing; a bend that is not a number counts as the lower clamp); s_{k+1} = s_k + H_k/r_k; grains while
 *             s_k - H_k < L.  Time-stretching falls out of src_k: marks are repeated or skipped.
 *   record    one mx_psola_grain per k (below).  A fraction that rounds to 1.f as binary32 moves into its integer.
 *             centre is non-decreasing in k and can repeat (H = 2 at r = 2: a spacing of exactly 1, the least the clamps
 *             allow); centre + centre_frac is strictly increasing.
 *   output    for sample i, over the grains with out_lo <= i < out_hi IN ASCENDING k, two binary32 sums:
 *               u = ((float)(i - centre) - centre_frac) * inv_half, the grain skipped if |u| >= 1;
 *               w = 0.5 + 0.5 cos(pi u);  x = (1 - src_frac) * audio[i + src_off] + src_frac * audio[i + src_off + 1]
 *               (zeros outside the file; the resampler's form, no contraction);  S += w * x, W += w;
 *             y_i = W > 0 ? S / max(W, 0.25f) : 0;  int16: the clamped form of "PCM conversions", as in the phase vocoder.
 *             A source sample that is NaN or Inf makes exactly the outputs not finite that read it as either tap of a
 *             grain (whatever the weights); every other output keeps its bytes.
 *             Dividing by the window sum makes a zero-bend, identity-map render the input and keeps the level of a raised
 *             pitch; the floor lets the tails taper where a lowered pitch leaves gaps.  The order is fixed, so the result
 *             does not depend on how the kernel tiles the output. */
#define MX_PSOLA_MAX_HALF 2048
typedef struct mx_psola_params {
  float threshold, rms_floor; /* the voicing rule's; finite */
  float unvoiced_period;      /* U, samples, in [32, MX_PSOLA_MAX_HALF] */
} mx_psola_params;
typedef struct mx_psola_grain {
  int32_t out_lo, out_hi; /* outputs i in [out_lo, out_hi): max(0, floor(s-H)+1) .. min(L, ceil(s+H)) */
  int32_t src_off;        /* floor(a_m - s): the grain reads the source at i + src_off (+1) */
  float src_frac;         /* (a_m - s) - src_off, in [0, 1) */
  int32_t centre;         /* floor(s) */
  float centre_frac;      /* s - centre */
  float inv_half;         /* 1 / H */
  int32_t mark;           /* m(k), for inspection */
} mx_psola_grain;
/* {0.15f, 1e-3f, 256.f} */
void mx_psola_params_default(mx_psola_params *p);
/* The grain records of a render and its length (host).  params NULL: the defaults.  *grains is library-allocated (free
 * with mx_free).  MX_ERR_INVALID for count != mx_frame_count(n, hop), hop outside [1, 16384], sr <= 0, U out of range or a
 * parameter that is not finite, n > INT32_MAX - 2*MX_AUDIO_PAD, and whatever mx_pv_render_length refuses of the markers. */
int mx_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                  const mx_marker *markers, int nmarkers, mx_psola_grain **grains, int64_t *ngrains, int64_t *nsamples);
/* The overlap-add over records in HBM; d_pcm_f32 / d_pcm_i16: nsamples each in HBM (either may be NULL).  Asynchronous on
 * the context's stream.  nsamples == 0: nothing; ngrains == 0: the outputs are zero-filled.
 * PRECONDITION (not checked on the device — mx_psola_synth, the host-pointer entry point, does check it): the records are
 * what mx_psola_plan makes for this audio: centre + centre_frac strictly increasing, 0 <= out_lo <= out_hi <= nsamples,
 * every window inside centre +- 2049, inv_half finite and >= 1/2048, both fractions in [0, 1), every source index
 * i + src_off (+1) inside [-MX_AUDIO_PAD, n + MX_AUDIO_PAD - 1].  Records that break it give wrong samples and nothing
 * worse: the kernel clamps every source index into the padded buffer, every scan to [0, ngrains), and stores nothing
 * outside [0, nsamples). */
int mx_psola_synth_dev(mx_ctx *ctx, const mx_audio *a, const mx_psola_grain *d_grains, int64_t ngrains, int64_t nsamples,
                       float *d_pcm_f32, int16_t *d_pcm_i16);
/* Same, host pointers.  Checks every record against the precondition above and returns MX_ERR_INVALID before any launch,
 * the outputs untouched.  Blocks. */
int mx_psola_synth(mx_ctx *ctx, const mx_audio *a, const mx_psola_grain *grains, int64_t ngrains, int64_t nsamples,
                   float *pcm_f32_out, int16_t *pcm_i16_out);
/* Plan and synthesis in one call: mx_pv_render_length(n, sr, markers) samples each (host, either may be NULL).  Blocks. */
int mx_psola_render(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                    const mx_psola_params *params, const mx_marker *markers, int nmarkers, float *pcm_f32_out,
                    int16_t *pcm_i16_out);
/* Same, the PCM stays in HBM (the track and the markers are host arrays).  Blocks until the device is done with the
 * records it uploaded. */
int mx_psola_render_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                        const mx_psola_params *params, const mx_marker *markers, int nmarkers, float *d_pcm_f32,
                        int16_t *d_pcm_i16);

/* ---- Independent formant shift on the PSOLA renderer (BUILD-DEFINED; restated in f64 by tests/psola_formant_ref.py) ----
 * PSOLA pins the spectral envelope; this moves it on purpose, by some semitones, while the note stays where the grain
 * spacing puts it.  A grain that is read from the source at step phi instead of 1, inside the same output window and at the
 * same output spacing, has its envelope scaled by phi; its pitch is still what the spacing says.  Marks, spacing, voicing,
 * r_k and the output length are exactly mx_psola_plan's: the same k, the same out_lo / out_hi / centre / centre_frac /
 * inv_half.
 *   curve     npoints control points {sample, semitones}; sample is a position in the SOURCE.  Samples strictly increasing,
 *             semitones finite, anything else MX_ERR_INVALID.  F(x) in binary64: the first point's value for x below its
 *             sample, the last point's from its sample on, and between points j and j+1 (sample_j <= x < sample_{j+1})
 *             F(x) = y_j + (x - sample_j) * (y_{j+1} - y_j) / (sample_{j+1} - sample_j), evaluated in that order; no
 *             points: F = 0.
 *   step      for grain k, phi_k = clamp(exp2(F(a_{m(k)}) / 12), 1/2, 2) in binary64, a_{m(k)} the analysis mark the plan
 *             picks for the grain; voiced and unvoiced grains alike, so the timbre has no step at a voicing switch.
 *             step_k = (int)floor(phi_k * 65536 + 0.5), in [32768, 131072].  The Q16 step IS the definition, not an
 *             approximation of it: everything downstream is exact integer arithmetic, on the host and on the device.
 *   record    p0 = a_m - ((double)step / 65536.0) * (double)centre_frac, the source position of output sample `centre`
 *             (centre_frac the stored binary32 value, after its carry); q = (int64)floor(p0 * 65536.0 + 0.5);
 *             src_idx = q >> 16 (a floor), src_q = q & 65535.
 *   output    for sample i, over the grains in ascending k: u and w exactly as above;
 *               pos = (src_idx << 16) + src_q + step * (i - centre)   (|step * (i - centre)| < 2^29: no window reaches
 *               further than 2049 from its centre);  idx = pos >> 16;  f = (float)(pos & 65535) * 2^-16, exact;
 *               x = (1 - f) * audio[idx] + f * audio[idx + 1] (zeros outside the file, no contraction);
 *             S, W, the floor of 1/4 and the int16 conversion unchanged.
 * What follows from the definition (not bugs):
 *   - phi > 1 reads the source faster than it plays it, through linear interpolation and with no anti-alias filter: the
 *     granular resampler at a raised pitch does the same.
 *   - at phi = 2 every grain holds twice as many periods, and the render's pitch is an octave up (the reference render
 *     shows +12.0 st at formant +12).  The clamp is therefore an octave; the useful range is a few semitones.
 *   - the source reach grows to 2 * 2049 samples either side of a mark: still well inside MX_AUDIO_PAD. */
typedef struct mx_formant_point {
  int32_t sample;  /* position in the source */
  float semitones; /* envelope shift there */
} mx_formant_point;
typedef struct mx_psola_fgrain {
  int32_t out_lo, out_hi; /* as mx_psola_grain */
  int32_t src_idx;        /* floor of the source position of output sample `centre` */
  uint32_t src_q;         /* its fraction in Q16, < 65536 */
  int32_t centre;         /* as mx_psola_grain */
  float centre_frac;
  float inv_half;
  uint32_t step; /* Q16 source step per output sample, in [32768, 131072] */
} mx_psola_fgrain;
/* mx_psola_plan with the curve: one record per synthesis mark (npoints == 0: every step is 65536).  *fgrains is
 * library-allocated (free with mx_free).  MX_ERR_INVALID for what mx_psola_plan refuses and for a bad curve. */
int mx_psola_plan_formant(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                          const mx_marker *markers, int nmarkers, const mx_formant_point *points, int npoints,
                          mx_psola_fgrain **fgrains, int64_t *ngrains, int64_t *nsamples);
/* mx_psola_synth_dev over such records in HBM.  Asynchronous on the context's stream.
 * PRECONDITION (not checked on the device — mx_psola_synth_formant does check it): mx_psola_synth_dev's on the fields the two
 * records share, step in [32768, 131072], src_q < 65536, and every source index idx (+1) a window reaches inside
 * [-MX_AUDIO_PAD, n + MX_AUDIO_PAD - 1].  Records that break it give wrong samples and nothing worse, by the same clamps. */
int mx_psola_synth_formant_dev(mx_ctx *ctx, const mx_audio *a, const mx_psola_fgrain *d_fgrains, int64_t ngrains,
                               int64_t nsamples, float *d_pcm_f32, int16_t *d_pcm_i16);
/* Same, host pointers.  Checks every record and returns MX_ERR_INVALID before any launch, the outputs untouched.  Blocks. */
int mx_psola_synth_formant(mx_ctx *ctx, const mx_audio *a, const mx_psola_fgrain *fgrains, int64_t ngrains, int64_t nsamples,
                           float *pcm_f32_out, int16_t *pcm_i16_out);
/* Plan and synthesis in one call, as mx_psola_render / mx_psola_render_dev.  With npoints == 0 they ARE those: the plain
 * records, the plain kernel, the same bytes. */
int mx_psola_render_formant(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                            const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                            const mx_formant_point *points, int npoints, float *pcm_f32_out, int16_t *pcm_i16_out);
int mx_psola_render_formant_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                                const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                                const mx_formant_point *points, int npoints, float *d_pcm_f32, int16_t *d_pcm_i16);

/* ---- Onset detection and tempo-grid timing markers (BUILD-DEFINED; restated in f64 by tests/onset_ref.py) ----
 * mx_marker.dTime is the editor's time-warp handle and every renderer follows it; this finds where events start and
 * computes the dTime values that put them on a tempo grid.  The reference has no detector.
 *
 * Onset strength.  The detector has a transform of its own (the reference window of the magnitude rows is rectangular with
 * an exponential tail: a steady tone's bins ripple from frame to frame, and spectral flux over them peaks every ~11 frames
 * on a held note).  For frame h of the bulk indexing (h < mx_frame_count(n, hop)), centred on sample h*hop:
 *   x_j = audio[h*hop - 512 + j], j < 1024, zeros outside the file;  w_j = 0.5 - 0.5 cos(2 pi j / 1024);
 *   X_k = the 1024-point DFT of w x;  m_k = |X_k| / 512;  c_h[k] = log1pf(compress * m_k), in f32;
 *   flux_h = sum_{k = kmin..kmax} max(0, c_h[k] - c_{h-lag}[k]), with c_h = 0 for h < 0;
 *   kmin = max(1, ceil(fmin * 1024 / sr)), kmax = min(511, floor(fmax * 1024 / sr)); fmax = 0 means sr / 2.
 * The level matters by design: log1p(compress * m) is linear in m for a quiet take, so a quiet take has small flux (at a
 * tenth of the level the curve is not a tenth, and the picker's additive term delta does not scale).  A frame of zeros has
 * c = 0; silence has flux exactly 0.  max(0, d) keeps a NaN d: a frame whose 1024 samples hold a NaN has flux NaN, and so
 * has frame h+lag, which is measured against it; a frame that holds +Inf or -Inf has a flux that is not finite.  Every other
 * frame keeps the bytes it has without the bad sample; the picker and the tempo estimate count values that are not finite as 0.
 * Accuracy: the f32-versus-f64 yardstick of the tests, |error| <= 2e-5 * max_h flux_h + 1e-9, is claimed for compress * level up
 * to 1e4, level the take's largest |sample| (compress <= 1e4 for a take at full scale).  log1p has slope compress at m = 0, so above
 * that the transform's f32 noise on the quiet bins (about 1e-7 of the frame's peak) stops being small against the curve: at
 * compress = 1e6 the tests allow 1.64 x the yardstick on a take with a 1e-4 noise floor.
 * The per-frame reduction has one fixed order, so frame h's value depends on nothing but its samples and frame h-lag's:
 * the same bytes whatever the launch split (first_frame, count) or the run length a walker takes.  No spectrum goes to HBM:
 * the launch writes 4 bytes per frame. */
typedef struct mx_onset_flux_params {
  float compress; /* finite, in (0, 1e6] */
  int32_t lag;    /* in [1, 4] */
  float fmin, fmax; /* Hz, finite, >= 0; fmax == 0: sr / 2 */
} mx_onset_flux_params;
/* {100.f, 1, 0.f, 0.f} */
void mx_onset_flux_params_default(mx_onset_flux_params *p);
/* Frames [first_frame, first_frame + count) -> d_flux (count floats in HBM).  Asynchronous on the context's stream.
 * params NULL: the defaults.  MX_ERR_INVALID, before any launch, for sr <= 0, hop outside [1, 16384], frames outside the
 * file, a parameter out of range or an empty band. */
int mx_onset_flux_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                      const mx_onset_flux_params *params, float *d_flux);
/* Same, host output through the context's staging buffers.  Blocks. */
int mx_onset_flux(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                  const mx_onset_flux_params *params, float *flux_out);

/* Peak picking (host, binary64, exact).  o_i = flux[i] as a double, 0 where it is not finite; windows are clipped to
 * [0, count).  Index f, taken in ascending order, is an onset when all three hold:
 *   o_f > o_g for every g in [f - pre_max, f) and o_f >= o_g for every g in (f, f + post_max] (a plateau: its first index);
 *   o_f >= ratio * mean(o over [f - pre_avg, f + post_avg]) + delta, the mean summed in ascending order and divided by the
 *   clipped window's length;
 *   f - (the previous accepted index) > wait.
 * Defaults {3, 3, 25, 1, 8, 2.0, 1.0}: values that separate tests/onset_ref.py's synthetic signals (notes with 5 and 30 ms
 * attacks, a legato, a vibrato, steady noise, clicks) with every decision at least 0.9 flux units from its threshold.  Nobody
 * has tuned them on recordings.  The multiplicative term is what keeps steady noise quiet; delta what keeps a near-silent
 * take quiet. */
typedef struct mx_onset_pick_params {
  int32_t pre_max, post_max, pre_avg, post_avg, wait; /* each in [0, 4096] */
  double ratio, delta;                                /* finite, >= 0 */
} mx_onset_pick_params;
typedef struct mx_onset {
  int32_t sample; /* frame * hop, absolute */
  int32_t frame;  /* first_frame + f */
  float strength; /* o_f */
  float margin;   /* o_f - threshold */
} mx_onset;
void mx_onset_pick_params_default(mx_onset_pick_params *p);
/* flux[i] is frame first_frame + i.  params NULL: the defaults.  *out is library-allocated (free with mx_free).
 * MX_ERR_INVALID for a parameter out of range, hop < 1 or frame centres beyond int32 samples. */
int mx_onset_pick(const float *flux, int64_t count, int hop, int64_t first_frame, const mx_onset_pick_params *params,
                  mx_onset **out, int64_t *nout);
/* Flux over the whole file and the picks from it.  Either params may be NULL.  Blocks. */
int mx_onsets_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_onset_flux_params *flux_params,
                     const mx_onset_pick_params *pick_params, mx_onset **out, int64_t *nout);

/* Timing markers (host, binary64, exact).  Anchors (source samples, e.g. mx_onset.sample) move towards the lines of a
 * tempo grid; the markers returned make every renderer play them there.
 *   anchors   strictly increasing, in [0, n); anchors at sample <= 0 are dropped (a marker at sample 0 has no span).
 *   targets   g = 60 / (bpm * division), t_i = a_i / sr;  q_i = floor((t_i - offset) / g + 0.5);
 *             d_i = offset + q_i * g - t_i, 0 where |d_i| > max_shift (such an anchor still pins its time);
 *             U_i = t_i + strength * d_i.
 *   monotone  T_{-1} = 0, a_{-1} = 0;  span = (a_i - a_{i-1}) / sr;
 *             T_i = T_{i-1} + clamp(U_i - T_{i-1}, span / max_stretch, span * max_stretch).
 *   warp      W(s): piecewise linear through (0, 0) and (a_i, T_i), in sample2Time's form
 *             T_{i-1} + (s - a_{i-1}) * (T_i - T_{i-1}) / (a_i - a_{i-1}); the natural rate behind the last anchor.
 *   output    one marker per sample in anchors U base samples, sorted, with
 *             dTime_j = (W(s_j) - W(s_{j-1})) - (s_j - s_{j-1}) / sr  (s_{-1} = 0);  |dTime_j| < 1e-10 s is written as 0: the
 *             rounding residue of the two differences, not a shift — strength 0 gives the identity map exactly.
 * base (may be NULL) is what mx_correction_markers gives: samples strictly increasing in [1, n), every dTime == 0.  A
 * marker on a base sample keeps that marker's note and pitchBend.  An inserted marker gets pitchBend by linear interpolation
 * in source samples through (0, 0), the base points and (n - 1, 0) — time2PitchBend's own curve, so the bend over the source
 * is unchanged — and note interpolated between its neighbours, the nearer end's note outside them, 0 with no base.
 * *out is library-allocated (free with mx_free).  MX_ERR_INVALID for anchors or base out of order or range, a base dTime
 * != 0 or a bend / note that is not finite, a parameter outside its range below, sr <= 0 or n outside [1, INT32_MAX]. */
typedef struct mx_timing_params {
  double bpm;         /* [30, 250], the reference's Tempo slider; default 120 */
  int32_t division;   /* grid lines per beat, [1, 64]; default 4 */
  double offset;      /* time of a grid line, seconds, finite; default 0 */
  double strength;    /* [0, 1]; default 1 */
  double max_shift;   /* seconds, >= 0, finite; default 0.1 */
  double max_stretch; /* [1, 4]; default 2 */
} mx_timing_params;
void mx_timing_params_default(mx_timing_params *p);
int mx_timing_markers(const int32_t *anchors, int64_t nanchors, int64_t n, int sampleRate, const mx_timing_params *params,
                      const mx_marker *base, int nbase, mx_marker **out, int64_t *nout);

/* ---- Tempo and grid-offset estimation (BUILD-DEFINED; restated by tests/tempo_ref.py) ----
 * mx_timing_params.bpm and .offset from the onset-strength curve itself: the one link of the timing chain (flux -> onsets ->
 * markers -> render) that was fed by hand.  The reference has a Tempo slider and no estimator.  The definition is
 * tolerance-free — f32 products, a binary64 running sum, integer positions — so the device, the host and numpy give the same
 * bytes.
 *
 * Smoothed curve.  Input: count flux values o_f.  z_f = o_f, 0 where o_f is not finite, 0 outside [0, count).  Half-width W
 * in [0, 32]; h_d = (float)(0.5 + 0.5 cos(pi d / (W + 1))), the cosine in binary64.
 *   e_f = sum_{d = -W..W} h_|d| * z_{f+d}, in f32, from 0.f in ascending d, each product rounded before it is added.
 * W = 0 is the sanitising copy.  The output must not overlap the input.
 *
 * Comb job {first, frames, period_q16}: frames >= 1, [first, first + frames) inside [0, count), period_q16 a beat period in
 * frames as Q16 in [2 * 65536, 4096 * 65536] — the Q16 value is the definition.  Phases phi = 0 .. nph - 1,
 * nph = ceil(period_q16 / 65536).  For a phase, positions in int64:
 *   start = (first + phi) << 16, lim = (first + frames - 1) << 16;  J = 0 if start > lim, else (lim - start) / period_q16 + 1;
 *   for j = 0 .. J - 1 ascending: pos = start + j * period_q16, idx = pos >> 16, fr = (float)(pos & 65535) * 2^-16 (exact),
 *     x = (1 - fr) * e[idx] + fr * e[min(idx + 1, count - 1)] in f32 (the resampler's form, products rounded before the sum),
 *     S += (double)x;
 *   score_phi = (float)(S / (double)J), 0.f when J = 0.
 * The record: score = the maximum over the phases, phase = the lowest phi that attains it, prev / next = the scores of phases
 * (phi -+ 1) mod nph.  A record depends on nothing but the curve and its job: the same bytes whatever the job list, its order,
 * the launch split or the thread mapping.  (The curve is meant to be finite — mx_tempo_smooth's output is; with a NaN in a
 * job's reach its record is some phase's, not a fault.) */
typedef struct mx_comb_job {
  int32_t first, frames;
  uint32_t period_q16;
} mx_comb_job;
typedef struct mx_comb {
  float score;
  int32_t phase;
  float prev, next;
} mx_comb;
/* Estimate (host, binary64, libm, no contraction).  fr = sr / hop frames per second.
 *   candidates  bpm_c = bpm_max * exp2(-c / per_octave), c = 0, 1, .. while bpm_c >= bpm_min;
 *               period_c = (uint32)floor(60 * fr / bpm_c * 65536 + 0.5); MX_ERR_INVALID if one leaves the Q16 range.
 *   windows     [w * stride_frames, w * stride_frames + window_frames) for every w that fits; count < window_frames: [0, count).
 *   coarse      one job per (window, candidate), T[w][c] its score;  prior_c = exp(-0.5 (log2(bpm_c / prior_bpm) / prior_octaves)^2);
 *               A_c = (sum_w T[w][c], binary64, ascending w) * prior_c;  c* = the lowest c that attains max A;  the anchor =
 *               the lowest w that attains max T[w][c*].  The window curve: per window the candidate that is the lowest argmax of
 *               T[w][c] * prior_c, as {first_frame + w * stride_frames, frames, (float)(60 * fr * 65536 / period), T[w][c]}.
 *   refinement  the grid must hold over ever longer stretches: segment and resolution grow together.  p = period_c*,
 *               step = max(1, (int)(p * (exp2(1 / per_octave) - 1) / 8)), L = the anchor's length, centre = its first + L / 2.
 *               Per level: len = min(L, count), first = clamp(centre - L / 2, 0, count - len); jobs over [first, first + len)
 *               with periods p + k * step, k = -12 .. 12, those outside the Q16 range dropped; best = the highest score, then
 *               the smallest |k|, then the lower k.  The first level's best score is the base.  A later level whose best score
 *               < lock_ratio * base ends the refinement with the previous level's result.  Otherwise p = the best period and
 *               {first, len, record} are kept; the refinement ends if len == count, else L = 8 L, step = max(1, step / 8).
 *   result      from the last kept level: g = (p / 65536) / fr, bpm = 60 / g;  delta = 0.5 (prev - next) / (prev - 2 score + next)
 *               clamped to +-0.5, 0 unless that curvature is < 0;  offset = fmod((first_frame + first + phase + delta) / fr, g),
 *               moved into [0, g);  score = the record's;  clarity = score / the mean of e (summed in binary64, ascending; 0 unless that mean is > 0);
 *               locked_frames = len;  levels = the number of levels kept.
 * An empty curve, or one whose every e_f is 0, is not an error: bpm 0, offset 0, score 0, clarity 0, locked_frames 0, levels 0
 * and an empty window curve.
 * What follows from the definition (not bugs):
 *   - the estimate is octave-ambiguous and the prior decides: 85 bpm at division 4 and 170 bpm at division 2 are the same grid
 *     lines.  The refinement follows the curve, so bpm can end a little outside [bpm_min, bpm_max];
 *   - clarity ~ 1 means no pulse was found: every phase of a steady curve scores its mean (steady noise gives 1.07 in
 *     tests/tempo_ref.py, the synthetic takes 7 to 16). */
typedef struct mx_tempo_params {
  double bpm_min, bpm_max;  /* inside [30, 250], bpm_min < bpm_max; default 30, 250 */
  int32_t per_octave;       /* candidates per octave, [8, 128]; default 64 */
  int32_t smooth;           /* W, [0, 32]; default 4 */
  int32_t window_frames;    /* coarse window length, [64, 65536]; default 2048 */
  int32_t stride_frames;    /* window stride, [1, window_frames]; default 512 */
  double prior_bpm;         /* centre of the tempo prior, finite, > 0; default 120 */
  double prior_octaves;     /* width of the tempo prior, finite, > 0; default 1 */
  double lock_ratio;        /* where refinement stops, [0, 1]; default 0.5 */
} mx_tempo_params;
typedef struct mx_tempo {
  double bpm, offset; /* beats per minute; the time of a beat, seconds, in [0, 60 / bpm) */
  float score, clarity;
  int64_t locked_frames;
  int32_t levels;
} mx_tempo;
typedef struct mx_tempo_window {
  int32_t first_frame, frames;
  float bpm, score;
} mx_tempo_window;
void mx_tempo_params_default(mx_tempo_params *p);
/* d_flux -> d_out (count floats each, in HBM, not overlapping).  Asynchronous on the context's stream.  MX_ERR_INVALID for
 * width outside [0, 32], count < 0 or beyond INT32_MAX, a null pointer with count > 0, overlapping ranges. */
int mx_tempo_smooth_dev(mx_ctx *ctx, const float *d_flux, int64_t count, int width, float *d_out);
/* Same, host pointers through the context's tempo work memory.  Blocks. */
int mx_tempo_smooth(mx_ctx *ctx, const float *flux, int64_t count, int width, float *out);
/* One record per job, d_out[i] for d_jobs[i].  Asynchronous on the context's stream.
 * PRECONDITION (not checked on the device — mx_tempo_comb does check it): every job as defined above.  Jobs that break it
 * give wrong numbers and nothing worse: every index is clamped into [0, count - 1], nph to 4096, J to count, and nothing is
 * stored outside the job's own record. */
int mx_tempo_comb_dev(mx_ctx *ctx, const float *d_curve, int64_t count, const mx_comb_job *d_jobs, int64_t njobs, mx_comb *d_out);
/* Same, host pointers.  Checks every job and returns MX_ERR_INVALID before any launch, the output untouched.  Blocks. */
int mx_tempo_comb(mx_ctx *ctx, const float *curve, int64_t count, const mx_comb_job *jobs, int64_t njobs, mx_comb *out);
/* The estimate from a host flux curve; flux[i] is frame first_frame + i (>= 0, first_frame + count <= INT32_MAX).  p NULL: the
 * defaults.  windows may be NULL; otherwise *windows is library-allocated (free with mx_free), *nwindows its length.  Every
 * parameter out of its range, sr <= 0, hop outside [1, 16384] or a candidate period outside the Q16 range: MX_ERR_INVALID
 * before any launch.  Blocks. */
int mx_tempo_from_flux(mx_ctx *ctx, const float *flux, int64_t count, int sampleRate, int hop, int64_t first_frame,
                       const mx_tempo_params *p, mx_tempo *out, mx_tempo_window **windows, int64_t *nwindows);
/* The whole file: mx_onset_flux_dev into the context's work memory, the smoothing and the comb launches there; what comes back
 * is the smoothed curve once (4 bytes per frame, for the mean behind clarity) and the job records.  fp / p NULL: the defaults.
 * The work memory (two curves; jobs and records in the context's job buffers) is the context's, kept between calls, released by
 * mx_ctx_release_scratch; MX_ERR_NOMEM when it cannot be had, nothing of the set that failed left allocated.  Blocks. */
int mx_tempo_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_onset_flux_params *fp,
                    const mx_tempo_params *p, mx_tempo *out, mx_tempo_window **windows, int64_t *nwindows);

/* ---- Sibilant detection, protection and balance (BUILD-DEFINED; restated in f64 by tests/sibilant_ref.py) ----
 * The pitch chain and the timing chain treat every frame that is not a tracked note alike.  Sibilants ("s", "sh", "z", "ch",
 * "t" bursts) are the one class of such frames an editor must know: a formant shift moves them with the note (the lisp), and
 * "sibilant balance" is the control next to the formant knob.  The YIN record cannot find them (aperiodicity separates voiced
 * from unvoiced, not "s" from a breath); the separation is spectral.  The reference has nothing of the kind.
 *
 * Features.  The onset detector's frame: for frame h of the bulk indexing (h < mx_frame_count(n, hop)),
 *   x_j = audio[h*hop - 512 + j], j < 1024, zeros outside the file;  w_j = 0.5 - 0.5 cos(2 pi j / 1024);
 *   X_k = the 1024-point DFT of w x;  P_k = (|X_k| / 512)^2, in f32;  ks = clamp(ceil(split_hz * 1024 / sr), 1, 512);
 *   low = sum_{k = 1..ks-1} P_k;  high = sum_{k = ks..511} P_k;
 *   centroid = sum_{k = 1..511} k P_k / (low + high), in bins, 0 where low + high is 0;
 *   zero_crossings = the number of j in 0..1022 with (x_j < 0) != (x_{j+1} < 0), on the raw samples: zeros, -0 and NaN count as
 *   "not negative", so silence and the pad give 0.
 * Bin 0 and bin 512 belong to neither sum.  ks = 1 makes low 0 for every frame, ks = 512 makes high 0.  The three sums have one
 * fixed order, so a record depends on its frame's samples alone: the same bytes whatever first_frame, count or the run
 * length a walker takes.  The launch writes 16 bytes per frame and no spectrum. */
typedef struct mx_sib_feat {
  float low, high;
  float centroid; /* bins of 1024: Hz = centroid * sr / 1024 */
  int32_t zero_crossings;
} mx_sib_feat;
typedef struct mx_sib_feature_params {
  float split_hz; /* finite, in (0, sr / 2] */
} mx_sib_feature_params;
/* {3500.f} */
void mx_sib_feature_params_default(mx_sib_feature_params *p);
/* Frames [first_frame, first_frame + count) -> d_feat (count records in HBM).  Asynchronous on the context's stream.
 * params NULL: the defaults.  MX_ERR_INVALID, before any launch, for sr <= 0, hop outside [1, 16384], frames outside the
 * file or split_hz out of range. */
int mx_sib_features_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                        const mx_sib_feature_params *params, mx_sib_feat *d_feat);
/* Same, host output through the context's staging buffers.  Blocks. */
int mx_sib_features(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                    const mx_sib_feature_params *params, mx_sib_feat *feat_out);

/* Segments (host, binary64, exact).  Per frame s = (double)low + (double)high; where s is finite and > 0,
 * level = sqrt(s) and share = (double)high / s, else both are 0.
 *   a run opens at a frame with level >= level_floor, share >= share_on and zero_crossings >= zc_min, and continues while
 *   level >= level_floor and share >= share_off (the frame that fails is not part of it);
 *   runs with at most merge_gap frames between them become one (the frames between them included);
 *   then runs of fewer than min_frames frames are dropped.
 * start_sample / end_sample are the centres of the run's first and last frame; share is the mean of the run's frames' shares
 * (binary64, ascending), level the maximum of their levels.  Runs come out in order and do not overlap.
 * Defaults {0.6, 0.4, 1e-3, 64, 2, 6}: values that separate tests/sibilant_ref.py's synthetic take (vowels, "s", "sh", a soft
 * "s", a breath, a click).  Nobody has tuned them on recordings.  Steady white noise IS a sibilant by this definition (more
 * than half of its energy lies above 3.5 kHz): one segment over the whole take. */
typedef struct mx_sibilant_params {
  double share_on, share_off; /* in [0, 1], share_off <= share_on */
  double level_floor;         /* finite, >= 0 */
  int32_t zc_min;             /* [0, 1023] */
  int32_t merge_gap;          /* frames, [0, 4096] */
  int32_t min_frames;         /* [1, 4096] */
} mx_sibilant_params;
typedef struct mx_sibilant {
  int32_t start_sample, end_sample; /* centres of the first and the last frame, absolute */
  int32_t first_frame, frames;
  float share, level;
} mx_sibilant;
void mx_sibilant_params_default(mx_sibilant_params *p);
/* feat[i] is frame first_frame + i.  params NULL: the defaults.  *out is library-allocated (free with mx_free).
 * MX_ERR_INVALID for a parameter out of range, hop < 1 or frame centres beyond int32 samples. */
int mx_sibilants(const mx_sib_feat *feat, int64_t count, int hop, int64_t first_frame, const mx_sibilant_params *params,
                 mx_sibilant **out, int64_t *nout);
/* Features over the whole file and the segments from them.  Either params may be NULL.  Blocks. */
int mx_sibilants_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_sib_feature_params *feature_params,
                        const mx_sibilant_params *params, mx_sibilant **out, int64_t *nout);

/* Spans (what protection and balance share).  Sibilants: 0 <= start_sample <= end_sample <= n - 1, each start_sample above
 * the end_sample before it; n in [1, INT32_MAX]; ramp_samples >= 1 (and <= 2^30).  A sibilant whose start_sample - ramp is
 * <= the end_sample + ramp of the span before it joins that span.  A span is {lo, start, end, hi}: start the first
 * sibilant's start_sample, end the last one's end_sample (the core), lo = max(start - ramp, 0), hi = min(end + ramp, n - 1).
 * A span gives the points lo (if lo < start), start, end (if end > start), hi (if hi > end): strictly increasing, and
 * strictly above the span before.
 *
 * Protection (host, binary64).  F: the curve of mx_psola_plan_formant.  The result keeps every point of F outside all
 * [lo, hi], and per span the points {lo, (float)F(lo)}, {start, 0}, {end, 0}, {hi, (float)F(hi)}: it equals F outside the
 * spans (to the binary32 rounding of F(lo), F(hi)), is exactly 0 st on [start, end] and linear on the ramps.
 * mx_psola_plan_formant accepts it as it is.  No points: no points.  No sibilants: the input.  *out is library-allocated.
 * MX_ERR_INVALID for a bad curve, sibilants out of order or range, ramp_samples < 1. */
int mx_formant_protect(const mx_formant_point *points, int npoints, const mx_sibilant *sibs, int64_t nsib, int32_t ramp_samples,
                       int64_t n, mx_formant_point **out, int64_t *nout);

/* Balance.  The gain is applied to the SOURCE, before any renderer: the granular resampler, the phase vocoder and PSOLA render
 * the result untouched, and the f0 track of the original take stays valid (periods do not depend on level).
 *   points    {sample, amp}: samples strictly increasing, amp finite and > 0 (the grain scan's zero crossings stay put).
 *   gain      g(i) in binary64: the first point's amp for i below its sample, the last point's from its sample on, and for
 *             s0 <= i < s1 between two points  g = a0 + (a1 - a0) * ((double)(i - s0) / (double)(s1 - s0)), no contraction.
 *   output    out_i = (float)((double)x_i * g(i)).  The host, the device and numpy give the same bytes. */
typedef struct mx_gain_point {
  int32_t sample;
  float amp;
} mx_gain_point;
/* A new audio object (free with mx_audio_free) of a's length with zeroed pads, like an upload; a is untouched.  npts == 0
 * copies.  Checks every point and returns MX_ERR_INVALID before any launch, *out untouched.  Blocks. */
int mx_audio_gain(mx_ctx *ctx, const mx_audio *a, const mx_gain_point *points, int64_t npts, mx_audio **out);
/* Same with the points in HBM.  Asynchronous on the context's stream (the points must stay until it has run).
 * PRECONDITION (not checked on the device — mx_audio_gain does check it): the points as defined above.  Points that break it
 * give wrong samples and nothing worse: nothing is stored outside samples [0, n) of the new object. */
int mx_audio_gain_dev(mx_ctx *ctx, const mx_audio *a, const mx_gain_point *d_points, int64_t npts, mx_audio **out);
/* Samples [first, first + count) of an audio object into host memory; the pads are readable: first >= -MX_AUDIO_PAD,
 * first + count <= n + MX_AUDIO_PAD.  Blocks. */
int mx_audio_download(mx_ctx *ctx, const mx_audio *a, int64_t first, int64_t count, float *host_out);
/* The points of a sibilant balance of db decibels (finite, in [-120, 40]): per span {lo, 1}, {start, A}, {end, A}, {hi, 1}
 * with A = (float)pow(10, db / 20) in binary64.  No sibilants: no points.  *out is library-allocated.  MX_ERR_INVALID as
 * mx_formant_protect, and for db out of range. */
int mx_sibilant_gain_points(const mx_sibilant *sibs, int64_t nsib, double db, int32_t ramp_samples, int64_t n,
                            mx_gain_point **out, int64_t *nout);

/* ---- Key, scale and tuning reference (BUILD-DEFINED; restated in f64 by tests/key_ref.py) ----
 * mx_correction_markers takes its scale from the caller and its grid from A = 440 Hz.  This section finds both in the audio:
 * the evidence is a chromagram of whatever the editor has loaded (the accompaniment or the mix says more about the key than a
 * monophonic f0 track), with a cheap host path from the detected notes for dry solo takes.  The reference has no detector.
 *
 * Chroma record.  Frame h of the bulk indexing (h < mx_frame_count(n, hop)) is centred on sample h*hop:
 *   x_j = audio[h*hop - 2048 + j], j < 4096, zeros outside the file;  w_j = 0.5 - 0.5 cos(2 pi j / 4096);
 *   X = the 4096-point DFT of w x;  m[k] = |X_k| / 1024 (a unit sine reads 1), in f32.
 *   band   kmin = max(2, ceil(fmin * 4096 / sr)), kmax = min(2046, floor(fmax * 4096 / sr)); kmin > kmax: MX_ERR_INVALID.
 *   peaks  bin k of the band is a peak when m[k] > m[k-1], m[k] >= m[k+1] and m[k] >= max(floor, rel * max of m over the band).
 *   place  delta = (a - c) / (2 (a - 2b + c)) on a, b, c = ln m[k-1], ln m[k], ln m[k+1], clamped to [-1/2, 1/2]; 0 where the
 *          denominator is not negative or a logarithm is not finite.  f = (k + delta) * sr / 4096; cents = 1200 log2(f / 55).
 *   record forty floats.  A peak weighs m[k].  Columns 0..35: a pitch-class profile of 36 bins, bin b centred 100 b / 3 cents
 *          above A (A = 0 as everywhere here); the peak at p = (cents mod 1200) / (100 / 3) adds m[k] * max(0, 1 - d/2) / 2
 *          to every bin at circular distance d = |p - b| < 2 — a partition of unity, so columns 0..35 sum to column 38.
 *          Columns 36, 37: the tuning phasor sum m cos t, sum m sin t, t = 2 pi (cents/100 - rint(cents/100)).  Column 38: sum m.
 *          Column 39: the number of peaks.  Every sum runs over the frame's peaks in ascending k.
 * A silent frame gives forty exact zeros.  So does a frame that holds an Inf or a NaN sample, and one whose band maximum
 * overflows f32: a record is never Inf or NaN.  A record depends on its frame's samples alone: the same bytes whatever
 * first_frame, count, the launch split or the pinned run length.  The launch writes 160 bytes per frame and no spectrum.
 * Defaults {100, 5000, 1e-4, 0.05}: the relative floor sits above a Hann window's highest side lobe (-31.5 dB).  Untuned. */
typedef struct mx_chroma_rec {
  float pcp[36];
  float tune_cos, tune_sin;
  float weight;
  float peaks;
} mx_chroma_rec;
typedef struct mx_chroma_params {
  float fmin, fmax; /* Hz, finite, 0 < fmin <= fmax */
  float floor;      /* finite, >= 0 */
  float rel;        /* in [0, 1] */
} mx_chroma_params;
void mx_chroma_params_default(mx_chroma_params *p);
/* Frames [first_frame, first_frame + count) -> d_out (count records in HBM).  Asynchronous on the context's stream.
 * params NULL: the defaults.  MX_ERR_INVALID, before any launch, for sr <= 0, hop outside [1, 16384], frames outside the
 * file, a parameter out of range or an empty band. */
int mx_chroma_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                  const mx_chroma_params *params, mx_chroma_rec *d_out);
/* Same, host output through the context's staging buffers.  Blocks. */
int mx_chroma(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
              const mx_chroma_params *params, mx_chroma_rec *out);

/* Sums over frame windows.  Job j gives 40 binary64 values: column c summed over records first_frame .. first_frame +
 * frames - 1 in ascending order, each f32 widened first, a value that is not finite counting as 0.  No tolerance: the device,
 * the host form and tests/key_ref.py give the same bytes.  A job must lie inside the `count` records (first_frame >= 0,
 * frames >= 0, first_frame + frames <= count): mx_chroma_sum checks it (MX_ERR_INVALID before any launch); the device form
 * cannot see its jobs and clips them to the records instead — a bad job gives a wrong sum and nothing worse. */
typedef struct mx_chroma_job {
  int64_t first_frame, frames;
} mx_chroma_job;
int mx_chroma_sum_dev(mx_ctx *ctx, const mx_chroma_rec *d_chroma, int64_t count, const mx_chroma_job *d_jobs, int64_t njobs,
                      double *d_out);
int mx_chroma_sum(mx_ctx *ctx, const mx_chroma_rec *chroma, int64_t count, const mx_chroma_job *jobs, int64_t njobs, double *out);

/* Key (host, binary64, exact: tests/key_ref.py does the same operations in the same order).  From a 40-value sum S, values
 * that are not finite read as 0:
 *   tuning_cents = 100 / (2 pi) * atan2(S37, S36), in (-50, 50]; tuning_confidence = sqrt(S36^2 + S37^2) / S38; both 0 where S38
 *   is not positive or the phasor is 0.
 *   The twelve-class profile is read at that tuning: p[c] = sum_b S_b * max(0, 1 - d / 2), d the circular distance of b from
 *   (100 c + tuning) / (100 / 3) over 36 bins.  p is Pearson-correlated with the 24 rotations of the Krumhansl-Kessler profiles
 *     major 6.35 2.23 3.48 2.33 4.38 4.09 2.52 5.19 2.39 3.66 2.29 2.88,  minor 6.33 2.68 3.52 5.38 2.60 3.53 2.54 4.75 3.98 2.69 3.34 3.17
 *   in the order major before minor, then ascending tonic; the first candidate that attains the maximum wins.
 *   correlation: the winner's; clarity: the winner's minus the best of the other 23; scale_mask: the winner's seven diatonic
 *   classes (major 0 2 4 5 7 9 11, natural minor 0 2 3 5 7 8 10 above the tonic) in mx_correction_markers' bit numbering.
 * A flat or empty profile gives tonic 0, mode 0, scale_mask 0, correlation 0, clarity 0: "don't know", which the marker calls
 * read as all twelve classes.  The profiles and the defaults above are untuned; nothing here was run on recordings. */
typedef struct mx_key {
  int32_t tonic;      /* 0..11, A = 0 */
  int32_t mode;       /* 0 major, 1 natural minor */
  int32_t scale_mask; /* for mx_correction_markers / mx_correction_markers_tuned */
  int32_t reserved;   /* 0 */
  double tuning_cents, tuning_confidence;
  double correlation, clarity;
} mx_key;
typedef struct mx_key_window {
  int32_t first_frame, frames;
  mx_key key;
} mx_key_window;
int mx_key_from_chroma(const double *sum40, mx_key *out);
/* The same estimate from mx_detect_notes' output, for dry solo takes.  A note weighs its `frames` (none where frames <= 0);
 * the phasor is taken from the notes' fractional parts, t = 2 pi (note - rint(note)); the profile is p[rint(note - tuning / 100)
 * mod 12] += frames.  The notes may overlap or be out of order.  MX_ERR_INVALID for a note that is not finite. */
int mx_key_from_notes(const mx_note *notes, int64_t count, mx_key *out);
/* The whole file: mx_chroma_dev, then mx_chroma_sum_dev over the windows and over the whole take, in device memory of the call;
 * what comes back is 320 bytes per job.  Window w covers frames [w * window_hop, w * window_hop + window_frames) cut at the
 * file's end, w = 0, 1, .. while w * window_hop lies inside the file; window_frames 0 or windows NULL: no windows (window_hop
 * >= 1 otherwise).  *key: the take's.  *windows is library-allocated (free with mx_free).  params NULL: the defaults.  A hop of
 * 2048 is plenty: key needs no 5 ms resolution.  Blocks. */
int mx_key_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_chroma_params *params,
                  int64_t window_frames, int64_t window_hop, mx_key *key, mx_key_window **windows, int64_t *nwindows);
/* mx_correction_markers on a grid tuning_cents (finite, in [-50, 50]) above A = 440 Hz: the target of a note is
 * snap(note - t / 100) + t / 100 with mx_correction_markers' snap, t = tuning_cents; everything else as there.  With
 * tuning_cents 0 the output is mx_correction_markers', byte for byte. */
int mx_correction_markers_tuned(const mx_note *notes, int64_t count, double strength, int scale_mask, double tuning_cents,
                                mx_marker *out);

/* ---- Pitch drift and vibrato inside notes (BUILD-DEFINED; restated in int64 / f64 by tests/contour_ref.py) ----
 * mx_correction_markers_tuned moves a note by one constant bend; what happens inside the note stays.  This section splits the f0
 * contour of every note into centre, slow drift and vibrato, reports the vibrato's rate and extent, turns the split into a
 * per-frame bend curve, and lets the PSOLA renderer follow that curve.  The reference has none of it.
 *
 * Stage A, cents.  A frame is voiced by mx_detect_notes' rule (tau > 0, aperiodicity < threshold, rms >= rms_floor) and, in
 * addition, has a finite period > 0.  A voiced frame gives
 *   cents = (int32)rint(16.0 * (1200.0 * log2((double)sr / (double)period / 55.0) + 2400.0)),
 * in binary64 from the f32 period, no contraction: units of 1/16 cent, 1600 x mx_bin_note's note, negative at low sample rates.
 * Any other frame gives MX_CONTOUR_NONE.  A value depends on its record alone.  THE int32 IS THE DEFINITION FROM HERE ON:
 * everything downstream is exact integer arithmetic, the same on the device, on the host and in numpy; no summation order
 * matters and there is no tolerance.  (Two correctly built log2 may differ in the last place, so a value whose pre-rounding
 * magnitude lies within 1e-11 of a tie can differ by one unit between the device and a host restatement: about two frames in a
 * million lie within 1e-6 of one.)
 *
 * Stage B, split and statistics.  A span {first, frames} is a note's frames relative to the array: spans sorted, disjoint, inside
 * the array, frames >= 1, possibly adjacent.  Parameters: half-width w in [0, 64], 1 <= lag_min <= lag_max <= 256.  For the span
 * [f0, f0 + F) and a frame f in it:
 *   mean(v, f) = floor((2 S + c) / (2 c)) in int64 (nearest, halves up; the floor toward minus infinity, also for negative S),
 *                S the sum of v_g over g in [max(f - w, f0), min(f + w, f0 + F - 1)], c the number of taps;
 *   b_f = mean(cents, f);  smooth_f = mean(b, f);  vib_f = cents_f - smooth_f.
 * The window is clipped to the span in both passes: nothing leaks across a span boundary, not even between adjacent spans.  Two
 * box passes make a triangle of 4w + 1 frames; at the default w (250 ms) each box has its first null at 4 Hz.
 * Record of every frame of the array: {smooth, vib}; {MX_CONTOUR_NONE, 0} outside every span.
 * Statistics of a span: sum_smooth, min_smooth, max_smooth over its frames; r0 = sum vib_f^2;
 *   r(L) = sum of vib_f * vib_{f+L} over f, f + L both in the span, L in [lag_min, min(lag_max, F - 1)];
 *   lag = the L with the greatest r(L), the lowest L on ties, r_lag = r(lag); an empty range gives lag = 0, r_lag = 0.
 * Bound: the tracker's default band (55 .. 1760 Hz) spans 6000 cents = 96000 units, so inside a span |vib| < 2^17, a product
 * is below 2^34 and a sum over a span of up to 2^29 frames (a month at 187.5 frames/s) stays inside int64; sum_smooth is
 * smaller still.  For arbitrary records |cents| < 2^22 (any positive f32 period at any int sample rate: |log2| < 181), a
 * product is below 2^46 and 2^17 frames of one span are safe.  Beyond that the int64 sums wrap: wrong values, nothing worse.
 * Defaults (mx_contour_params_default): w = floor(0.125 sr / hop) clamped to [0, 64]; lag_min = max(1, floor(sr / hop / 12)),
 * lag_max = min(256, ceil(sr / hop / 3)) (at least lag_min): vibrato between 3 and 12 Hz.  The window, the band and the glide of
 * mx_bend_params are tuned on nothing but synthetic takes; nothing here was run on recordings. */
#define MX_CONTOUR_NONE INT32_MIN
typedef struct mx_contour_span {
  int32_t first, frames;
} mx_contour_span;
typedef struct mx_contour_params {
  int32_t half_width;       /* w, in [0, 64] */
  int32_t lag_min, lag_max; /* 1 <= lag_min <= lag_max <= 256 */
} mx_contour_params;
typedef struct mx_contour_rec {
  int32_t smooth; /* centre + drift, 1/16 cent (MX_CONTOUR_NONE outside every span) */
  int32_t vib;    /* cents - smooth (0 outside every span) */
} mx_contour_rec;
typedef struct mx_contour_stat {
  int64_t sum_smooth;
  int32_t min_smooth, max_smooth;
  int64_t r0;
  int32_t lag;      /* 0: no lag in range */
  int32_t reserved; /* 0 */
  int64_t r_lag;
} mx_contour_stat;
/* MX_ERR_INVALID for sr <= 0, hop outside [1, 16384] or p NULL. */
int mx_contour_params_default(int sampleRate, int hop, mx_contour_params *p);
/* Stage A over count records in HBM -> count int32 in HBM.  A thread per frame; asynchronous on the context's stream.
 * MX_ERR_INVALID, before any launch, for count outside [0, INT32_MAX], sr <= 0, a threshold or rms_floor that is not finite,
 * a null argument where count > 0. */
int mx_contour_cents_dev(mx_ctx *ctx, const mx_f0 *d_track, int64_t count, int sampleRate, float threshold, float rms_floor,
                         int32_t *d_cents);
/* Same, host pointers, through the context's staging buffers.  Blocks. */
int mx_contour_cents(mx_ctx *ctx, const mx_f0 *track, int64_t count, int sampleRate, float threshold, float rms_floor,
                     int32_t *cents);
/* Stage B: count values and nspans spans in HBM -> count records at d_rec and nspans statistics at d_stat (either may be NULL),
 * in HBM.  Asynchronous on the context's stream.  The smoothing is one launch (a workgroup per 256 frames, both box passes
 * through LDS), the statistics two (partial sums per 1024 frames of a span, then one workgroup per span): a span of a whole take
 * is spread over the device, and integer sums give the same bytes whatever the tiling.  Work memory (24 + 8 x lags bytes per
 * span and per 1024 frames, 8 bytes per frame where d_rec is NULL) belongs to the context, kept between calls, released by
 * mx_ctx_release_scratch; MX_ERR_NOMEM when it cannot be had.
 * MX_ERR_INVALID, before any launch, for count outside [0, INT32_MAX], nspans outside [0, count], parameters out of range, p NULL
 * or a null argument that is needed.
 * PRECONDITION (not checked on the device — mx_contour_split does check it): the spans are sorted, disjoint, inside the array
 * with frames >= 1, and no frame inside a span holds MX_CONTOUR_NONE.  Anything else gives wrong values and nothing worse:
 * every span is clipped to the array and every index into its array. */
int mx_contour_split_dev(mx_ctx *ctx, const int32_t *d_cents, int64_t count, const mx_contour_span *d_spans, int64_t nspans,
                         const mx_contour_params *p, mx_contour_rec *d_rec, mx_contour_stat *d_stat);
/* Same, host pointers (rec and stat: either may be NULL).  Checks the precondition first: MX_ERR_INVALID, before any launch
 * and with the outputs untouched, for spans out of order, overlapping, outside the array or with frames < 1, and for a frame
 * inside a span that holds MX_CONTOUR_NONE.  Blocks. */
int mx_contour_split(mx_ctx *ctx, const int32_t *cents, int64_t count, const mx_contour_span *spans, int64_t nspans,
                     const mx_contour_params *p, mx_contour_rec *rec, mx_contour_stat *stat);

/* Host logic (binary64, no contraction; tests/contour_ref.py does the same operations in the same order).
 * mx_contour_spans: spans[i] = {notes[i].first_frame - first_frame, notes[i].frames}, first_frame the frame index of the
 * track's record 0 (mx_detect_notes').  MX_ERR_INVALID for a null argument or a negative count; the spans are not judged here. */
int mx_contour_spans(const mx_note *notes, int64_t nnotes, int64_t first_frame, mx_contour_span *spans);
/* Vibrato figures of a span of `frames` frames at sr / hop frames per second:
 *   rate_hz = sr / hop / lag;  extent_cents = sqrt(2 r0 / frames) / 16, the peak of the sinusoid of the same power;
 *   strength = (r_lag / r0) * frames / (frames - lag), 1 for a pure sinusoid;  drift_cents = (max_smooth - min_smooth) / 16.
 * All four are 0 where lag == 0 or r0 == 0.  MX_ERR_INVALID for a null argument, frames < 1, frames <= lag, sr <= 0 or hop
 * outside [1, 16384]. */
typedef struct mx_vibrato {
  double rate_hz, extent_cents, strength, drift_cents;
} mx_vibrato;
int mx_contour_vibrato(const mx_contour_stat *stat, int32_t frames, int sampleRate, int hop, mx_vibrato *out);
/* The bend curve (semitones per frame of the array) that corrects the notes.  For frame h of note i (span i):
 *   bend_h = (float)(shift_i - drift_amount * ((double)smooth_h / 1600 - notes[i].note)
 *                    + (vibrato_scale - 1) * (double)vib_h / 1600),  evaluated in that order;
 * shift_i: the note's own move in semitones (shift NULL: 0), e.g. mx_correction_markers_tuned's target minus the note.  With
 * drift_amount 1, vibrato_scale 0 and shift_i = T_i - note_i the note's contour becomes flat at T_i: cents = centre + drift +
 * vib, the centre at the note's median, which is what the correction markers snap.  Between two notes whose gap is <=
 * glide_frames frames: binary64 linear interpolation between the bend of the last frame of one (x0, as a float) and of the
 * first frame of the next (x1), frame j of the G gap frames (j = 1..G) getting (float)(x0 + (x1 - x0) * j / (G + 1)).
 * Everywhere else outside notes: 0.  Parameters: drift_amount in [0, 1], vibrato_scale in [0, 4], glide_frames >= 0; defaults
 * {1, 1, 8}.  MX_ERR_INVALID for parameters out of range or not finite, a shift or a note that is not finite, spans that are
 * not what mx_contour_split accepts for `count` frames, a null argument.  p NULL: the defaults. */
typedef struct mx_bend_params {
  double drift_amount, vibrato_scale;
  int32_t glide_frames;
} mx_bend_params;
void mx_bend_params_default(mx_bend_params *p);
int mx_contour_bend(const mx_contour_rec *rec, int64_t count, const mx_note *notes, const mx_contour_span *spans, int64_t nnotes,
                    const double *shift, const mx_bend_params *p, float *bend_out);
/* One call: stage A over the host track (track[0] = frame first_frame, as in mx_detect_notes, with the note parameters'
 * threshold and rms_floor), stage B over the notes' spans, in device memory of the context.  params NULL:
 * mx_contour_params_default(sr, hop).  rec_out (count records) and stat_out (nnotes): either may be NULL.  Blocks.
 * MX_ERR_INVALID for what the stages refuse; an unvoiced frame inside a note is refused like any MX_CONTOUR_NONE inside a span. */
int mx_pitch_contour(mx_ctx *ctx, const mx_f0 *track, int64_t count, int sampleRate, int hop, int64_t first_frame,
                     const mx_note *notes, int64_t nnotes, float threshold, float rms_floor, const mx_contour_params *params,
                     mx_contour_rec *rec_out, mx_contour_stat *stat_out);

/* PSOLA follows a bend curve.  `bend`: count floats, semitones, one per frame of the track — a curve over the SOURCE, like the
 * formant curve, so it follows a time-stretch.  For a voiced grain
 *   r_k = clamp(exp2(((double)time2pitchbend(s_k / sr) + (double)bend[h]) / 12), 1/2, 2),
 *   h = clamp(floor((a_m + (2048 - p_m) / 2) / hop + 1/2), 0, count - 1), a_m = a_{m(k)} the grain's analysis mark, p_m its period:
 * the frame whose MEASUREMENT is centred on the mark.  The tracker's frame h reads samples [h hop - 2048, h hop + tau), so its
 * period describes the signal (2048 - tau) / 2 samples before h hop, 18 ms at 150 Hz and 48 kHz: a tenth of a 6 Hz vibrato
 * cycle, and a curve read at the frame P(a_m) reads would leave three quarters of such a vibrato standing (tests/
 * test_gpu_contour_render.py: 25.8 of 34.1 cents; 8.0 with the lead).  Everything else is mx_psola_plan's /
 * mx_psola_plan_formant's; bend NULL adds nothing (those entry points' bytes), and so does an all-zero curve.  The record
 * types and the kernels are the existing ones.  MX_ERR_INVALID for a bend value that is not finite and for whatever the
 * existing plans refuse.  The phase-vocoder and granular renderers follow markers only. */
int mx_psola_plan_bend(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                       const mx_marker *markers, int nmarkers, const float *bend, mx_psola_grain **grains, int64_t *ngrains,
                       int64_t *nsamples);
int mx_psola_plan_formant_bend(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                               const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                               const mx_formant_point *points, int npoints, const float *bend, mx_psola_fgrain **fgrains,
                               int64_t *ngrains, int64_t *nsamples);
/* Plan and synthesis in one call, as mx_psola_render_formant / mx_psola_render_formant_dev: npoints == 0 selects the plain
 * records and the plain kernel. */
int mx_psola_render_bend(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                         const mx_psola_params *params, const mx_marker *markers, int nmarkers, const mx_formant_point *points,
                         int npoints, const float *bend, float *pcm_f32_out, int16_t *pcm_i16_out);
int mx_psola_render_bend_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                             const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                             const mx_formant_point *points, int npoints, const float *bend, float *d_pcm_f32,
                             int16_t *d_pcm_i16);

/* ---- Loudness and note levelling (BUILD-DEFINED; restated by tests/loudness_ref.py) ----
 * The level macro of a vocal editor: how loud a take and each of its notes is, in LUFS (ITU-R BS.1770-4, one channel), the
 * gain points that even the notes out, and the gain that brings an export to a target loudness.  The output side is
 * mx_audio_gain (above): applied to the source ahead of any renderer, the f0 track stays valid.  mx_f0.rms and the sibilant
 * powers are unweighted and window-shaped; neither is a loudness.  The reference has no meter.
 *
 * Geometry, all integer, for sampleRate sr in [8000, 384000] and a take of n samples:
 *   S = (sr + 50) / 100                    a step, 10 ms;
 *   G = 10                                 steps per group: the 100 ms gating hop of BS.1770;
 *   W = 4 * ((32 * sr + 1499) / 1500)      warm-up samples (4096 at 48 kHz, 3764 at 44.1 kHz, 32768 = MX_AUDIO_PAD at 384 kHz:
 *                                          the warm-up never reads outside the left pad);
 *   steps = ceil(n / S), groups = ceil(steps / G).
 *
 * K-weighting, binary64 on the host, once per sample rate (the bilinear re-derivation of the two BS.1770 stages):
 *   shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / sr),
 *              Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K K;
 *              b = {Vh + Vb K/Q + K K, 2 (K K - Vh), Vh - Vb K/Q + K K} / a0,  a1 = 2 (K K - 1) / a0, a2 = (1 - K/Q + K K) / a0;
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 likewise; c = {1, -2, 1}, d1 and d2 as a1 and a2.
 * At 48 kHz these are the table of BS.1770-4 to the last digit it prints.  mx_loudness_coeffs gives {b0, b1, b2, a1, a2,
 * c0, c1, c2, d1, d2}; the device receives them as kernel arguments and computes no transcendental.
 *
 * Filter: binary64, transposed direct form II, no contraction, this order.  Group g starts with its four states zero at
 * sample i0 = g G S - W and runs i = i0 .. min((g + 1) G S, n) - 1, with v = (double)x_i and v = 0 for i < 0:
 *   y = b0*v + s1;  s1 = (b1*v - a1*y) + s2;  s2 = b2*v - a2*y;
 *   z = c0*y + t1;  t1 = (c1*y - d1*z) + t2;  t2 = c2*y - d2*z;
 * From i >= g G S on, step k = (i - g G S) / S of the group accumulates  energy += z*z  in ascending i, and  peak = the largest
 * |x_i| among the step's samples that are not NaN (Inf counts; 0 if there are none).  Samples at or beyond n are not visited
 * (the right pad is not relied on).  A record depends on the samples [g G S - W, (g + 1) G S) alone: the same bytes whatever
 * the launch split.  THE TRUNCATED WARM-UP IS PART OF THE DEFINITION.  (For information: at 48 kHz it differs from the
 * untruncated filter by at most 3.4e-9 relative per 100 ms — a 30 Hz sine; noise 4e-12.)
 *
 * Consequences (tests pin all three):
 *   silence gives energy == +0.0 and peak == 0 exactly, for -0.0f samples too;
 *   2^k x gives 4^k energy and 2^k peak bit for bit wherever 2^k x is exact in binary32 (and nothing under- or overflows);
 *   a NaN or +-Inf sample at position p makes energy non-finite (NaN or +Inf) in the groups with
 *   g G S - W <= p < min((g + 1) G S, n), there in the steps whose last sample is at or after p, and nowhere else: every other
 *   step keeps the bytes it has without the bad sample. */
typedef struct mx_loud_step {
  double energy;   /* sum of z*z over the step's samples */
  float peak;      /* sample peak of the step (the true peak: mx_tp_step below) */
  int32_t samples; /* S, or n - b*S for the last, partial step */
} mx_loud_step;
/* ceil(n / S); 0 for n < 1 or sampleRate outside [8000, 384000]. */
int64_t mx_loudness_step_count(int64_t n, int sampleRate);
/* out10 = {b0, b1, b2, a1, a2} of the shelf, then of the high-pass.  MX_ERR_INVALID (out10 untouched) for sampleRate out of range. */
int mx_loudness_coeffs(int sampleRate, double *out10);
/* The records of steps [G*first_group, min(G*(first_group + ngroups), steps)) -> d_steps (in HBM, 16-byte aligned: a record is
 * written as one 16-byte store).  Asynchronous on the context's stream.  MX_ERR_INVALID, before any launch, for sampleRate out
 * of range, first_group < 0, ngroups < 0, groups beyond the file, or NULLs (d_steps may be NULL where ngroups is 0). */
int mx_loudness_steps_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_group, int64_t ngroups,
                          mx_loud_step *d_steps);
/* Same, host output through the context's staging buffers.  Blocks. */
int mx_loudness_steps(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_group, int64_t ngroups, mx_loud_step *steps_out);
/* Loudness over a sliding window (host, binary64): for b >= window_steps - 1 with all window_steps steps full (samples == S)
 *   out[b] = -0.691 + 10 log10((energies of steps b - window_steps + 1 .. b, summed ascending) / (window_steps * S)),
 * else out[b] = -inf.  steps[0] is step 0 of the take.  window_steps 40: momentary (400 ms); 300: short-term (3 s).
 * MX_ERR_INVALID for sampleRate out of range, window_steps outside [1, 6000], a step whose samples lie outside [1, S]. */
int mx_loudness_curve(const mx_loud_step *steps, int64_t nsteps, int sampleRate, int window_steps, double *out);
/* Integrated loudness (BS.1770-4 gating, decided in the energy domain).  Block j covers steps [10 j, 10 j + 40), all 40 full
 * (j < blocks = the number of such blocks);  z_j = (their energies, summed ascending) / (40 S).  A block whose z is not finite
 * is left out and counted (bad_blocks).  Absolute gate: z_j > 0x1.f791ec6e1d5b7p-24 (= 10^((-70 + 0.691) / 10)).  Relative
 * gate: z_j > 0.1 * ((the z that pass the absolute gate, summed ascending) / passed_abs).
 *   integrated = -0.691 + 10 log10((the z that pass both gates, summed ascending) / passed_rel); -inf when passed_abs is 0;
 *   momentary_max, shortterm_max = the largest value of mx_loudness_curve with windows 40 and 300 that is not NaN (-inf: none);
 *   peak = the largest step peak (sample peak; the oversampled TRUE PEAK is mx_true_peak_measure's, below: DESIGN 5n). */
typedef struct mx_loudness {
  double integrated, momentary_max, shortterm_max; /* LUFS */
  float peak;
  int64_t blocks, passed_abs, passed_rel, bad_blocks;
} mx_loudness;
int mx_loudness_integrated(const mx_loud_step *steps, int64_t nsteps, int sampleRate, mx_loudness *out);
/* The whole take: its records on the GPU, then mx_loudness_integrated.  Blocks. */
int mx_loudness_measure(mx_ctx *ctx, const mx_audio *a, int sampleRate, mx_loudness *out);
/* Loudness per note (host, binary64): over the steps b < nsteps that lie inside the note, b*S >= start_sample and
 * (b + 1)*S - 1 <= end_sample; if there are none, over the step that holds (start_sample + end_sample) / 2:
 *   lufs = -0.691 + 10 log10(sum of energies, ascending / sum of samples);  -inf for zero energy, NaN if a chosen step's
 * energy is not finite.  MX_ERR_INVALID (lufs_out untouched) for a note with start_sample < 0, end_sample < start_sample, or
 * end_sample at or beyond the samples the records cover. */
int mx_note_loudness(const mx_loud_step *steps, int64_t nsteps, int sampleRate, const mx_note *notes, int64_t nnotes,
                     double *lufs_out);
/* Note levelling.  reference = the median of the finite lufs (an even count: the mean of the two middle values; none: NaN).
 * Per note d = reference - lufs_i, db = clamp((d > 0 ? raise : lower) * d, -max_db, max_db), A = (float)pow(10, db / 20) in
 * binary64; a note whose lufs is not finite gets A = 1.  out (2*nnotes points): {start_sample, A}, {end_sample, A} per note —
 * strictly increasing samples, accepted by mx_audio_gain as they are; between notes the gain is its linear ramp.  raise scales
 * the lift of quiet notes, lower the cut of loud ones.  params NULL: the defaults.  reference_out may be NULL.
 * MX_ERR_INVALID for notes out of order or overlapping (as mx_correction_markers), raise or lower outside [0, 1], max_db
 * outside [0, 40]. */
typedef struct mx_level_params {
  double raise, lower; /* [0, 1] */
  double max_db;       /* [0, 40] */
} mx_level_params;
/* {1.0, 1.0, 12.0} */
void mx_level_params_default(mx_level_params *p);
int mx_level_gain_points(const mx_note *notes, int64_t nnotes, const double *lufs, const mx_level_params *params,
                         mx_gain_point *out, double *reference_out);
/* The one gain that brings a measured take to target_lufs without its sample peak passing ceiling_db (dBFS):
 *   amp = (float)min(10^((target_lufs - integrated) / 20), 10^(ceiling_db / 20) / peak).
 * MX_ERR_INVALID (amp untouched) when integrated is not finite, peak is 0 or not finite, or an argument is not finite. */
int mx_normalize_gain(const mx_loudness *m, double target_lufs, double ceiling_db, float *amp);

/* ---- True peak, limiter and loudness range (BUILD-DEFINED; restated by tests/truepeak_ref.py) ----
 * The end of the export chain: the inter-sample ("true") peak of a take in the sense of BS.1770-4 annex 2, a look-ahead limiter
 * that holds a ceiling on it and writes the final int16, and the loudness range of EBU Tech 3342 from the mx_loud_step records.
 * One arithmetic: the same bytes on the device, in the CPU emulation and in numpy, whatever the launch split.  The reference
 * has none of it.
 *
 * Geometry, for sampleRate sr in [8000, 384000]:  S = (sr + 50) / 100, the 10 ms step of mx_loud_step; steps = ceil(n / S);
 * oversampling L = 4 for sr < 88200, 2 for 88200 <= sr < 176400, else 1 (true peak = sample peak).
 *
 * Taps: T = 12 per fractional offset u in {1/4, 1/2, 3/4}, rate-independent; for d = -5 .. 6 and v = d - u
 *   c_u[d] = (float)(sinc(v) * (0.42 + 0.5 cos(pi v / 6) + 0.08 cos(2 pi v / 6))),  sinc(v) = sin(pi v) / (pi v), in binary64.
 * L = 4 uses all three offsets, L = 2 uses 1/2 alone.  Offset 0 is the sample itself (an L-th-band prototype).  The 36 values
 * are literals of the library (mx_true_peak_taps): no libm between a test and the bytes.
 *
 * Per-sample peak, binary32 without contraction, x_j = 0 for j outside [0, n):
 *   y_{i,u} = sum over d ascending of x_{i+d} * c_u[d], from +0.f, each product rounded, then added;
 *   p_i = |x_i| if x_i is not NaN, else 0; then for each used u, ascending: p_i = |y_{i,u}| > p_i ? |y_{i,u}| : p_i.
 * A NaN never enters p_i; +-Inf counts.
 *
 * Record of step b (8 bytes): true_peak = the largest p_i, sample_peak = the largest |x_i| that is not NaN (mx_loud_step.peak's
 * rule) over the step's samples; true_peak >= sample_peak.  It depends on the samples [b S - 5, (b + 1) S + 6) alone.
 *
 * Limiter, for a ceiling amplitude c (a normal binary32, 0 < c <= 1) and a look-ahead of A samples (1 <= A <= 1024):
 *   q_j = 2^30 for j outside [0, n) and wherever !(p_j > c), else (int32)floor(((double)c / (double)p_j) * 2^30)  (0 for Inf);
 *   m_t = min over j in [t, t + A] of q_j;   s_i = sum over t in [i - A, i] of m_t  (int64);
 *   g_i = (double)s_i / (double)((int64_t)(A + 1) << 30);   out_i = (float)((double)x_i * g_i);   pcm_i = the clamped int16
 *   conversion of out_i ("PCM conversions" above).
 * Everything between p and g is integer: any tiling, scan order or prefix-sum scheme gives the same bytes.
 *
 * Consequences (tests pin all five):
 *   1. |out_i| <= c for every finite input;
 *   2. out_i has x_i's bytes wherever no j in [i - A, i + A] has p_j > c (g is exactly 1);
 *   3. limit(2^k x, 2^k c) = 2^k limit(x, c) bit for bit where 2^k scales exactly and nothing under- or overflows; the records
 *      scale likewise;
 *   4. silence, of -0.0f samples too, gives records {0, 0} and an output with the input's bytes;
 *   5. a NaN or +-Inf sample at s changes no record outside the steps that hold samples of [s - 6, s + 5] and no output sample
 *      outside [s - A - 6, s + A + 6].
 * The TRUE peak of the output is not bounded by c exactly (a moving gain changes the values between the samples): by how much
 * is a measurement, DESIGN 5n. */
typedef struct mx_tp_step {
  float true_peak;   /* the largest p_i of the step */
  float sample_peak; /* the largest |x_i| that is not NaN */
} mx_tp_step;
/* L; 0 for sampleRate outside [8000, 384000]. */
int mx_true_peak_oversampling(int sampleRate);
/* out36 = c_{1/4}[-5 .. 6], c_{1/2}[-5 .. 6], c_{3/4}[-5 .. 6].  MX_ERR_INVALID for NULL. */
int mx_true_peak_taps(float *out36);
/* The records of steps [first_step, first_step + nsteps) -> d_steps (in HBM, 8-byte aligned: a record is one 8-byte store).
 * Asynchronous on the context's stream.  MX_ERR_INVALID, before any launch, for sampleRate out of range, a step range outside
 * the file's steps, or NULLs (d_steps may be NULL where nsteps is 0). */
int mx_true_peak_steps_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, mx_tp_step *d_steps);
/* Same, host output through the context's staging buffers.  Blocks. */
int mx_true_peak_steps(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, mx_tp_step *steps_out);
/* The whole take: the largest true_peak and the largest sample_peak of its records (0 for an empty take).  Either output may
 * be NULL, not both.  Blocks. */
int mx_true_peak_measure(mx_ctx *ctx, const mx_audio *a, int sampleRate, float *true_peak, float *sample_peak);
typedef struct mx_limit_params {
  float ceiling_amp; /* c: an amplitude, a normal binary32 in (0, 1] */
  int32_t lookahead; /* A: samples, [1, 1024] */
} mx_limit_params;
/* {(float)10^(-1/20) (-1 dBTP), min(1024, (sampleRate + 100) / 200) (5 ms)}.  MX_ERR_INVALID (p untouched) for sampleRate out
 * of range or NULL. */
int mx_limit_params_default(int sampleRate, mx_limit_params *p);
/* The limited take as a new audio object (zeroed pads, as mx_audio_gain_dev; release it with mx_audio_free) and, where
 * d_pcm16 is not NULL, its n int16 samples in HBM.  params NULL: the defaults.  Asynchronous on the context's stream.
 * MX_ERR_INVALID, before any launch and with *out untouched, for sampleRate out of range, NULLs, c not normal or outside
 * (0, 1], A outside [1, 1024].  n = 0 gives an empty object. */
int mx_audio_limit_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out,
                       int16_t *d_pcm16);
/* Same with a host pcm16_out (n int16, may be NULL).  Blocks. */
int mx_audio_limit(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out, int16_t *pcm16_out);
/* Loudness range (EBU Tech 3342; host, binary64) of mx_loud_step records, steps[0] = step 0.  Short-term mean squares z_k =
 * (the energies of steps b - 299 .. b, summed ascending) / (300 S) at b = 299 + 10 k, all 300 steps full: 3 s every 100 ms.
 * A z that is not finite is left out and counted (bad).  Absolute gate: z > 0x1.f791ec6e1d5b7p-24 (mx_loudness_integrated's);
 * relative gate: z > 0.01 * ((the z that pass the absolute gate, summed ascending) / their count), -20 LU.  The m survivors
 * sorted ascending:  low = sorted[floor((m - 1) * 0.10 + 0.5)], high = sorted[floor((m - 1) * 0.95 + 0.5)],
 *   lra = 10 log10(high / low), low_lufs / high_lufs = -0.691 + 10 log10(low / high);  m = 0: lra 0, low_lufs = high_lufs = -inf.
 * values = the z_k that exist (bad ones included), gated = m.  MX_ERR_INVALID as mx_loudness_integrated. */
typedef struct mx_loudness_range_result {
  double lra, low_lufs, high_lufs;
  int64_t values, gated, bad;
} mx_loudness_range_result;
int mx_loudness_range(const mx_loud_step *steps, int64_t nsteps, int sampleRate, mx_loudness_range_result *out);
/* mx_normalize_gain with a measured true peak in place of m->peak and the ceiling in dBTP:
 *   amp = (float)min(10^((target_lufs - integrated) / 20), 10^(ceiling_dbtp / 20) / true_peak).
 * MX_ERR_INVALID (amp untouched) when integrated is not finite, true_peak is 0 or not finite, or an argument is not finite. */
int mx_normalize_gain_tp(const mx_loudness *m, float true_peak, double target_lufs, double ceiling_dbtp, float *amp);

/* ---- Sample-rate conversion (BUILD-DEFINED; restated by tests/resample_ref.py) ----
 * A take at another sample rate: a polyphase windowed-sinc filter with one table, one summation order and the same bytes on the
 * device, in the CPU emulation and in numpy, whatever the launch split.  The reference has none of it (its SwrContext keeps the
 * rate).  In the export chain it sits BEFORE the limiter: a true peak is a property of the samples at the delivered rate.
 *
 * Plan, for rates in [8000, 384000]:  g = gcd(in, out), L = out / g, M = in / g, s = min(1, L / M);  Z = 32 zero crossings a
 * side, H = ceil(Z / s) = ceil(Z max(L, M) / L) in integers, T = 2 H taps.  Refused (MX_ERR_INVALID): a rate out of range,
 * L > 1024, T > 512.  Equal rates are not refused: the plan is {L = 1, M = 1, T = 0, H = 0} and every form below copies the
 * input's bytes; there is no table.  48000 -> 44100 is 147 / 160 with T = 70, 44100 -> 48000 is 160 / 147 with T = 64,
 * 96000 -> 48000 is 1 / 2 with T = 128, 192000 -> 44100 is 147 / 640 with T = 280; 384000 -> 44100 (T = 558) and
 * 44100 -> 48001 (L = 48001) are refused.
 *
 * Length: m = ceil(n L / M) outputs; output j sits at input time j M / L: the conversion is centred and adds no delay.
 *
 * Table: h[phi][k], phase phi < L, tap k < T, belongs to the input sample at offset d = k - (H - 1) from i_j, at distance
 * u = d - phi / L from the output.  In binary64:  h = s sinc(s u) w(u / H),  sinc(v) = sin(pi v) / (pi v) (1 at 0),
 * w(t) = I0(12 sqrt(1 - t^2)) / I0(12), the Kaiser window with beta = 12;  I0(x) is the power series sum of ((x / 2)^k / k!)^2
 * summed in ascending k until a term falls below 2^-60 of the sum.  Each row is divided by its binary64 sum (k ascending), so DC
 * passes at 1; then each tap is rounded to binary32.  One exception, exact by definition: where s = 1 and phi = 0 the row is the
 * unit row, 1 at d = 0 and +0 elsewhere (sin(pi k) is not 0 in floating point, and an output that falls on an input sample shall
 * be that sample).  mx_resample_taps hands the table out: the device, the emulation and numpy all read that one table.
 *
 * An output:  i_j = floor(j M / L), phi_j = (j M) mod L, in 64-bit integers;
 *   y_j = sum over k ascending of x[i_j - (H - 1) + k] * h[phi_j][k], from +0.f, each product rounded, then added, in binary32
 * without contraction (the true peak's rule).  Samples outside [0, n) are zeros whatever the pads hold.  A NaN or +-Inf is plain
 * arithmetic.
 *
 * Consequences (tests pin all six, on the emulation and on the device):
 *   1. unit rows: where L > M, out[j] for (j M) mod L = 0 has the bytes of x[j M / L] for every finite window;
 *   2. scale: resample(2^k x) = 2^k resample(x) bit for bit where nothing leaves the normal range;
 *   3. silence, of -0.0f samples too, gives +0.f everywhere;
 *   4. locality: sample s changes no output outside those j with s - H <= i_j <= s + H - 1; a NaN at s makes exactly those NaN;
 *   5. shift: x delayed by M samples is the output delayed by L samples, byte for byte, away from the file's ends;
 *   6. split: any split of [0, m) into ranges gives the same bytes. */
typedef struct mx_resample_plan {
  int32_t L;    /* phases: out / gcd */
  int32_t M;    /* in / gcd */
  int32_t taps; /* T = 2 H; 0 for equal rates */
  int32_t half; /* H */
} mx_resample_plan;
/* The plan of inRate -> outRate.  MX_ERR_INVALID (out untouched) for what the plan refuses, or NULL. */
int mx_resample_plan_for(int inRate, int outRate, mx_resample_plan *out);
/* m for n samples; negative (MX_ERR_INVALID) for n < 0 or a refused rate pair. */
int64_t mx_resample_length(int64_t n, int inRate, int outRate);
/* out = h[0][0 .. T), h[1][0 .. T), ...: L * T floats (none for equal rates).  MX_ERR_INVALID for a refused rate pair or NULL. */
int mx_resample_taps(int inRate, int outRate, float *out);
/* Outputs [first_out, first_out + count) of the converted take -> d_out[0 .. count) (in HBM, at any 4-byte-aligned address).
 * Asynchronous on the context's stream.  An empty range is legal.  MX_ERR_INVALID, before any launch and with nothing written,
 * for a refused rate pair, a range outside [0, m), NULLs (d_out may be NULL where count is 0) or a misaligned d_out. */
int mx_resample_dev(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, int64_t first_out, int64_t count, float *d_out);
/* Same, host output staged through device memory of the call's own.  Blocks. */
int mx_resample(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, int64_t first_out, int64_t count, float *out);
/* The converted take as a new audio object of m samples (zeroed pads, as mx_audio_gain_dev; release it with mx_audio_free).
 * Asynchronous on the context's stream.  MX_ERR_INVALID, with *out untouched, for a refused rate pair or NULLs, and, before
 * anything is allocated, for m > 0x7fffffff - 2 * MX_AUDIO_PAD (mx_audio_upload's bound: no kernel could walk the object; a
 * maximal 44.1 kHz take to 48 kHz asks for 2 337 325 836).  The range forms above keep serving outputs above 2^31. */
int mx_audio_resample(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, mx_audio **out);

/* ---- Noise reduction (BUILD-DEFINED; restated in f64 by tests/denoise_ref.py) ----
 * Spectral noise reduction of a take from a noise print: the step before every analyser and renderer.  The reference has none
 * of it (app.cpp decodes to mono and edits what it got).  One transform size, one wavefront per frame on the onset detector's
 * transform, a gain rule without discontinuities.
 *
 * Framing: N = 1024, hop H = 256, any sample rate.  w[j] = 0.5 - 0.5 cos(2 pi j / 1024) (periodic Hann).  Frame f starts at
 * sample (f - 3) H, f = 0 .. F - 1, F = ceil(n / H) + 3 (mx_denoise_frames): every sample of [0, n) lies in exactly four
 * frames.  Samples outside [0, n) are zeros whatever the pads hold.  X_f[k], k = 0 .. 512, is the real transform of w x.
 *
 * Noise print: P[k], 513 binary32 values.  Learned from samples [begin, end) of a take (0 <= begin <= end <= n): over the frames
 * that lie wholly inside, begin <= (f - 3) H and (f - 3) H + N <= end — at least 1 and at most 8192 of them, anything else is
 * refused before any launch —, P[k] = the binary64 sum, in ascending frame order, of the binary32 powers
 * a_f[k] = (|X_f[k]| / 512)^2 (the sibilant features' scale), divided by the frame count in binary64 and rounded to binary32.
 * A print may equally be the caller's own (a saved one, a synthetic one); a negative or non-finite value is refused.
 *
 * Parameters: reduction_db in [0, 60], sensitivity_db in [-12, 24], NaN refused.  The host turns them into two binary32
 * factors, once, in binary64: floor = 10^(-reduction_db / 20), sens = 10^(sensitivity_db / 10); mx_denoise_factors hands them
 * out: the device, the emulation and numpy all read those two floats.
 *
 * Raw gain per frame and bin, binary32, written as comparisons:  theta = sens P[k];  g = a > theta ? 1 - theta / a : 0;
 * g = g < floor ? floor : g.  Continuous in a; a NaN power gives `floor`; no square root, no threshold at which a bin flips.
 * Smoothed gain: first over time, ((g_{f-1} + (g_f + g_f)) + g_{f+1}) * 0.25 with f - 1, f + 1 clamped to [0, F - 1]; then over
 * frequency, the same expression of the time-smoothed values at k - 1, k, k + 1 with k - 1, k + 1 clamped to [0, 512].
 *
 * Output: y_f = the inverse real transform of G_f X_f, times w, times the binary32 constant 2/3 (the squared windows of the four
 * frames sum to exactly 3/2).  out[t] = the sum of its four frames in ascending f from +0.f, each product rounded, then added,
 * without contraction.  int16: the clamped conversion of "PCM conversions".
 *
 * Consequences (tests/denoise_ref.py check_laws pins them on the emulation and on the device):
 *   split         any split of the output range gives the same bytes, and so does any run length;
 *   scale         x 2^k with P 4^k gives out 2^k bit for bit where nothing leaves the normal range (k = -7, -20);
 *   zero print    P = 0 gives out = x within 2e-5 max|x| + 1e-9: the transform pair's own error;
 *   full          a print of 1e6 times the take's largest power gives out = floor x within the same bound;
 *   silence       silence, of -0.0f samples too, gives zeros;
 *   locality      a NaN at sample s makes exactly the outputs of [(floor(s / H) - 3) H, (floor(s / H) + 4) H) in [0, n) NaN:
 *                 its four frames' gains are `floor` and their spectra NaN; the frames either side see those gains through the
 *                 time smoothing, so no output outside [(floor(s / H) - 4) H, (floor(s / H) + 5) H) changes a bit, and where
 *                 every gain is `floor` anyway (the full-reduction print) none outside the NaN stretch does. */
typedef struct mx_denoise_params {
  float reduction_db;   /* the most a bin is turned down, dB: [0, 60] */
  float sensitivity_db; /* how far above the print a bin counts as noise, dB of power: [-12, 24] */
} mx_denoise_params;
#define MX_DENOISE_BINS 513
/* F for a take of n samples; negative (MX_ERR_INVALID) for n < 0. */
int64_t mx_denoise_frames(int64_t n);
/* out[0] = floor, out[1] = sens.  MX_ERR_INVALID (out untouched) for parameters out of range, NaN or NULLs. */
int mx_denoise_factors(const mx_denoise_params *params, float *out);
/* The power rows of frames [first_frame, first_frame + count) -> d_rows[513 f + k] (HBM, 4-byte aligned).  Asynchronous on the
 * context's stream.  MX_ERR_INVALID, before any launch, for frames outside [0, F) or NULLs (d_rows may be NULL where count is 0). */
int mx_noise_rows_dev(mx_ctx *ctx, const mx_audio *a, int64_t first_frame, int64_t count, float *d_rows);
/* The print of `count` rows on the host (the definition's sum, what the device's second kernel computes): count in [1, 8192]. */
int mx_noise_print_rows(const float *rows, int64_t count, float *print);
/* The print of samples [begin, end) -> d_print[0 .. 513) (HBM, 4-byte aligned): the rows pass through work memory of the
 * context.  Asynchronous on the context's stream.  MX_ERR_INVALID, before any launch and with nothing written, for a region
 * outside the take, with no frame or with more than 8192, or NULLs. */
int mx_noise_print_dev(mx_ctx *ctx, const mx_audio *a, int64_t begin, int64_t end, float *d_print);
/* Same, host output.  Blocks. */
int mx_noise_print(mx_ctx *ctx, const mx_audio *a, int64_t begin, int64_t end, float *print);
/* Outputs [first, first + count) of the cleaned take -> d_f32[0 .. count) and / or d_i16[0 .. count) (HBM, at any 4-byte / 2-byte
 * aligned address; each may be NULL, not both where count > 0).  print: 513 values in HOST memory, checked and copied before the
 * call returns.  Asynchronous on the context's stream.  An empty range is legal.  MX_ERR_INVALID, before any launch and with
 * nothing written, for refused parameters, a refused print, a range outside [0, n), NULLs or a misaligned output. */
int mx_denoise_dev(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, int64_t first,
                   int64_t count, float *d_f32, int16_t *d_i16);
/* Same, host outputs staged through device memory of the call's own.  Blocks. */
int mx_denoise(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, int64_t first, int64_t count,
               float *f32_out, int16_t *i16_out);
/* The cleaned take as a new audio object of n samples (zeroed pads, as mx_audio_gain_dev; release it with mx_audio_free): the
 * source of every analyser and renderer without a round trip.  Asynchronous on the context's stream.  MX_ERR_INVALID, with *out
 * untouched, for refused parameters, a refused print or NULLs. */
int mx_audio_denoise(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, mx_audio **out);

/* ---- Dynamics compressor (BUILD-DEFINED; restated in binary64 and Python integers by tests/compress_ref.py) ----
 * A feed-forward peak compressor with a threshold, a ratio, a soft knee, attack and release times, a look-ahead and a make-up
 * gain: the step between note levelling (one gain per note) and the limiter (nothing over the ceiling), and its gain-reduction
 * curve, the meter an editor draws.  The reference has none of it (app.cpp exports what process() wrote).  Integers from one
 * table look-up on: the device, the CPU emulation and numpy give the same bytes whatever the launch split.
 *
 * Geometry: sr in [8000, 384000].  A control step is D = (sr + 500) / 1000 samples (integer division: 48 at 48 kHz, 44 at
 * 44.1 kHz), B = ceil(n / D) steps (mx_compress_steps); step b covers samples [b D, (b + 1) D) of [0, n).  Samples outside the
 * file do not exist, whatever the pads hold.
 *
 * Parameters (mx_compress_params; NaN and anything out of range refused before any launch): threshold_db [-60, 0], ratio
 * [1, 100], knee_db [0, 24], attack_ms [0, 500], release_ms [0, 2000], lookahead_ms [0, 20], makeup_amp a normal number in
 * [1/16, 16] (an amplitude: the facade converts dB).  Defaults: -18 dB, 4, 6 dB, 5 ms, 100 ms, 0 ms, 1.
 *
 * Plan (mx_compress_plan_for; binary64 on the host, once): K = floor(lookahead_ms sr / (1000 D) + 0.5) steps;
 * c = round((1 - exp(-D / (sr tau))) 2^24) clamped to [1, 2^24] for tau = attack, release in seconds, 2^24 for tau = 0; the group
 * length Gc = 4096 steps; the warm-up W = min(32768, 16 ceil(2^24 / min(c_att, c_rel))) steps.
 *
 * Curve (mx_compress_curve): T[j], j = 0 .. 2048, the Q30 gain target of the level p whose binary32 bit pattern is
 * ((127 - 24) << 23) + (j << 17): 64 entries an octave from 2^-24 to 2^8.  In binary64: L = 20 log10 p, o = L - threshold,
 * s = 1 / ratio - 1; g_dB = 0 where 2 o <= -knee, s (o + knee / 2)^2 / (2 knee) where |2 o| < knee, s o otherwise;
 * T[j] = min(2^30, floor(10^(g_dB / 20) 2^30)), then a running minimum over j: non-increasing, and at least 1 inside the ranges.
 *
 * Peak: p_b = the largest |x_i| of step b that is not a NaN (+-Inf counts); 0 for a step without one and for b outside [0, B).
 * Target: p clamped to [2^-24, 2^8], u = bits(p) - ((127 - 24) << 23), j = u >> 17, r = u & 0x1ffff:
 * q_b = T[j] + (((int64)(T[j + 1] - T[j]) r) >> 17) (arithmetic shift), T[2048] at the top.  (T[0] = 2^30: a step outside the
 * file asks for unity.)
 * Smoothed gain, int64: q_b < s ? s -= ((s - q_b) c_att + 2^24 - 1) >> 24 : s += ((q_b - s) c_rel + 2^24 - 1) >> 24: rounded
 * towards the target, so it arrives.  Group g owns steps [g Gc, (g + 1) Gc): it starts from s = 2^30 at step g Gc - W and its s_b
 * count from g Gc on; s_b = 2^30 for b < 0; for b >= B the recurrence goes on with q = 2^30 as far as K asks.  The truncated
 * warm-up is part of the definition: s_b depends on the peaks of [floor(b / Gc) Gc - W, b] alone.
 * Output, sample i of step b at offset o = i - b D: G_i = s_{b+K-1} (D - o) + s_{b+K} o (int64);
 * out_i = (float)(((double)x_i (double)makeup_amp) (double)G_i / (double)(D 2^30)) in binary64 without contraction; where
 * G_i = D 2^30 and makeup_amp = 1 the quotient is left out: out_i = x_i, the same value.  int16: the clamped conversion of "PCM
 * conversions".
 *
 * Laws (tests/compress_ref.py check_laws pins them on the emulation and on the device):
 *   split        any [first, count) and any launch geometry give the whole call's bytes;
 *   ratio 1      ratio 1 with makeup 1 gives the input's bytes;
 *   below        a take whose every |x| lies a table interval below the knee's lower edge — at most edge / (1 + 1/64): the entry
 *                above the edge pulls the interpolation under it below unity — gives the input's bytes (makeup 1); silence, of
 *                -0.0f too, gives its own bytes;
 *   steady       a constant |x| = a gives s = q(a) exactly after finitely many steps (at a seam, where the attack is no slower than
 *                the release), then out = the quotient with G = D q(a): a m q(a) / 2^30 to the last binary32 place;
 *   recovery     after the last step over that level s returns to exactly 2^30; from there out = x (makeup 1);
 *   monotone     raising any |x_i| raises no s_b;
 *   NaN          a NaN in place of a sample that is not its step's largest changes out_t alone (the peak passes over it);
 *   Inf          an +-Inf at sample t changes no output before sample (floor(t / D) - K - 1) D, and none from sample
 *                ((floor((floor(t / D) + W) / Gc) + 1) Gc - K + 1) D on: the steps after it in its own group, and the groups
 *                whose warm-up still reads it, are all that see its step. */
typedef struct mx_compress_params {
  float threshold_db; /* [-60, 0] */
  float ratio;        /* [1, 100] */
  float knee_db;      /* full width of the soft knee, dB: [0, 24] */
  float attack_ms;    /* [0, 500] */
  float release_ms;   /* [0, 2000] */
  float lookahead_ms; /* [0, 20] */
  float makeup_amp;   /* a normal number in [1/16, 16] */
} mx_compress_params;
typedef struct mx_compress_plan {
  int32_t D;     /* samples per control step */
  int32_t K;     /* look-ahead, steps */
  int32_t c_att; /* Q24 */
  int32_t c_rel; /* Q24 */
  int32_t W;     /* warm-up, steps */
  int32_t Gc;    /* steps per group */
} mx_compress_plan;
#define MX_COMPRESS_CURVE 2049
/* The defaults at sampleRate.  MX_ERR_INVALID for a rate out of range or a NULL. */
int mx_compress_params_default(int sampleRate, mx_compress_params *p);
/* The plan of `params` (NULL: the defaults) at sampleRate.  MX_ERR_INVALID (plan untouched) for refused parameters or rate, NULL. */
int mx_compress_plan_for(int sampleRate, const mx_compress_params *params, mx_compress_plan *plan);
/* T[0 .. 2049) of `params` (NULL: the defaults; the curve does not depend on the rate).  MX_ERR_INVALID (out untouched) likewise. */
int mx_compress_curve(const mx_compress_params *params, int32_t *out);
/* B for a take of n samples; negative (MX_ERR_INVALID) for n < 0 or a rate out of range. */
int64_t mx_compress_steps(int64_t n, int sampleRate);
/* p_b of steps [first_step, first_step + nsteps) of [0, B) -> d_peaks[0 .. nsteps) (HBM, 4-byte aligned).  Asynchronous on the
 * context's stream.  MX_ERR_INVALID, before any launch, for steps outside [0, B), a refused rate, NULLs or a misaligned output. */
int mx_compress_peaks_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, float *d_peaks);
/* s_b of steps [first_step, first_step + nsteps) of [0, B), Q30 -> d_gain[0 .. nsteps) (HBM, 4-byte aligned): the meter
 * (20 log10(s / 2^30) dB).  The peaks pass through work memory of the context.  Asynchronous on the context's stream. */
int mx_compress_gain_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first_step,
                         int64_t nsteps, int32_t *d_gain);
/* Same, host output.  Blocks. */
int mx_compress_gain(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first_step,
                     int64_t nsteps, int32_t *gain);
/* Outputs [first, first + count) of the compressed take -> d_f32[0 .. count) and / or d_i16[0 .. count) (HBM, at any 4-byte /
 * 2-byte aligned address; each may be NULL, not both where count > 0).  Only the groups the range and its look-ahead touch are
 * computed, in work memory of the context.  Asynchronous on the context's stream.  An empty range is legal.  MX_ERR_INVALID,
 * before any launch and with nothing written, for refused parameters or rate, a range outside [0, n), NULLs or a misaligned
 * output. */
int mx_compress_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first, int64_t count,
                    float *d_f32, int16_t *d_i16);
/* Same, host outputs staged through device memory of the call's own.  Blocks. */
int mx_compress(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first, int64_t count,
                float *f32_out, int16_t *i16_out);
/* The compressed take as a new audio object of n samples (zeroed pads, as mx_audio_gain_dev; release it with mx_audio_free): the
 * source of the loudness measure, the gain, the converter and the limiter without a round trip.  Asynchronous on the context's
 * stream.  MX_ERR_INVALID, with *out untouched, for refused parameters or rate or NULLs. */
int mx_audio_compress(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, mx_audio **out);

/* ---- WAV writer -------------------------------------------------------------
 * Replaces saveWav (save-wav.cpp:17-48).  strict_reference_header != 0
 * reproduces the size-field quirk of save-wav.cpp:43 byte for byte (data size
 * = 2m+16, PCM samples 0 and 1 zeroed); 0 writes a correct RIFF header. */
int mx_save_wav(const char *path, const int16_t *pcm, int64_t m, int sampleRate,
                int strict_reference_header);

#ifdef __cplusplus
}
#endif
#endif /* MELONIX_AMD_H */
