// capi_internal.h — what the units of the C-ABI implementation (capi_*.cpp) share: the context and audio handle types, the error
// slot behind mx_last_error, the per-N table cache, and the sequences written once: the owners of device memory (DeviceArray for a
// call; WorkMem, a locked set of GrowBufs, for a context), the chunked host-staged loop (staged_batch), the host form of a job-list
// call (job_pass), the host form of a device form that writes one array (array_to_host) or PCM in two formats (pcm_to_host), the
// tail of a PCM range entry point (pcm_range), the arrays handed out for mx_free (HandOver, hand_over), the MELONIX_TIMING
// phase clock (PhaseClock); for the per-frame tracks (f0, onset strength, sibilant features, chroma): the frame-span check
// (frame_span), the staged host form (staged_records), a call's common head, its parse and its one-record host form (TrackCall,
// track_parse, staged_track), the small argument checks (handles_check, handles_out_check, align_check, hop_check, rate_check,
// frames_i32, notes_check); for the step records
// (loudness, true peak): their rate check, span check, head and parse (step_rate_check, unit_span, StepsCall, steps_parse); a whole
// take's records reduced on the host (whole_take); the parameters in force and their defaults (params_or, params_default), the
// device tables built on the host (upload_table).
// Not installed; include/melonix_amd.h is the boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/melonix_amd.h"
#include "host_logic.h"
#include "kernels.h"
#include "step_core.h"

namespace mx {

// records the message mx_last_error returns on this thread and hands `code` back (a fixed thread-local buffer: recording an
// error allocates nothing and cannot throw — it is what the handlers below call)
int fail(int code, const char *fmt, ...) noexcept __attribute__((format(printf, 2, 3)));

// NOTHING THROWN CROSSES extern "C" (SURVEY 8b "Errors": the reference's callers get empty results, never exceptions; an
// exception that reached the C boundary would std::terminate the editor).  By construction: the body of EVERY entry point of
// capi_*.cpp is a lambda run by one of these three — tests/test_abi.py checks that of the sources, tests/cpp/fault_sweep.cpp makes
// operator new fail at the k-th call inside the library for every k and watches the statuses.
//   mx_guard       entry points that return a status (int) or a count / size that is negative on error (int64_t)
//   mx_guard_or    entry points that return a value (time maps: double, float, int): `fallback` + the error recorded
//   mx_guard_void  entry points that return nothing (destructors, pure out-parameter helpers)
template <class T, class F>
T mx_guard_or(T fallback, F &&body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    fail(MX_ERR_NOMEM, "out of host memory");
  } catch (const std::exception &e) {
    fail(MX_ERR_INVALID, "%s", e.what());
  } catch (...) {
    fail(MX_ERR_INVALID, "unknown exception");
  }
  return fallback;
}
template <class F>
auto mx_guard(F &&body) noexcept -> decltype(body()) {
  using R = decltype(body());
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return (R)fail(MX_ERR_NOMEM, "out of host memory");
  } catch (const std::exception &e) {
    return (R)fail(MX_ERR_INVALID, "%s", e.what());
  } catch (...) {
    return (R)fail(MX_ERR_INVALID, "unknown exception");
  }
}
template <class F>
void mx_guard_void(F &&body) noexcept {
  try {
    body();
  } catch (const std::bad_alloc &) {
    fail(MX_ERR_NOMEM, "out of host memory");
  } catch (const std::exception &e) {
    fail(MX_ERR_INVALID, "%s", e.what());
  } catch (...) {
    fail(MX_ERR_INVALID, "unknown exception");
  }
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return ::mx::fail(MX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct NTables {
  float2 *tw2 = nullptr, *tw3 = nullptr, *ubase = nullptr;
  float *wext = nullptr;  // d-indexed window weights, pre-scaled by 1/(2N)
  std::vector<float> wext_host;
};

// Device memory a call (or a staged rank job) owns: n elements, freed on every path, and only once `stream` has drained — nothing
// of ours may still be in flight when it goes.
template <class T>
struct DeviceArray {
  T *p = nullptr;
  size_t n = 0;
  hipStream_t stream = nullptr;
  DeviceArray() = default;
  DeviceArray(const DeviceArray &) = delete;
  DeviceArray &operator=(const DeviceArray &) = delete;
  ~DeviceArray() { reset(); }
  void reset() {
    if (!p) return;
    hipStreamSynchronize(stream);
    hipFree(p);
    p = nullptr;
  }
  T *release() { return std::exchange(p, nullptr); }  // (the buffer goes on living: its new owner frees it)
  hipError_t alloc(hipStream_t s, size_t count) {  // (count 0: no buffer)
    reset();
    stream = s;
    n = count;
    return count ? hipMalloc(&p, count * sizeof(T)) : hipSuccess;
  }
  // the first `count` elements (default: all) into host memory (may be null: nothing), queued on the stream behind what wrote them
  hipError_t download(T *host, size_t count = SIZE_MAX) const {
    return p && host ? hipMemcpyAsync(host, p, std::min(count, n) * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess;
  }
};

// Device memory a context keeps between calls: grows to the largest request, never shrinks until dropped — a screen-sized
// batch otherwise spends more time in hipMalloc/hipFree than in the kernel.  The lock of its set (WorkMem) guards it.
struct GrowBuf {
  void *p = nullptr;
  size_t cap = 0;
  void drop() {
    hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
// The one form of a context's kept device memory: K buffers behind one lock.  A call holds the set (Hold) while anything it queued
// may use the buffers and asks for each with get(): room for n elements of T (bytes where T is void), contents undefined.  Where a
// buffer cannot be had the stream is drained and the WHOLE set is given back — nothing of it stays allocated behind an
// MX_ERR_NOMEM — and `what` names the set in the message.
// LOCK ORDER, the one every path keeps: the staging set (staged_batch, staged_records), then a family's own set (tempo), then `jobs`
// (job_pass); a set that only a device form takes (contour inside job_pass's launch, f0dec inside staged_records' run) comes last.  No path takes two sets
// in two orders, and job_pass is never entered from inside its own launch.
template <int K>
struct WorkMem {
  std::mutex mu;
  GrowBuf buf[K];
  void drop() { for (GrowBuf &b : buf) b.drop(); }  // (the caller holds the set or owns the context outright)
};
enum StageSlot { kStageMags, kStagePitch, kStageRanges, kStageTexels, kStageSlots };
enum ChainSlot { kChainBitmap7, kChainBitmap3, kChainRanks, kChainTables, kChainSlots };
enum F0DecSlot { kF0DecBp, kF0DecProd, kF0DecMap, kF0DecSlots };
enum TempoSlot { kTempoFlux, kTempoCurve, kTempoSlots };
enum ContourSlot { kContourPart, kContourRec, kContourSlots };  // (the records: where the caller wants the statistics alone)
enum JobSlot { kJobsIn, kJobsOut, kJobSlots };
enum DenoiseSlot { kDenoiseRows, kDenoisePrint, kDenoiseSlots };  // (the power rows of a learned print; the print a launch reads)
enum CompressSlot { kCompressPeaks, kCompressCurve, kCompressTable, kCompressSlots };  // (step peaks, the s_b curve, the 2049 targets)

// Arrays handed to the caller, who frees them with mx_free.  add(): a fresh malloc block of n elements (at least one, so an
// empty result is not a null pointer), copied from src or, src null, left for a download.  give(): every block is there and
// the caller's pointers are set, or MX_ERR_NOMEM; whatever was not given is freed on every path out.
class HandOver {
  void *blk_[4] = {}, *out_[4] = {};
  int n_ = 0;
  bool ok_ = true;

 public:
  HandOver() = default;
  HandOver(const HandOver &) = delete;
  HandOver &operator=(const HandOver &) = delete;
  ~HandOver() {
    for (int i = 0; i < n_; ++i) free(blk_[i]);
  }
  template <class T>
  T *add(T **out, const T *src, size_t n) {
    T *p = static_cast<T *>(malloc(std::max<size_t>(n, 1) * sizeof(T)));
    if (p && src && n) memcpy(p, src, n * sizeof(T));
    ok_ = ok_ && p;
    blk_[n_] = p;
    out_[n_++] = out;
    return p;
  }
  bool ok() const { return ok_; }
  int give() {
    if (!ok_) return fail(MX_ERR_NOMEM, "out of host memory");
    for (int i = 0; i < n_; ++i) memcpy(out_[i], &blk_[i], sizeof(void *));
    n_ = 0;
    return MX_OK;
  }
};
// the records of `v` as one such array at *out, their number at *nout (`null_if_empty`: no records, no array)
template <class T>
int hand_over(const std::vector<T> &v, T **out, int64_t *nout, bool null_if_empty = false) {
  HandOver h;
  if (null_if_empty && v.empty()) *out = nullptr;
  else h.add(out, v.data(), v.size());
  if (const int rc = h.give()) return rc;
  *nout = (int64_t)v.size();
  return MX_OK;
}

// the parameters in force: the caller's or, p null, the defaults; and the body of every mx_*_params_default
template <class P>
P params_or(const P *p, const P &defaults) { return p ? *p : defaults; }
template <class P>
void params_default(P *p, const P &defaults) { if (p) *p = defaults; }

// A table built on the host as device memory at *out (D: the device's name for T, float2 for cpx_h); nothing is left allocated
// where it fails.
template <class T, class D>
int upload_table(const std::vector<T> &host, D **out) {
  static_assert(sizeof(T) == sizeof(D), "the device reads the host's elements as they are");
  D *d = nullptr;
  hipError_t e = hipMalloc(&d, host.size() * sizeof(T));
  if (e == hipSuccess) e = hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    hipFree(d);
    return fail(MX_ERR_DEVICE, "table upload: %s", hipGetErrorString(e));
  }
  *out = d;
  return MX_OK;
}

// MELONIX_TIMING: the phases of one call, for the one line it prints on stderr.  mark() ends a phase; ms(i) is the length of
// phase i — up to now for the one still running, 0 for one the call never reached.
class PhaseClock {
  using clk = std::chrono::steady_clock;
  clk::time_point t_[6];
  int n_ = 1;

 public:
  const bool on = getenv("MELONIX_TIMING") != nullptr;
  PhaseClock() { t_[0] = clk::now(); }
  void mark() { t_[n_++] = clk::now(); }
  double ms(int i) const {
    if (i >= n_) return 0.;
    return std::chrono::duration<double, std::milli>((i + 1 < n_ ? t_[i + 1] : clk::now()) - t_[i]).count();
  }
};

struct PvPipe;  // pv_pipe.h: the phase vocoder's work arena, streams and events

}  // namespace mx

struct mx_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::map<int, mx::NTables> tables;
  std::map<std::pair<int, int>, float *> wtabs;  // (N, hop) -> forward weights
  int frames_per_block = 0;  // 0 = per-N default
  float2 *onset_tw = nullptr;  // the 1024-point transform's twiddles (onset_table), built on first use under mu
  float *chroma_hann = nullptr;  // the chroma frame's window (chroma_window), built on first use under mu
  std::map<std::pair<int, int>, float *> rtabs;  // (L, M) -> the resampler's taps, a row per tap index (resample_table_dev)
  std::mutex mu;
  // Device memory kept between calls, one WorkMem each (for_each_work names them all; mx_ctx_release_scratch gives them back).
  // stage: staging of the host-pointer entry points (mx_stft_ranges, mx_stft_hop, mx_stft_ranges_rgb*, mx_rows_colormap, mx_f0_track,
  // mx_f0_candidates, mx_f0_decode, mx_f0_track_decoded, mx_onset_flux, mx_sib_features, mx_sibilants_detect, mx_chroma, mx_contour_cents,
  // mx_contour_split, mx_pitch_contour, mx_loudness_steps, mx_loudness_measure, mx_true_peak_steps, mx_true_peak_measure): one
  // host-staged call per context at a time
  mx::WorkMem<mx::kStageSlots> stage;
  // chain: work buffers of the grain chain (mx_grains_dev).  Its lock also guards zc_scratch, the host landing zone of the zero-
  // crossing bitmaps: a copy into pages that are already mapped runs at PCIe rate, a fresh 2 x n/8-byte buffer pays ~3 ms of faults
  mx::WorkMem<mx::kChainSlots> chain;
  mx::ZcBitmaps zc_scratch;
  // f0dec: work buffers of the f0 decode (mx_f0_decode*).  Its lock also guards f0_chunk (0: the default chunk length)
  mx::WorkMem<mx::kF0DecSlots> f0dec;
  int64_t f0_chunk = 0;
  // tempo, contour: work buffers of the tempo estimate (capi_tempo.cpp) and of the pitch-contour split (capi_contour.cpp); jobs: the
  // job list and the results of a job-list call (job_pass: combs, chroma sums, contour spans)
  mx::WorkMem<mx::kTempoSlots> tempo;
  mx::WorkMem<mx::kContourSlots> contour;
  mx::WorkMem<mx::kJobSlots> jobs;
  // denoise: the power rows of mx_noise_print* and the print mx_denoise* and mx_audio_denoise hand their launch (capi_denoise.cpp)
  mx::WorkMem<mx::kDenoiseSlots> denoise;
  // compress: the step peaks and the gain curve of the groups a call touches, and the curve's table (capi_compress.cpp)
  mx::WorkMem<mx::kCompressSlots> compress;
  // the phase vocoder's bounded work arena, second stream and events (capi_pv_arena.cpp): built on first use, kept for the next
  // call, released by mx_ctx_release_scratch / mx_ctx_destroy; pv_chunk_frames = 0: the default chunk length
  std::mutex pv_mu;
  mx::PvPipe *pv = nullptr;
  int64_t pv_chunk_frames = 0;
  // the arena's budget: set (mx_pv_set_arena_budget; 0 = not set) and the automatic one (a quarter of the free device memory when
  // the context first needed an arena; forgotten by mx_ctx_release_scratch)
  int64_t pv_budget_bytes = 0, pv_budget_auto = 0;
  // a signal overflowed the compact record regions once: the context's arenas are laid out with full-size regions from then on
  // (until mx_ctx_release_scratch)
  bool pv_rec_full = false;
};

struct mx_audio {
  float *d_padded = nullptr;
  int64_t n = 0;
  bool owned = false;
};

namespace mx {

int default_frames_per_block(int N, int mode, int hop, int64_t count);
int get_tables(mx_ctx *ctx, int N, NTables &out);
int get_wtab(mx_ctx *ctx, int N, int hop, const NTables &nt, const float **out);
int check_common(mx_ctx *ctx, const mx_audio *a, int N, int64_t count, int &kmin, int &kmax);
// What the per-frame track entry points (f0, onset strength) check of a frame span: the handles, hop in [1, 16384] — file_frames,
// which gives the ceil(n / hop) frames of the file —, [first_frame, first_frame + count) inside them, and `out`, the output the
// entry point cannot do without, null only where count is 0.  (The STFT's hop mode keeps stft_hop_check: other rules.)
int file_frames(const mx_ctx *ctx, const mx_audio *a, int hop, int64_t &frames);
int frame_span(const mx_ctx *ctx, const mx_audio *a, int hop, int64_t first_frame, int64_t count, const void *out);
// The 1024-point transform's twiddle table (capi_onset.cpp): W1024^j, j < 1024, in HBM, built on the context's first use and kept
// until it goes.  Onset strength and sibilant features share it.
int onset_table(mx_ctx *ctx, const float2 **out);
// The chroma frame's window (capi_key.cpp): periodic Hann over 4096 samples, pre-scaled by 1/2048, in HBM, built on the context's
// first use and kept until it goes.
int chroma_window(mx_ctx *ctx, const float **out);
// The sample-rate conversion's pieces that its entry points (capi_resample.cpp) and mx_audio_resample (capi_audio.cpp) share:
// the plan of a rate pair or its refusal, worded once; the plan's tap table in HBM (a row per tap index), built on the context's
// first use of (L, M) and kept until it goes, null for equal rates; and outputs [first, first + count) queued on the context's
// stream — the kernel, or for equal rates a copy of the input's bytes.
int resample_plan_check(int inRate, int outRate, mx_resample_plan &p);
int resample_table_dev(mx_ctx *ctx, const mx_resample_plan &p, const float **out);
hipError_t resample_enqueue(mx_ctx *ctx, const mx_audio *a, const mx_resample_plan &p, const float *d_table, int64_t first,
                            int64_t count, float *d_out);
// The noise reduction's pieces that its entry points (capi_denoise.cpp) and mx_audio_denoise (capi_audio.cpp) share: the check of
// the parameters and the print, worded once, -> the two factors; and outputs [first, first + count) queued on the context's stream,
// the host print copied into the context's work memory in front of the launch.
int denoise_check(const float *print, const mx_denoise_params *params, float *floor, float *sens);
int denoise_enqueue(mx_ctx *ctx, const mx_audio *a, const float *print, float floor, float sens, int64_t first, int64_t count,
                    float *d_f32, int16_t *d_i16);
// The compressor's pieces that its entry points (capi_compress.cpp) and mx_audio_compress (capi_audio.cpp) share: the check of the
// rate and the parameters (null: the defaults), worded once, -> the parameters in force and their plan; and outputs [first, first +
// count) queued on the context's stream: the peaks and the curve of the groups the range touches, in the context's work memory,
// then the product.
int compress_check(int sampleRate, const mx_compress_params *params, mx_compress_params &p, mx_compress_plan &plan);
int compress_enqueue(mx_ctx *ctx, const mx_audio *a, const mx_compress_params &p, const mx_compress_plan &plan, int64_t first,
                     int64_t count, float *d_f32, int16_t *d_i16);
int stft_launch(mx_ctx *ctx, const mx_audio *a, int N, int mode, int hop, int64_t first_frame, const int32_t *d_ranges,
                int64_t count, int kmin, int kmax, float *d_mags, mx_pitch *d_pitch, uint8_t *d_rgb, float cmap_k,
                int run_length = 0);
// frames per host-staging chunk: keep the device staging buffer <= ~1 GiB
int64_t chunk_frames(int N);
template <int K>
struct Hold {
  mx_ctx *ctx;
  WorkMem<K> &mem;
  std::lock_guard<std::mutex> lk;
  Hold(mx_ctx *c, WorkMem<K> &m) : ctx(c), mem(m), lk(m.mu) {}
  template <class T>
  int get(int slot, size_t n, T **out, const char *what) {
    GrowBuf &b = mem.buf[slot];
    const size_t bytes = n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    if (b.cap < bytes) {
      b.drop();
      const hipError_t e = hipMalloc(&b.p, bytes);
      if (e != hipSuccess) {
        hipStreamSynchronize(ctx->stream);
        mem.drop();
        return fail(MX_ERR_NOMEM, "%s: %s", what, hipGetErrorString(e));
      }
      b.cap = bytes;
    }
    *out = static_cast<T *>(b.p);
    return MX_OK;
  }
};
// Bulk jobs stage up to 1 GiB per buffer: give those back, keep what a screen of columns needs.
inline void stage_trim(Hold<kStageSlots> &stage) {
  for (GrowBuf &b : stage.mem.buf)
    if (b.cap > ((size_t)256 << 20)) b.drop();
}
// every WorkMem of a context: a new family's set is one more line here
template <class F>
void for_each_work(mx_ctx *ctx, F &&f) {
  f(ctx->stage);
  f(ctx->chain);
  f(ctx->f0dec);
  f(ctx->tempo);
  f(ctx->contour);
  f(ctx->jobs);
  f(ctx->denoise);
  f(ctx->compress);
}
// gives the phase vocoder's arena, stream and events back (capi_pv_arena.cpp); the caller holds ctx->pv_mu or owns the context
// outright (mx_ctx_destroy)
void pv_release(mx_ctx *ctx);

// One host-staged batch: `count` rows of N/2 bins, walked in chunks of chunk_frames(N) rows through the context's staging
// buffers.  Callers fill it in this order: {N, count, ranges, mags_out, pitch_out, rgb_out, d_rows}, trailing nulls left out.
struct StagedBatch {
  int N = 0;
  int64_t count = 0;
  const int32_t *ranges = nullptr;  // host (start, end) pairs, uploaded chunk by chunk; null: the call has none
  float *mags_out = nullptr;        // host outputs, each or null
  mx_pitch *pitch_out = nullptr;
  uint8_t *rgb_out = nullptr;
  float *d_rows = nullptr;  // device rows that stay resident: chunk `done` lands at d_rows + done*N/2, not in a staging buffer
};
// The host-pointer form of a row entry point: `run(done, c, d_ranges, d_mags, d_pitch, d_rgb) -> status` queues rows
// [done, done + c) on the context's stream; a device pointer is null where the batch has no such output.  Each chunk's rows
// reach the caller's buffers before the next chunk overwrites the staging buffers.
template <class F>
int staged_batch(mx_ctx *ctx, const StagedBatch &b, F &&run) {
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t row = (size_t)(b.N / 2);
  const int64_t chunk = std::min<int64_t>(b.count, chunk_frames(b.N));
  float *d_mags = nullptr;
  mx_pitch *d_pitch = nullptr;
  int32_t *d_ranges = nullptr;
  uint8_t *d_rgb = nullptr;
  Hold stage(ctx, ctx->stage);
  const char *what = "device staging buffers";
  int rc = MX_OK;
  if (b.mags_out && !b.d_rows) rc = stage.get(kStageMags, (size_t)chunk * row, &d_mags, what);
  if (rc == MX_OK && b.pitch_out) rc = stage.get(kStagePitch, (size_t)chunk, &d_pitch, what);
  if (rc == MX_OK && b.ranges) rc = stage.get(kStageRanges, (size_t)chunk * 2, &d_ranges, what);
  if (rc == MX_OK && b.rgb_out) rc = stage.get(kStageTexels, (size_t)chunk * row * 3, &d_rgb, what);
  hipError_t e = hipSuccess;
  for (int64_t done = 0; done < b.count && rc == MX_OK; done += chunk) {
    const int64_t c = std::min(chunk, b.count - done);
    if (b.d_rows) d_mags = b.d_rows + (size_t)done * row;
    if (b.ranges)
      e = hipMemcpyAsync(d_ranges, b.ranges + 2 * done, (size_t)c * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) rc = fail(MX_ERR_DEVICE, "ranges upload: %s", hipGetErrorString(e));
    if (rc == MX_OK) rc = run(done, c, d_ranges, d_mags, d_pitch, d_rgb);
    if (rc) break;
    if (b.mags_out)
      e = hipMemcpyAsync(b.mags_out + (size_t)done * row, d_mags, (size_t)c * row * sizeof(float), hipMemcpyDeviceToHost,
                         ctx->stream);
    if (e == hipSuccess && b.pitch_out)
      e = hipMemcpyAsync(b.pitch_out + done, d_pitch, (size_t)c * sizeof(mx_pitch), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && b.rgb_out)
      e = hipMemcpyAsync(b.rgb_out + (size_t)done * row * 3, d_rgb, (size_t)c * row * 3, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(MX_ERR_DEVICE, "result download: %s", hipGetErrorString(e));
  }
  stage_trim(stage);
  return rc;
}

// The host-pointer form of a PCM entry point: `to_device(d_f32, d_i16)`, its device form, fills device buffers of n samples in the
// formats the caller asked for; they reach the caller's buffers only if it succeeded.
template <class F>
int pcm_to_host(mx_ctx *ctx, int64_t n, float *f_out, int16_t *i_out, F &&to_device) {
  HIP_TRY(hipSetDevice(ctx->device));
  DeviceArray<float> f;
  DeviceArray<int16_t> i;
  hipError_t e = f.alloc(ctx->stream, f_out ? (size_t)n : 0);
  if (e == hipSuccess) e = i.alloc(ctx->stream, i_out ? (size_t)n : 0);
  if (e != hipSuccess) return fail(MX_ERR_NOMEM, "device PCM buffers: %s", hipGetErrorString(e));
  const int rc = to_device(f.p, i.p);
  if (rc) return rc;
  e = f.download(f_out);
  if (e == hipSuccess) e = i.download(i_out);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "PCM download: %s", hipGetErrorString(e));
}

// The host-pointer form of a device form that writes one array: `to_device(d) -> status` fills a device array of n elements of T,
// which reach `host` only if it succeeded.  `device_what` names the array where it cannot be had, `download_what` its way back.
template <class T, class F>
int array_to_host(mx_ctx *ctx, int64_t n, T *host, const char *device_what, const char *download_what, F &&to_device) {
  HIP_TRY(hipSetDevice(ctx->device));
  DeviceArray<T> d;
  hipError_t e = d.alloc(ctx->stream, (size_t)n);
  if (e != hipSuccess) return fail(MX_ERR_NOMEM, "%s: %s", device_what, hipGetErrorString(e));
  if (const int rc = to_device(d.p)) return rc;
  e = d.download(host);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "%s: %s", download_what, hipGetErrorString(e));
}

// One kind of per-frame record of a staged call: the staging buffer it passes through, its bytes per frame (0: the call has no
// such records, the device pointer is null), the caller's records to upload and the caller's room for the result, each or null.
struct StagedSlot {
  StageSlot slot;
  size_t frame_bytes;
  const void *in;
  void *out;
};
// The host-pointer form of a per-frame track entry point: `count` frames of every slot pass through the context's staging
// buffers, held for the whole call.  `run(d) -> status` queues the device form on the context's stream, d[i] the
// device records of slot i; the results come back only if it succeeded.  `what` names the call in a device error.  Blocks, on
// the failure path too: the uploads read the caller's memory.
template <size_t K, class F>
int staged_records(mx_ctx *ctx, int64_t count, const StagedSlot (&slots)[K], const char *what, F &&run) {
  if (count == 0) return MX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Hold stage(ctx, ctx->stage);
  void *d[K] = {};
  int rc = MX_OK;
  for (size_t i = 0; i < K && rc == MX_OK; ++i)
    if (slots[i].frame_bytes) rc = stage.get(slots[i].slot, (size_t)count * slots[i].frame_bytes, &d[i], "device staging buffers");
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < K && rc == MX_OK && e == hipSuccess; ++i)
    if (d[i] && slots[i].in)
      e = hipMemcpyAsync(d[i], slots[i].in, (size_t)count * slots[i].frame_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (rc == MX_OK && e != hipSuccess) rc = fail(MX_ERR_DEVICE, "%s upload: %s", what, hipGetErrorString(e));
  if (rc == MX_OK) rc = run(d);
  for (size_t i = 0; i < K && rc == MX_OK && e == hipSuccess; ++i)
    if (d[i] && slots[i].out)
      e = hipMemcpyAsync(slots[i].out, d[i], (size_t)count * slots[i].frame_bytes, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (rc == MX_OK && e == hipSuccess) e = es;
  if (rc == MX_OK && e != hipSuccess) rc = fail(MX_ERR_DEVICE, "%s download: %s", what, hipGetErrorString(e));
  stage_trim(stage);
  return rc;
}

// The host form of a job-list call: records that are already on the device, a host list of `njobs` jobs, `res_per_job` results of Res
// per job back at `out`.  `launch(d_jobs, d_res) -> status` queues the unit's device form on the context's stream; the jobs and the
// results pass through the context's `jobs` set, held for the call.  out null: no result buffer, d_res is null.  No jobs: MX_OK and
// nothing queued.  `what` names the call in an error.  Blocks, on every path: the upload reads the caller's memory.
template <class Job, class Res, class F>
int job_pass(mx_ctx *ctx, const char *what, const Job *jobs, int64_t njobs, size_t res_per_job, Res *out, F &&launch) {
  if (njobs == 0) return MX_OK;
  Hold work(ctx, ctx->jobs);
  Job *d_jobs = nullptr;
  Res *d_res = nullptr;
  hipError_t e = hipSetDevice(ctx->device);  // (before the buffers are had: they belong on the context's device)
  int rc = e == hipSuccess ? work.get(kJobsIn, (size_t)njobs, &d_jobs, what) : MX_OK;
  if (rc == MX_OK && e == hipSuccess && out) rc = work.get(kJobsOut, (size_t)njobs * res_per_job, &d_res, what);
  if (rc == MX_OK && e == hipSuccess) e = hipMemcpyAsync(d_jobs, jobs, (size_t)njobs * sizeof(Job), hipMemcpyHostToDevice, ctx->stream);
  if (rc == MX_OK && e == hipSuccess) rc = launch(static_cast<const Job *>(d_jobs), d_res);
  if (rc == MX_OK && e == hipSuccess && out)
    e = hipMemcpyAsync(out, d_res, (size_t)njobs * res_per_job * sizeof(Res), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (a caller's upload of the records may be in flight too)
  if (e == hipSuccess) e = es;
  if (rc == MX_OK && e != hipSuccess) rc = fail(MX_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  return rc;
}

// The head of every per-frame track call (f0, onset strength, sibilant features, chroma): the arguments its two forms share,
// checked.  A unit's own call derives from it and adds what its parameters give.
struct TrackCall {
  mx_ctx *ctx;
  const mx_audio *a;
  int sampleRate, hop;
  int64_t first_frame, count;
};
// The small argument checks, each refusal worded once: the handles every call needs (handles_check) and with them the handle a
// call hands out (handles_out_check), a device pointer's alignment (`noun`: what the message calls the memory), the hop range
// (file_frames' too), a positive sample rate, a frame count the kernels index with int32, and of a note list — `finite`: every note
// number; `ordered`: none reversed, empty or overlapping.
inline int handles_check(const mx_ctx *ctx, const mx_audio *a) {
  return ctx && a ? MX_OK : fail(MX_ERR_INVALID, "null context or audio handle");
}
inline int handles_out_check(const mx_ctx *ctx, const mx_audio *a, const void *out) {
  return ctx && a && out ? MX_OK : fail(MX_ERR_INVALID, "null context, audio handle or output");
}
inline bool misaligned(const void *p, unsigned k) { return reinterpret_cast<uintptr_t>(p) % k != 0; }
inline int align_check(const void *p, unsigned k, const char *noun) {
  return misaligned(p, k) ? fail(MX_ERR_INVALID, "%s must be %u-byte aligned", noun, k) : MX_OK;
}
inline int hop_check(int hop) { return hop >= 1 && hop <= 16384 ? MX_OK : fail(MX_ERR_INVALID, "hop %d outside [1, 16384]", hop); }
inline int rate_check(int sampleRate) { return sampleRate > 0 ? MX_OK : fail(MX_ERR_INVALID, "sample rate %d", sampleRate); }
inline int frames_i32(int64_t count) {
  return count >= 0 && count <= INT32_MAX ? MX_OK : fail(MX_ERR_INVALID, "%lld frames outside [0, INT32_MAX]", (long long)count);
}
inline int notes_check(const mx_note *notes, int64_t count, bool finite, bool ordered) {
  for (int64_t i = 0; i < count; ++i) {
    if (finite && !std::isfinite(notes[i].note)) return fail(MX_ERR_INVALID, "note %lld is not finite", (long long)i);
    if (ordered && (notes[i].end_sample <= notes[i].start_sample || (i > 0 && notes[i].start_sample <= notes[i - 1].end_sample)))
      return fail(MX_ERR_INVALID, "notes out of order or overlapping at %lld", (long long)i);
  }
  return MX_OK;
}
// the frame span (frame_span: `out`), then the sample rate
inline int track_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count, const void *out,
                       TrackCall &q) {
  if (const int rc = frame_span(ctx, a, hop, first_frame, count, out)) return rc;
  if (const int rc = rate_check(sampleRate)) return rc;
  q = TrackCall{ctx, a, sampleRate, hop, first_frame, count};
  return MX_OK;
}
// the context's pinned run length (0: the kernel's default); no track's bytes depend on it
inline int pinned_run(const mx_ctx *ctx) { return ctx->frames_per_block > 0 ? ctx->frames_per_block : 0; }
// The host form of a call with one kind of record (staged_records): `count` records of Rec pass through staging buffer `slot`
// to `out`; `launch(d_out) -> status` is the device form.
template <class Rec, class F>
int staged_track(mx_ctx *ctx, int64_t count, StageSlot slot, const char *what, Rec *out, F &&launch) {
  const StagedSlot slots[] = {{slot, sizeof(Rec), nullptr, out}};
  return staged_records(ctx, count, slots, what, [&](void *const *d) { return launch(static_cast<Rec *>(d[0])); });
}

// The head of the step-record calls (loudness records: groups of ten steps; true-peak records: steps — step_core.h): the arguments
// their two forms share, checked; `records`: how many the call writes (steps_parse: `count`; the loudness unit counts its groups').
struct StepsCall {
  mx_ctx *ctx;
  const mx_audio *a;
  int sampleRate;
  int64_t first, count, records;
};
inline bool step_rate_ok(int sr) { return sr >= step::kMinRate && sr <= step::kMaxRate; }
inline int step_rate_check(int sr) {
  return step_rate_ok(sr) ? MX_OK : fail(MX_ERR_INVALID, "sample rate %d outside [%d, %d]", sr, step::kMinRate, step::kMaxRate);
}
// what frame_span checks of frames, of a span of `unit`s ("groups", "steps"): [first, first + count) inside the file's `total`,
// and `out` null only where count is 0
inline int unit_span(const char *unit, int64_t first, int64_t count, int64_t total, const void *out) {
  if (first < 0 || count < 0 || first > total || count > total - first)
    return fail(MX_ERR_INVALID, "%s [%lld, %lld) outside the file's %lld", unit, (long long)first, (long long)(first + count),
                (long long)total);
  if (count > 0 && !out) return fail(MX_ERR_INVALID, "null output");
  return MX_OK;
}
// the handles, the sample rate, then the span against `total(n, sampleRate)` units
template <class Total>
int steps_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, const char *unit, Total &&total, int64_t first, int64_t count,
                const void *out, StepsCall &q) {
  if (const int rc = handles_check(ctx, a)) return rc;
  if (const int rc = step_rate_check(sampleRate)) return rc;
  if (const int rc = unit_span(unit, first, count, total(a->n, sampleRate), out)) return rc;
  q = StepsCall{ctx, a, sampleRate, first, count, count};
  return MX_OK;
}

// The tail of a PCM range entry point (resample, denoise, compress), after the unit's own check of its parameters: outputs [first,
// first + count) inside the unit's `total`, in the formats the caller gave room for — `f32_only`: the call has no int16 form —; of
// the device form the pointers' alignment; nothing to do for an empty range; then `enqueue(d_f32, d_i16) -> status`, the unit's
// launch on the context's stream, into the caller's device memory or through the host form.
template <class F>
int pcm_range(mx_ctx *ctx, bool device, bool f32_only, int64_t first, int64_t count, int64_t total, float *f32, int16_t *i16,
              F &&enqueue) {
  if (const int rc = unit_span("outputs", first, count, total, f32 ? (const void *)f32 : i16)) return rc;
  if (device && f32_only) {
    if (const int rc = align_check(f32, 4, "device samples")) return rc;
  } else if (device && (misaligned(f32, 4) || misaligned(i16, 2))) {
    return fail(MX_ERR_INVALID, "device samples must be 4-byte (f32) and 2-byte (int16) aligned");
  }
  if (count == 0) return MX_OK;
  if (!device && f32_only)
    return array_to_host(ctx, count, f32, "device samples", "sample download", [&](float *d) { return enqueue(d, nullptr); });
  if (!device) return pcm_to_host(ctx, count, f32, i16, enqueue);
  HIP_TRY(hipSetDevice(ctx->device));
  return enqueue(f32, i16);
}

// A measure of a whole take: room for `count` records on the host (at least one), `parse(rec, q) -> status` the unit's parse of
// the whole file into its call head, `host(q, rec) -> status` its host form, then `reduce(rec) -> status` on the host.
template <class Call, class Rec, class Parse, class Host, class Reduce>
int whole_take(int64_t count, Parse &&parse, Host &&host, Reduce &&reduce) {
  std::vector<Rec> rec((size_t)std::max<int64_t>(count, 1));
  Call q;
  if (const int rc = parse(rec.data(), q)) return rc;
  if (const int rc = host(q, rec.data())) return rc;
  return reduce(rec.data());
}

}  // namespace mx
