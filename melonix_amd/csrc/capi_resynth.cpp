// capi_resynth.cpp — time maps, grains, the export schedule, granular resynthesis, WAV export.
// One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  There is no CPU compute path:
// every transform entry point needs a live gfx950 device and fails with MX_ERR_DEVICE otherwise.
#include "capi_internal.h"

using namespace mx;

extern "C" {

// ---- time maps -----------------------------------------------------------------
double mx_sample2time(const mx_marker *m, int nm, int sr, int val) {
  return mx_guard_or<double>(std::nan(""), [&]() -> double {
    return TimeMap(m, nm, sr, 0).sample2time(val);
  });
}
int mx_time2sample(const mx_marker *m, int nm, int sr, double val) {
  return mx_guard([&]() -> int {
    return TimeMap(m, nm, sr, 0).time2sample(val);
  });
}
double mx_duration(const mx_marker *m, int nm, int sr, int64_t n) {
  return mx_guard_or<double>(std::nan(""), [&]() -> double {
    return TimeMap(m, nm, sr, n).duration();
  });
}
float mx_time2pitchbend(const mx_marker *m, int nm, int sr, int64_t n, double val) {
  return mx_guard_or<float>(std::nanf(""), [&]() -> float {
    return TimeMap(m, nm, sr, n).time2pitchbend(val);
  });
}
void mx_column_range(const mx_marker *m, int nm, int sr, double time, int width, double rangeTime, int *key,
                     int *start, int *end) {
  mx_guard_void([&] {
    const TimeMap tm(m, nm, sr, 0);
    const int k = static_cast<int>(time * width / rangeTime);  // spec-cache.cpp:12
    const double st = k * rangeTime / width;                   // spec-cache.cpp:63
    const double pixelSize = rangeTime / width;                // spec-cache.cpp:64
    if (key) *key = k;
    if (start) *start = tm.time2sample(st);                    // spec-cache.cpp:65
    if (end) *end = tm.time2sample(st + pixelSize);
  });
}

// ---- grains + schedule -----------------------------------------------------------
int mx_grains(const float *host_wav, int64_t n, int32_t **starts, int32_t **lens, int64_t *count) {
  return mx_guard([&]() -> int {
    if (!starts || !lens || !count || n < 0 || (n > 0 && !host_wav)) return fail(MX_ERR_INVALID, "bad argument");
    ZcBitmaps zc;
    zc_bitmaps_host(host_wav, n, zc);
    std::vector<int32_t> s, l;
    grains_from_bitmaps(zc, s, l);
    HandOver h;
    h.add(starts, s.data(), s.size());
    h.add(lens, l.data(), l.size());
    if (const int rc = h.give()) return rc;
    *count = (int64_t)s.size();
    return MX_OK;
  });
}

int mx_grain_table_dev(mx_ctx *ctx, const mx_audio *a, int32_t **starts, int32_t **lens, float **firsts, int64_t *count) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || !starts || !lens || !count) return fail(MX_ERR_INVALID, "bad argument");
    *starts = *lens = nullptr;
    if (firsts) *firsts = nullptr;
    *count = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    PhaseClock phases;
    Hold chain(ctx, ctx->chain);
    const int64_t n = a->n;
    const size_t words = (size_t)((n + 63) >> 6);
    uint32_t ngr = 0;
    int32_t *d_s = nullptr, *d_l = nullptr;
    float *d_f = nullptr;
    if (words && n >= 1501) {  // (the reference's size_t arithmetic wraps below 1501 samples, app.cpp:161: no grains)
      uint64_t *d7 = nullptr, *d3 = nullptr;
      void *rk = nullptr, *ch = nullptr;
      const char *what = "grain chain buffers";
      if (const int rc = chain.get(kChainBitmap7, words, &d7, what)) return rc;
      if (const int rc = chain.get(kChainBitmap3, words, &d3, what)) return rc;
      if (const int rc = chain.get(kChainRanks, grain_rank_scratch_bytes(n), &rk, what)) return rc;
      HIP_TRY(launch_zc_bitmaps(a->d_padded, n, d7, d3, ctx->stream));
      HIP_TRY(launch_grain_rank(a->d_padded, n, d7, d3, rk, ctx->stream));
      uint32_t hdr[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemcpyAsync(hdr, rk, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));  // the node count sizes the lifting tables
      phases.mark();
      int levels;
      uint32_t out_cap;
      size_t bytes;
      grain_chain_sizes(n, hdr[2], &levels, &out_cap, &bytes);
      if (const int rc = chain.get(kChainTables, bytes, &ch, what)) return rc;
      HIP_TRY(launch_grain_chain(a->d_padded, n, d7, d3, rk, hdr[2], ch, &d_s, &d_l, &d_f, ctx->stream));
      HIP_TRY(hipMemcpyAsync(hdr, rk, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      phases.mark();
      ngr = hdr[1];
      if (ngr > out_cap) return fail(MX_ERR_DEVICE, "grain chain: %u grains exceed the bound %u", ngr, out_cap);
    }
    HandOver h;  // (the arrays are filled by the download: nothing to copy)
    int32_t *ps = h.add<int32_t>(starts, nullptr, ngr), *pl = h.add<int32_t>(lens, nullptr, ngr);
    float *pf = firsts ? h.add<float>(firsts, nullptr, ngr) : nullptr;
    if (!h.ok()) return h.give();
    if (ngr) {
      hipError_t e = hipMemcpyAsync(ps, d_s, (size_t)ngr * 4, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(pl, d_l, (size_t)ngr * 4, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && pf) e = hipMemcpyAsync(pf, d_f, (size_t)ngr * 4, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) return fail(MX_ERR_DEVICE, "grain table download: %s", hipGetErrorString(e));
    }
    if (phases.on)
      fprintf(stderr, "mx_grain_table_dev: bitmaps + ranks %.2f ms, chain %.2f, download of %u grains %.2f\n", phases.ms(0),
              phases.ms(1), ngr, phases.ms(2));
    *count = (int64_t)ngr;
    return h.give();
  });
}

int mx_grains_dev(mx_ctx *ctx, const mx_audio *a, int32_t **starts, int32_t **lens, int64_t *count) {
  return mx_guard([&]() -> int {
    return mx_grain_table_dev(ctx, a, starts, lens, nullptr, count);
  });
}

// the schedule from a grain table: first samples read from host_wav, or from `firsts` where the caller has no samples
static int schedule_common(const float *host_wav, const float *firsts, int64_t n, int sampleRate, const int32_t *grain_starts,
                           const int32_t *grain_lens, int64_t ngrains, const mx_marker *markers, int nmarkers,
                           double cursor0, int64_t need, mx_step **steps, int64_t *nsteps, int64_t *nsamples,
                           double *cursor_end) {
  if (!steps || !nsteps || !nsamples || n < 0 || ngrains < 0 || nmarkers < 0 ||
      (ngrains > 0 && (!grain_starts || !grain_lens)) || (nmarkers > 0 && !markers))
    return fail(MX_ERR_INVALID, "bad argument");
  PhaseClock phases;
  for (int64_t g = 0; g < ngrains; ++g)
    if (grain_starts[g] < 0 || grain_lens[g] <= 0 || (int64_t)grain_starts[g] + grain_lens[g] > n)
      return fail(MX_ERR_INVALID, "grain %lld lies outside the audio", (long long)g);
  std::vector<mx_step> v;
  std::string err;
  int64_t total = 0;
  phases.mark();
  int rc = build_schedule(host_wav, n, sampleRate, grain_starts, grain_lens, ngrains, markers, nmarkers, v, total, err,
                          cursor0, need, cursor_end, firsts);
  phases.mark();
  if (rc) return fail(rc, "%s", err.c_str());
  HandOver h;
  h.add(steps, v.data(), v.size());
  if ((rc = h.give())) return rc;
  if (phases.on)
    fprintf(stderr, "mx_schedule_build: validate %.2f ms, recurrence %.2f ms (%zu steps), hand-over %.2f ms\n", phases.ms(0),
            phases.ms(1), v.size(), phases.ms(2));
  *nsteps = (int64_t)v.size();
  *nsamples = total;
  return MX_OK;
}

int mx_schedule_build(const float *host_wav, int64_t n, int sampleRate, const int32_t *grain_starts,
                      const int32_t *grain_lens, int64_t ngrains, const mx_marker *markers, int nmarkers,
                      mx_step **steps, int64_t *nsteps, int64_t *nsamples) {
  return mx_guard([&]() -> int {
    return mx_schedule_build_from(host_wav, n, sampleRate, grain_starts, grain_lens, ngrains, markers, nmarkers, 0., -1,
                                  steps, nsteps, nsamples, nullptr);
  });
}

int mx_schedule_build_from(const float *host_wav, int64_t n, int sampleRate, const int32_t *grain_starts,
                           const int32_t *grain_lens, int64_t ngrains, const mx_marker *markers, int nmarkers,
                           double cursor0, int64_t need, mx_step **steps, int64_t *nsteps, int64_t *nsamples,
                           double *cursor_end) {
  return mx_guard([&]() -> int {
    if (n > 0 && !host_wav) return fail(MX_ERR_INVALID, "bad argument");
    return schedule_common(host_wav, nullptr, n, sampleRate, grain_starts, grain_lens, ngrains, markers, nmarkers, cursor0,
                           need, steps, nsteps, nsamples, cursor_end);
  });
}

int mx_schedule_build_table(int64_t n, int sampleRate, const int32_t *grain_starts, const int32_t *grain_lens,
                            const float *grain_firsts, int64_t ngrains, const mx_marker *markers, int nmarkers,
                            double cursor0, int64_t need, mx_step **steps, int64_t *nsteps, int64_t *nsamples,
                            double *cursor_end) {
  return mx_guard([&]() -> int {
    if (ngrains > 0 && !grain_firsts) return fail(MX_ERR_INVALID, "bad argument");
    static const float kNoGrain = 0.f;  // (an empty table: the loop never reads a first sample)
    return schedule_common(nullptr, grain_firsts ? grain_firsts : &kNoGrain, n, sampleRate, grain_starts, grain_lens, ngrains,
                           markers, nmarkers, cursor0, need, steps, nsteps, nsamples, cursor_end);
  });
}

// ---- resynthesis -------------------------------------------------------------------
int mx_resynth_dev(mx_ctx *ctx, const mx_audio *a, const mx_step *d_steps, int64_t nsteps, int64_t nsamples,
                   float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || nsteps < 0 || nsamples < 0 || (nsteps > 0 && !d_steps))
      return fail(MX_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    // Samples past the last step's run are zeros (the terminating process() calls append 1500 zeros each: one for an
    // export, ceil(missing/1500) for a playback refill — mx_schedule_build_from).  The device-resident entry point does
    // not see the schedule, so the kernel itself clears [covered, nsamples): its last workgroup knows where the steps end.
    if (nsteps == 0 && nsamples > 0) {
      if (d_pcm_f32) HIP_TRY(hipMemsetAsync(d_pcm_f32, 0, (size_t)nsamples * sizeof(float), ctx->stream));
      if (d_pcm_i16) HIP_TRY(hipMemsetAsync(d_pcm_i16, 0, (size_t)nsamples * sizeof(int16_t), ctx->stream));
    }
    ResynthArgs r{};
    r.audio = a->d_padded;
    r.steps = d_steps;
    r.nsteps = nsteps;
    r.nsamples = nsamples;
    r.pcm_f32 = d_pcm_f32;
    r.pcm_i16 = d_pcm_i16;
    HIP_TRY(launch_resynth(r, ctx->stream));
    return MX_OK;
  });
}

}  // extern "C"

namespace {
// Checks a schedule's invariants against the audio; *covered: the samples its steps emit.
int resynth_check(mx_ctx *ctx, const mx_audio *a, const mx_step *steps, int64_t nsteps, int64_t nsamples, int64_t *covered) {
  if (!ctx || !a || nsteps < 0 || nsamples < 0 || (nsteps > 0 && !steps)) return fail(MX_ERR_INVALID, "bad argument");
  *covered = 0;
  for (int64_t i = 0; i < nsteps; ++i) {
    const mx_step &s = steps[i];
    if (s.out_offset != *covered || s.sz < 0 || s.grain_start < 0 || s.grain_len <= 0 ||
        (int64_t)s.grain_start + s.grain_len > a->n)
      return fail(MX_ERR_INVALID, "step %lld is inconsistent with the schedule invariants", (long long)i);
    *covered += s.sz;
  }
  if (*covered > nsamples) return fail(MX_ERR_INVALID, "steps emit %lld samples, nsamples is %lld", (long long)*covered,
                                       (long long)nsamples);
  return MX_OK;
}
// The device half of mx_resynth / mx_resynth_to_wav behind resynth_check: uploads the schedule into d_steps and runs the kernel
// into the device PCM (either may be null), asynchronously on the context's stream.
int resynth_to_device(mx_ctx *ctx, const mx_audio *a, const mx_step *steps, int64_t nsteps, int64_t nsamples, int64_t covered,
                      DeviceArray<mx_step> &d_steps, float *d_f, int16_t *d_i) {
  HIP_TRY(hipSetDevice(ctx->device));
  hipError_t e = d_steps.alloc(ctx->stream, (size_t)nsteps);
  if (e != hipSuccess) return fail(MX_ERR_NOMEM, "device buffers: %s", hipGetErrorString(e));
  if (nsteps)
    if ((e = hipMemcpyAsync(d_steps.p, steps, (size_t)nsteps * sizeof(mx_step), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
      return fail(MX_ERR_DEVICE, "schedule upload: %s", hipGetErrorString(e));
  // anything between the covered run and the tail is zero by definition
  if (d_f) hipMemsetAsync(d_f + covered, 0, (size_t)(nsamples - covered) * sizeof(float), ctx->stream);
  if (d_i) hipMemsetAsync(d_i + covered, 0, (size_t)(nsamples - covered) * sizeof(int16_t), ctx->stream);
  return mx_resynth_dev(ctx, a, d_steps.p, nsteps, nsamples, d_f, d_i);
}
}  // namespace

extern "C" {

int mx_resynth(mx_ctx *ctx, const mx_audio *a, const mx_step *steps, int64_t nsteps, int64_t nsamples,
               float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    int64_t covered = 0;
    if (const int rc = resynth_check(ctx, a, steps, nsteps, nsamples, &covered)) return rc;
    DeviceArray<mx_step> d_steps;
    return pcm_to_host(ctx, nsamples, pcm_f32_out, pcm_i16_out, [&](float *d_f, int16_t *d_i) {
      return resynth_to_device(ctx, a, steps, nsteps, nsamples, covered, d_steps, d_f, d_i);
    });
  });
}

int mx_resynth_to_wav(mx_ctx *ctx, const mx_audio *a, const mx_step *steps, int64_t nsteps, int64_t nsamples,
                      const char *path, int sampleRate, int strict_reference_header) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || !path) return fail(MX_ERR_INVALID, "bad argument");
    int64_t covered = 0;
    int rc = resynth_check(ctx, a, steps, nsteps, nsamples, &covered);
    if (rc) return rc;
    // The PCM never exists as one host buffer: it leaves the device in 16 MiB pieces through two pinned landing
    // buffers, and each piece goes into the file while the next one is in flight.
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceArray<mx_step> d_steps;
    DeviceArray<int16_t> pcm;
    hipError_t e = pcm.alloc(ctx->stream, (size_t)nsamples);
    if (e != hipSuccess) return fail(MX_ERR_NOMEM, "device buffers: %s", hipGetErrorString(e));
    rc = resynth_to_device(ctx, a, steps, nsteps, nsamples, covered, d_steps, nullptr, pcm.p);
    WavStream ws;
    if (rc == MX_OK && wav_begin(ws, path, nsamples, sampleRate, strict_reference_header != 0) != MX_OK)
      rc = fail(MX_ERR_IO, "cannot write %s", path);
    if (rc != MX_OK) return rc;
    constexpr int64_t kPiece = 8 << 20;  // samples
    int16_t *land[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    const int64_t pieces = (nsamples + kPiece - 1) / kPiece;
    for (int i = 0; i < 2 && e == hipSuccess && i < pieces; ++i) {
      e = hipHostMalloc((void **)&land[i], (size_t)std::min<int64_t>(kPiece, nsamples) * sizeof(int16_t), hipHostMallocDefault);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    }
    auto piece_len = [&](int64_t k) { return std::min<int64_t>(kPiece, nsamples - k * kPiece); };
    for (int64_t k = 0; k <= pieces && e == hipSuccess; ++k) {
      if (k < pieces) {
        e = hipMemcpyAsync(land[k & 1], pcm.p + k * kPiece, (size_t)piece_len(k) * sizeof(int16_t), hipMemcpyDeviceToHost,
                           ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ev[k & 1], ctx->stream);
      }
      if (k > 0 && e == hipSuccess) {
        e = hipEventSynchronize(ev[(k - 1) & 1]);
        if (e == hipSuccess) wav_append(ws, land[(k - 1) & 1], piece_len(k - 1));
      }
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) rc = fail(MX_ERR_DEVICE, "PCM download: %s", hipGetErrorString(e));
    for (int i = 0; i < 2; ++i) {
      if (ev[i]) hipEventDestroy(ev[i]);
      if (land[i]) hipHostFree(land[i]);
    }
    if (wav_end(ws) != MX_OK && rc == MX_OK) rc = fail(MX_ERR_IO, "cannot write %s", path);
    return rc;
  });
}

int mx_export_wav(mx_ctx *ctx, const float *host_wav, int64_t n, int sampleRate, const mx_marker *markers,
                  int nmarkers, const char *path, int strict_reference_header) {
  return mx_guard([&]() -> int {
    if (!ctx || !path || n < 0 || (n > 0 && !host_wav)) return fail(MX_ERR_INVALID, "bad argument");
    PhaseClock phases;
    mx_audio *a = nullptr;
    int rc = mx_audio_upload(ctx, host_wav, n, &a);
    if (rc) return rc;
    phases.mark();
    int32_t *gs = nullptr, *gl = nullptr;
    int64_t ng = 0, nsteps = 0, nsamples = 0;
    mx_step *steps = nullptr;
    rc = mx_grains_dev(ctx, a, &gs, &gl, &ng);
    phases.mark();
    if (rc == MX_OK) rc = mx_schedule_build(host_wav, n, sampleRate, gs, gl, ng, markers, nmarkers, &steps, &nsteps, &nsamples);
    phases.mark();
    if (rc == MX_OK) rc = mx_resynth_to_wav(ctx, a, steps, nsteps, nsamples, path, sampleRate, strict_reference_header);
    phases.mark();
    mx_free(steps); mx_free(gs); mx_free(gl);
    mx_audio_free(ctx, a);
    if (phases.on)
      fprintf(stderr, "mx_export_wav: upload %.2f ms, grains %.2f, schedule %.2f, resynth + D2H + file %.2f, free %.2f\n",
              phases.ms(0), phases.ms(1), phases.ms(2), phases.ms(3), phases.ms(4));
    return rc;
  });
}

int mx_save_wav(const char *path, const int16_t *pcm, int64_t m, int sampleRate, int strict_reference_header) {
  return mx_guard([&]() -> int {
    const int rc = write_wav(path, pcm, m, sampleRate, strict_reference_header != 0);
    if (rc == MX_ERR_INVALID) return fail(rc, "bad argument");
    if (rc == MX_ERR_IO) return fail(rc, "cannot write %s", path);
    return rc;
  });
}

}  // extern "C"
