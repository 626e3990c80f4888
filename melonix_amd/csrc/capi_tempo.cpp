// capi_tempo.cpp — tempo and grid offset from the onset-strength curve (tempo_kernels.hip: smoothing and comb; tempo_logic.cpp:
// the estimate over them): BUILD-DEFINED, the reference has a Tempo slider and no estimator.  One unit of the C-ABI
// implementation behind include/melonix_amd.h (see capi_internal.h).
#include "capi_internal.h"
#include "tempo_logic.h"

using namespace mx;

namespace {

const char *const kWork = "tempo work memory";  // (the flux curve, the smoothed curve: held for one blocking call)

int smooth_check(const mx_ctx *ctx, const float *in, int64_t count, int width, const float *out) {
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  if (width < 0 || width > tempo::kMaxWidth) return fail(MX_ERR_INVALID, "smoothing half-width %d outside [0, 32]", width);
  if (const int rc = frames_i32(count)) return rc;
  if (count > 0 && (!in || !out)) return fail(MX_ERR_INVALID, "null argument");
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out), bytes = (uintptr_t)count * sizeof(float);
  if (count > 0 && a < b + bytes && b < a + bytes) return fail(MX_ERR_INVALID, "the smoothed curve overlaps its input");
  return MX_OK;
}

// what the two comb forms check alike: everything but the jobs themselves
int comb_check(const mx_ctx *ctx, const float *curve, int64_t count, const mx_comb_job *jobs, int64_t njobs, const mx_comb *out) {
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  if (njobs < 0) return fail(MX_ERR_INVALID, "%lld jobs", (long long)njobs);
  if (const int rc = frames_i32(count)) return rc;
  if (njobs > 0 && (!curve || !jobs || !out)) return fail(MX_ERR_INVALID, "null argument");
  if (njobs > 0 && count < 1) return fail(MX_ERR_INVALID, "jobs over an empty curve");
  return MX_OK;
}

// jobs -> records (job_pass), over a curve that is already on the device.  Blocks.
int comb_staged(mx_ctx *ctx, const float *d_curve, int64_t count, const mx_comb_job *jobs, int64_t njobs, mx_comb *out) {
  return job_pass(ctx, "comb", jobs, njobs, 1, out, [&](const mx_comb_job *d_jobs, mx_comb *d_rec) -> int {
    HIP_TRY(launch_tempo_comb(d_curve, count, d_jobs, njobs, d_rec, ctx->stream));
    return MX_OK;
  });
}

// What the two estimate entry points share: their arguments, checked
struct EstimateCall {
  mx_tempo_params p;
  TempoLadder ladder;
};
int estimate_parse(const mx_ctx *ctx, int sampleRate, int hop, const mx_tempo_params *params, const mx_tempo *out,
                   mx_tempo_window *const *windows, const int64_t *nwindows, EstimateCall &q) {
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  if (!out || (windows && !nwindows)) return fail(MX_ERR_INVALID, "null argument");
  q.p = params_or(params, kTempoDefaults);
  if (const char *why = tempo_params_error(q.p)) return fail(MX_ERR_INVALID, "tempo parameters: %s", why);
  if (const char *why = tempo_ladder(q.p, sampleRate, hop, q.ladder)) return fail(MX_ERR_INVALID, "tempo candidates: %s", why);
  return MX_OK;
}

// the flux curve at d_flux (work memory) -> the estimate: smoothing, the curve's one download, the comb launches
int estimate_staged(mx_ctx *ctx, Hold<kTempoSlots> &w, const float *d_flux, int64_t count, int64_t first_frame, const EstimateCall &q, mx_tempo *out,
                    mx_tempo_window **windows, int64_t *nwindows) {
  std::vector<float> e((size_t)count);
  float *d_curve = nullptr;
  if (count > 0) {
    if (const int rc = w.get(kTempoCurve, (size_t)count, &d_curve, kWork)) return rc;
    hipStream_t s = ctx->stream;
    HIP_TRY(launch_tempo_smooth(d_flux, count, q.p.smooth, smooth_weights(q.p.smooth), d_curve, s));
    HIP_TRY(hipMemcpyAsync(e.data(), d_curve, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  mx_tempo t{};
  std::vector<mx_tempo_window> win;
  const int rc = tempo_estimate(e.data(), count, first_frame, q.p, q.ladder,
                                [&](const std::vector<mx_comb_job> &jobs, std::vector<mx_comb> &rec) {
                                  return comb_staged(ctx, d_curve, count, jobs.data(), (int64_t)jobs.size(), rec.data());
                                },
                                t, win);
  if (rc) return rc;
  if (windows)
    if (const int rh = hand_over(win, windows, nwindows)) return rh;
  *out = t;
  return MX_OK;
}

}  // namespace

extern "C" {

void mx_tempo_params_default(mx_tempo_params *p) {
  mx_guard_void([&] { params_default(p, kTempoDefaults); });
}

int mx_tempo_smooth_dev(mx_ctx *ctx, const float *d_flux, int64_t count, int width, float *d_out) {
  return mx_guard([&]() -> int {
    if (const int rc = smooth_check(ctx, d_flux, count, width, d_out)) return rc;
    if (count == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_tempo_smooth(d_flux, count, width, smooth_weights(width), d_out, ctx->stream));
    return MX_OK;
  });
}

int mx_tempo_smooth(mx_ctx *ctx, const float *flux, int64_t count, int width, float *out) {
  return mx_guard([&]() -> int {
    if (const int rc = smooth_check(ctx, flux, count, width, out)) return rc;
    if (count == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    Hold w(ctx, ctx->tempo);
    float *d_flux = nullptr, *d_curve = nullptr;
    if (const int rc = w.get(kTempoFlux, (size_t)count, &d_flux, kWork)) return rc;
    if (const int rc = w.get(kTempoCurve, (size_t)count, &d_curve, kWork)) return rc;
    hipError_t e = hipMemcpyAsync(d_flux, flux, (size_t)count * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_tempo_smooth(d_flux, count, width, smooth_weights(width), d_curve, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_curve, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "smoothing: %s", hipGetErrorString(e));
  });
}

int mx_tempo_comb_dev(mx_ctx *ctx, const float *d_curve, int64_t count, const mx_comb_job *d_jobs, int64_t njobs, mx_comb *d_out) {
  return mx_guard([&]() -> int {
    if (const int rc = comb_check(ctx, d_curve, count, d_jobs, njobs, d_out)) return rc;
    if (njobs == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_tempo_comb(d_curve, count, d_jobs, njobs, d_out, ctx->stream));
    return MX_OK;
  });
}

int mx_tempo_comb(mx_ctx *ctx, const float *curve, int64_t count, const mx_comb_job *jobs, int64_t njobs, mx_comb *out) {
  return mx_guard([&]() -> int {
    if (const int rc = comb_check(ctx, curve, count, jobs, njobs, out)) return rc;
    for (int64_t i = 0; i < njobs; ++i)
      if (const char *why = comb_job_error(jobs[i], count)) return fail(MX_ERR_INVALID, "job %lld: %s", (long long)i, why);
    if (njobs == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    Hold w(ctx, ctx->tempo);
    float *d_curve = nullptr;
    if (const int rc = w.get(kTempoCurve, (size_t)count, &d_curve, kWork)) return rc;
    HIP_TRY(hipMemcpyAsync(d_curve, curve, (size_t)count * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return comb_staged(ctx, d_curve, count, jobs, njobs, out);
  });
}

int mx_tempo_from_flux(mx_ctx *ctx, const float *flux, int64_t count, int sampleRate, int hop, int64_t first_frame,
                       const mx_tempo_params *p, mx_tempo *out, mx_tempo_window **windows, int64_t *nwindows) {
  return mx_guard([&]() -> int {
    EstimateCall q;
    if (const int rc = estimate_parse(ctx, sampleRate, hop, p, out, windows, nwindows, q)) return rc;
    if (count < 0 || first_frame < 0 || first_frame > INT32_MAX || count > INT32_MAX || first_frame + count > INT32_MAX)
      return fail(MX_ERR_INVALID, "frames [%lld, +%lld) outside [0, INT32_MAX]", (long long)first_frame, (long long)count);
    if (count > 0 && !flux) return fail(MX_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    Hold w(ctx, ctx->tempo);
    float *d_flux = nullptr;
    if (count > 0) {
      if (const int rc = w.get(kTempoFlux, (size_t)count, &d_flux, kWork)) return rc;
      HIP_TRY(hipMemcpyAsync(d_flux, flux, (size_t)count * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    const int rc = estimate_staged(ctx, w, d_flux, count, first_frame, q, out, windows, nwindows);
    const hipError_t es = hipStreamSynchronize(ctx->stream);  // (on every path: the upload reads the caller's memory)
    return rc == MX_OK && es != hipSuccess ? fail(MX_ERR_DEVICE, "tempo estimate: %s", hipGetErrorString(es)) : rc;
  });
}

int mx_tempo_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_onset_flux_params *fp,
                    const mx_tempo_params *p, mx_tempo *out, mx_tempo_window **windows, int64_t *nwindows) {
  return mx_guard([&]() -> int {
    EstimateCall q;
    if (const int rc = estimate_parse(ctx, sampleRate, hop, p, out, windows, nwindows, q)) return rc;
    int64_t count = 0;  // (the whole file)
    if (const int rc = file_frames(ctx, a, hop, count)) return rc;
    if (const int rc = frames_i32(count)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    Hold w(ctx, ctx->tempo);
    float *d_flux = nullptr;
    if (const int rc = w.get(kTempoFlux, (size_t)count, &d_flux, kWork)) return rc;
    if (const int rc = mx_onset_flux_dev(ctx, a, sampleRate, hop, 0, count, fp, d_flux)) return rc;
    return estimate_staged(ctx, w, d_flux, count, 0, q, out, windows, nwindows);
  });
}

}  // extern "C"
