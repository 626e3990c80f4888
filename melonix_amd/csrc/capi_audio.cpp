// capi_audio.cpp — the audio objects made from another one on the device: the source gain (gain_kernels.hip), the look-ahead
// limiter (truepeak_kernels.hip), the sample-rate conversion (resample_kernels.hip; its range forms: capi_resample.cpp) and the
// noise reduction (denoise_kernels.hip; its range forms and prints: capi_denoise.cpp), the dynamics compressor
// (compress_kernels.hip; its range forms and its curve: capi_compress.cpp), and
// the download of an audio object's samples: BUILD-DEFINED, the reference has none of it.  One
// unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  (mx_audio_upload, _wrap_device, _free:
// capi_ctx.cpp.)
#include "capi_internal.h"
#include "resample_core.h"
#include "sibilant_logic.h"
#include "truepeak_core.h"

using namespace mx;

namespace {

// a device call's status as an entry point's: the error recorded the way every derived-audio call words it
int hip_status(const char *what, hipError_t e) {
  return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

// A new audio object of n samples at *out: zeroed pads, and the samples that `fill(dst) -> status` queues behind the two clears
// (not called for an empty take); a fill that fails has recorded its error.  Queued on the context's stream.  The call owns the
// buffer until the object does: on every other path out, a throw included, the stream is drained and the buffer freed.  `what`
// names the call in a device error of the clears.
template <class F>
int derived_audio(mx_ctx *ctx, int64_t length, const char *what, F &&fill, mx_audio **out) {
  if (length > 0x7fffffffLL - 2 * MX_AUDIO_PAD)  // (mx_audio_upload's bound, before anything is allocated)
    return fail(MX_ERR_INVALID, "%s: audio longer than the reference's int sample indices allow", what);
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<mx_audio> b(new mx_audio());
  const size_t n = (size_t)length, pad = (size_t)MX_AUDIO_PAD;
  DeviceArray<float> d;
  hipError_t e = d.alloc(ctx->stream, n + 2 * pad);
  if (e != hipSuccess) return fail(MX_ERR_NOMEM, "audio buffer: %s", hipGetErrorString(e));
  e = hipMemsetAsync(d.p, 0, pad * sizeof(float), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d.p + pad + n, 0, pad * sizeof(float), ctx->stream);
  if (const int rc = hip_status(what, e)) return rc;
  if (n > 0)
    if (const int rc = fill(d.p + pad)) return rc;
  b->d_padded = d.release();
  b->n = length;
  b->owned = true;
  *out = b.release();
  return MX_OK;
}

// The blocking form: `d`, the call's device array (may be empty), stays allocated until the stream has drained; its elements
// reach `host` (may be null: nothing) behind the fill; one synchronise; where that fails the new object goes the way
// mx_audio_free releases one and *out is left alone.
template <class T, class F>
int derived_audio_host(mx_ctx *ctx, int64_t length, const char *what, const DeviceArray<T> &d, T *host, F &&fill, mx_audio **out) {
  mx_audio *b = nullptr;
  if (const int rc = derived_audio(ctx, length, what, fill, &b)) return rc;
  hipError_t e = d.download(host);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    mx_audio_free(ctx, b);
    return fail(MX_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  }
  *out = b;
  return MX_OK;
}

// the samples a's (npts == 0) or a's through the gain of `d_pts`
auto gain_fill(mx_ctx *ctx, const mx_audio *a, const mx_gain_point *d_pts, int64_t npts) {
  return [=](float *dst) {
    const float *src = a->d_padded + MX_AUDIO_PAD;
    return hip_status("audio gain", npts == 0 ? hipMemcpyAsync(dst, src, (size_t)a->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream)
                                              : launch_audio_gain(src, dst, a->n, d_pts, npts, ctx->stream));
  };
}

mx_limit_params limit_defaults(int sr) {
  const int a = (sr + 100) / 200;
  return mx_limit_params{0x1.c8520ap-1f /* (float)10^(-1/20) */, a < tp::kMaxLookahead ? a : tp::kMaxLookahead};
}

// what the two limiter entry points check of their arguments -> p, the parameters in force
int limit_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out, mx_limit_params &p) {
  if (const int rc = handles_out_check(ctx, a, out)) return rc;
  if (const int rc = step_rate_check(sampleRate)) return rc;
  p = params_or(params, limit_defaults(sampleRate));
  if (!std::isnormal(p.ceiling_amp) || !(p.ceiling_amp > 0.f && p.ceiling_amp <= 1.f))
    return fail(MX_ERR_INVALID, "ceiling amplitude %g: a normal number in (0, 1]", (double)p.ceiling_amp);
  if (p.lookahead < 1 || p.lookahead > tp::kMaxLookahead)
    return fail(MX_ERR_INVALID, "look-ahead of %d samples outside [1, %d]", p.lookahead, tp::kMaxLookahead);
  return MX_OK;
}

// the samples a's through the limiter; d_pcm16 (may be null): their int16
auto limit_fill(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params &p, int16_t *d_pcm16) {
  return [=](float *dst) {
    LimitArgs g{};
    g.image = a->d_padded;
    g.n = a->n;
    g.L = tp::oversampling(sampleRate);
    g.ceiling = p.ceiling_amp;
    g.lookahead = p.lookahead;
    g.dst = dst;
    g.pcm16 = d_pcm16;
    return hip_status("audio limit", launch_audio_limit(g, ctx->stream));
  };
}

}  // namespace

extern "C" {

int mx_audio_gain_dev(mx_ctx *ctx, const mx_audio *a, const mx_gain_point *d_points, int64_t npts, mx_audio **out) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || !out || npts < 0 || (npts > 0 && !d_points)) return fail(MX_ERR_INVALID, "bad argument");
    return derived_audio(ctx, a->n, "audio gain", gain_fill(ctx, a, d_points, npts), out);
  });
}

int mx_audio_gain(mx_ctx *ctx, const mx_audio *a, const mx_gain_point *points, int64_t npts, mx_audio **out) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || !out || npts < 0 || (npts > 0 && !points)) return fail(MX_ERR_INVALID, "bad argument");
    if (const char *why = gain_points_error(points, npts)) return fail(MX_ERR_INVALID, "%s", why);
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceArray<mx_gain_point> d;
    hipError_t e = d.alloc(ctx->stream, (size_t)npts);
    if (e != hipSuccess) return fail(MX_ERR_NOMEM, "gain points: %s", hipGetErrorString(e));
    if (npts) e = hipMemcpyAsync(d.p, points, (size_t)npts * sizeof(mx_gain_point), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(MX_ERR_DEVICE, "gain points upload: %s", hipGetErrorString(e));
    return derived_audio_host(ctx, a->n, "audio gain", d, (mx_gain_point *)nullptr, gain_fill(ctx, a, d.p, npts), out);
  });
}

int mx_audio_download(mx_ctx *ctx, const mx_audio *a, int64_t first, int64_t count, float *host_out) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_check(ctx, a)) return rc;
    if (count < 0 || first < -(int64_t)MX_AUDIO_PAD || first > a->n + MX_AUDIO_PAD || count > a->n + MX_AUDIO_PAD - first)
      return fail(MX_ERR_INVALID, "samples [%lld, %lld) outside the padded audio", (long long)first, (long long)(first + count));
    if (count > 0 && !host_out) return fail(MX_ERR_INVALID, "null output");
    if (count == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(host_out, a->d_padded + MX_AUDIO_PAD + first, (size_t)count * sizeof(float), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MX_OK;
  });
}

int mx_limit_params_default(int sampleRate, mx_limit_params *p) {
  return mx_guard([&]() -> int {
    if (const int rc = step_rate_check(sampleRate)) return rc;
    if (!p) return fail(MX_ERR_INVALID, "null output");
    *p = limit_defaults(sampleRate);
    return MX_OK;
  });
}

int mx_audio_limit_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out,
                       int16_t *d_pcm16) {
  return mx_guard([&]() -> int {
    mx_limit_params p;
    if (const int rc = limit_parse(ctx, a, sampleRate, params, out, p)) return rc;
    return derived_audio(ctx, a->n, "audio limit", limit_fill(ctx, a, sampleRate, p, d_pcm16), out);
  });
}

int mx_audio_limit(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out, int16_t *pcm16_out) {
  return mx_guard([&]() -> int {
    mx_limit_params p;
    if (const int rc = limit_parse(ctx, a, sampleRate, params, out, p)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceArray<int16_t> d;
    const hipError_t e = d.alloc(ctx->stream, pcm16_out ? (size_t)a->n : 0);
    if (e != hipSuccess) return fail(MX_ERR_NOMEM, "device PCM buffer: %s", hipGetErrorString(e));
    return derived_audio_host(ctx, a->n, "audio limit", d, pcm16_out, limit_fill(ctx, a, sampleRate, p, d.p), out);
  });
}

int mx_audio_resample(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, mx_audio **out) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_out_check(ctx, a, out)) return rc;
    mx_resample_plan p;
    if (const int rc = resample_plan_check(inRate, outRate, p)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const float *d_table = nullptr;
    if (const int rc = resample_table_dev(ctx, p, &d_table)) return rc;
    const int64_t m = rs::out_length(a->n, p);
    return derived_audio(ctx, m, "audio resample", [=](float *dst) {
      return hip_status("audio resample", resample_enqueue(ctx, a, p, d_table, 0, m, dst));
    }, out);
  });
}

int mx_audio_denoise(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, mx_audio **out) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_out_check(ctx, a, out)) return rc;
    float floor = 0.f, sens = 0.f;
    if (const int rc = denoise_check(print, params, &floor, &sens)) return rc;
    return derived_audio(ctx, a->n, "audio denoise", [&](float *dst) {
      return denoise_enqueue(ctx, a, print, floor, sens, 0, a->n, dst, nullptr);
    }, out);
  });
}

int mx_audio_compress(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, mx_audio **out) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_out_check(ctx, a, out)) return rc;
    mx_compress_params p;
    mx_compress_plan plan;
    if (const int rc = compress_check(sampleRate, params, p, plan)) return rc;
    return derived_audio(ctx, a->n, "audio compress", [&](float *dst) {
      return compress_enqueue(ctx, a, p, plan, 0, a->n, dst, nullptr);
    }, out);
  });
}

}  // extern "C"
