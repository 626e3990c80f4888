// capi_denoise.cpp — spectral noise reduction from a noise print (denoise_kernels.hip; the checks, the factors and the host form
// of the print: denoise_logic.cpp): BUILD-DEFINED, the reference has none of it.  One unit of the C-ABI implementation behind
// include/melonix_amd.h (see capi_internal.h).  (The cleaned take as a new audio object, mx_audio_denoise: capi_audio.cpp.)
#include "capi_internal.h"
#include "denoise_core.h"
#include "denoise_logic.h"

using namespace mx;

namespace mx {

int denoise_check(const float *print, const mx_denoise_params *params, float *floor, float *sens) {
  if (!print || !params) return fail(MX_ERR_INVALID, "null print or parameters");
  if (const char *why = denoise_params_error(*params)) return fail(MX_ERR_INVALID, "%s", why);
  if (const char *why = noise_print_error(print)) return fail(MX_ERR_INVALID, "%s", why);
  const DenoiseFactors f = denoise_factors(*params);
  *floor = f.floor;
  *sens = f.sens;
  return MX_OK;
}

int denoise_enqueue(mx_ctx *ctx, const mx_audio *a, const float *print, float floor, float sens, int64_t first, int64_t count,
                    float *d_f32, int16_t *d_i16) {
  if (count == 0) return MX_OK;
  DenoiseArgs g{};
  if (const int rc = onset_table(ctx, &g.tw)) return rc;
  Hold w(ctx, ctx->denoise);
  float *d_print = nullptr;
  if (const int rc = w.get(kDenoisePrint, (size_t)dn::kBins, &d_print, "noise print")) return rc;
  // (behind whatever launch still reads the buffer: the same stream)
  HIP_TRY(hipMemcpyAsync(d_print, print, dn::kBins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  g.image = a->d_padded;
  g.n = a->n;
  g.print = d_print;
  g.sens = sens;
  g.floor = floor;
  g.first = first;
  g.count = count;
  g.f32 = d_f32;
  g.i16 = d_i16;
  g.run = pinned_run(ctx);
  HIP_TRY(launch_denoise(g, ctx->stream));
  return MX_OK;
}

}  // namespace mx

namespace {

// the two range forms: the unit's own checks -> the two factors, then the tail
int range_call(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, int64_t first, int64_t count,
               float *f32, int16_t *i16, bool device) {
  if (const int rc = handles_check(ctx, a)) return rc;
  float floor = 0.f, sens = 0.f;
  if (const int rc = denoise_check(print, params, &floor, &sens)) return rc;
  return pcm_range(ctx, device, false, first, count, a->n, f32, i16, [&](float *d_f32, int16_t *d_i16) {
    return denoise_enqueue(ctx, a, print, floor, sens, first, count, d_f32, d_i16);
  });
}

int rows_launch(mx_ctx *ctx, const mx_audio *a, int64_t first_frame, int64_t count, float *d_rows) {
  if (count == 0) return MX_OK;
  NoiseRowsArgs g{};
  if (const int rc = onset_table(ctx, &g.tw)) return rc;
  g.image = a->d_padded;
  g.n = a->n;
  g.first_frame = first_frame;
  g.count = count;
  g.rows = d_rows;
  g.run = pinned_run(ctx);
  HIP_TRY(launch_noise_rows(g, ctx->stream));
  return MX_OK;
}

// the region's frames, or its refusal
int region_parse(mx_ctx *ctx, const mx_audio *a, int64_t begin, int64_t end, const void *out, int64_t *first_frame, int64_t *count) {
  if (const int rc = handles_out_check(ctx, a, out)) return rc;
  if (!noise_region_frames(a->n, begin, end, first_frame, count))
    return fail(MX_ERR_INVALID, "samples [%lld, %lld): a region inside the take's %lld samples with 1 to %d whole frames of %d", (long long)begin,
                (long long)end, (long long)a->n, dn::kMaxPrintFrames, dn::kN);
  return MX_OK;
}

// the device form: the rows into the context's work memory, their print to d_print
int print_launch(mx_ctx *ctx, const mx_audio *a, int64_t first_frame, int64_t count, float *d_print) {
  if (const int rc = align_check(d_print, 4, "a device print")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  Hold w(ctx, ctx->denoise);
  float *d_rows = nullptr;
  if (const int rc = w.get(kDenoiseRows, (size_t)count * dn::kBins, &d_rows, "noise power rows")) return rc;
  if (const int rc = rows_launch(ctx, a, first_frame, count, d_rows)) return rc;
  HIP_TRY(launch_noise_print(d_rows, count, d_print, ctx->stream));
  return MX_OK;
}

}  // namespace

extern "C" {

int64_t mx_denoise_frames(int64_t n) {
  return mx_guard([&]() -> int64_t {
    if (n < 0) return fail(MX_ERR_INVALID, "negative length");
    return dn::frames_of(n);
  });
}

int mx_denoise_factors(const mx_denoise_params *params, float *out) {
  return mx_guard([&]() -> int {
    if (!params || !out) return fail(MX_ERR_INVALID, "null parameters or output");
    if (const char *why = denoise_params_error(*params)) return fail(MX_ERR_INVALID, "%s", why);
    const DenoiseFactors f = denoise_factors(*params);
    out[0] = f.floor;
    out[1] = f.sens;
    return MX_OK;
  });
}

int mx_noise_rows_dev(mx_ctx *ctx, const mx_audio *a, int64_t first_frame, int64_t count, float *d_rows) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_check(ctx, a)) return rc;
    if (const int rc = unit_span("frames", first_frame, count, dn::frames_of(a->n), d_rows)) return rc;
    if (const int rc = align_check(d_rows, 4, "device rows")) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return rows_launch(ctx, a, first_frame, count, d_rows);
  });
}

int mx_noise_print_rows(const float *rows, int64_t count, float *print) {
  return mx_guard([&]() -> int {
    if (!rows || !print) return fail(MX_ERR_INVALID, "null rows or output");
    if (count < 1 || count > dn::kMaxPrintFrames) return fail(MX_ERR_INVALID, "%lld rows outside [1, %d]", (long long)count, dn::kMaxPrintFrames);
    noise_print_of_rows(rows, count, print);
    return MX_OK;
  });
}

int mx_noise_print_dev(mx_ctx *ctx, const mx_audio *a, int64_t begin, int64_t end, float *d_print) {
  return mx_guard([&]() -> int {
    int64_t f0 = 0, count = 0;
    if (const int rc = region_parse(ctx, a, begin, end, d_print, &f0, &count)) return rc;
    return print_launch(ctx, a, f0, count, d_print);
  });
}

int mx_noise_print(mx_ctx *ctx, const mx_audio *a, int64_t begin, int64_t end, float *print) {
  return mx_guard([&]() -> int {
    int64_t f0 = 0, count = 0;
    if (const int rc = region_parse(ctx, a, begin, end, print, &f0, &count)) return rc;
    return array_to_host(ctx, dn::kBins, print, "device print", "print download",
                         [&](float *d_print) { return print_launch(ctx, a, f0, count, d_print); });
  });
}

int mx_denoise_dev(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, int64_t first,
                   int64_t count, float *d_f32, int16_t *d_i16) {
  return mx_guard([&]() -> int { return range_call(ctx, a, print, params, first, count, d_f32, d_i16, true); });
}

int mx_denoise(mx_ctx *ctx, const mx_audio *a, const float *print, const mx_denoise_params *params, int64_t first, int64_t count,
               float *f32_out, int16_t *i16_out) {
  return mx_guard([&]() -> int { return range_call(ctx, a, print, params, first, count, f32_out, i16_out, false); });
}

}  // extern "C"
