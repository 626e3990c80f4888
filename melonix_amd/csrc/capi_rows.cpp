// capi_rows.cpp — device-resident magnitude rows (Spec's device-side row cache) and the colormap.
// One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  There is no CPU compute path:
// every transform entry point needs a live gfx950 device and fails with MX_ERR_DEVICE otherwise.
#include "capi_internal.h"

using namespace mx;

extern "C" {

// ---- device-resident magnitude rows (Spec's device-side row cache) ---------------------------------
struct mx_rows {
  int N = 0;
  int device = 0;
  int64_t count = 0;
  float *d = nullptr;  // count x N/2
  // (a plain hipFree, which synchronises the device itself: kept rows outlive mx_ctx_set_stream changes, no stream is theirs)
  ~mx_rows() { hipFree(d); }
};

int mx_stft_ranges_keep(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count, float k,
                        float *mags_out, uint8_t *rgb_out, mx_rows **rows_out) {
  return mx_guard([&]() -> int {
    if (rows_out) *rows_out = nullptr;
    int kmin = -1, kmax = -1;
    int rc = check_common(ctx, a, N, count, kmin, kmax);
    if (rc) return rc;
    if (!rows_out) return fail(MX_ERR_INVALID, "rows_out is null");
    if (count == 0) return MX_OK;
    if (!ranges) return fail(MX_ERR_INVALID, "ranges is null");
    const bool want_rgb = rgb_out != nullptr && k != 0.f;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = (size_t)(N / 2);
    std::unique_ptr<mx_rows> keep(new (std::nothrow) mx_rows);
    if (!keep) return fail(MX_ERR_NOMEM, "host memory");
    keep->N = N;
    keep->device = ctx->device;
    keep->count = count;
    hipError_t e = hipMalloc((void **)&keep->d, (size_t)count * row * sizeof(float));
    if (e != hipSuccess) return fail(MX_ERR_NOMEM, "device rows (%lld x %zu floats): %s", (long long)count, row, hipGetErrorString(e));
    const StagedBatch b{N, count, ranges, mags_out, nullptr, want_rgb ? rgb_out : nullptr, keep->d};
    rc = staged_batch(ctx, b, [&](int64_t, int64_t c, const int32_t *d_ranges, float *d_mags, mx_pitch *, uint8_t *d_rgb) {
      return want_rgb ? mx_stft_ranges_rgb_dev(ctx, a, N, d_ranges, c, k, d_mags, d_rgb)
                      : mx_stft_ranges_dev(ctx, a, N, d_ranges, c, -1, -1, d_mags, nullptr);
    });
    if (rc) return rc;
    *rows_out = keep.release();
    return MX_OK;
  });
}

int64_t mx_rows_count(const mx_rows *rows) {
  return mx_guard([&]() -> int64_t {
    return rows ? rows->count : 0;
  });
}

void mx_rows_free(mx_ctx *ctx, mx_rows *rows) {
  mx_guard_void([&] {
    if (!rows) return;
    if (ctx) hipSetDevice(ctx->device);
    delete rows;
  });
}

namespace {
int rows_span_ok(mx_ctx *ctx, const mx_rows *rows, int64_t first, int64_t count, const void *out) {
  if (!ctx || !rows) return fail(MX_ERR_INVALID, "null context / rows");
  if (rows->device != ctx->device) return fail(MX_ERR_INVALID, "rows belong to another device");
  if (first < 0 || count < 0 || first + count > rows->count) return fail(MX_ERR_INVALID, "row span outside the batch");
  if (count > 0 && !out) return fail(MX_ERR_INVALID, "output is null");
  return MX_OK;
}
}  // namespace

int mx_rows_fetch(mx_ctx *ctx, const mx_rows *rows, int64_t first, int64_t count, float *mags_out) {
  return mx_guard([&]() -> int {
    int rc = rows_span_ok(ctx, rows, first, count, mags_out);
    if (rc || count == 0) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = (size_t)(rows->N / 2);
    HIP_TRY(hipMemcpyAsync(mags_out, rows->d + (size_t)first * row, (size_t)count * row * sizeof(float), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MX_OK;
  });
}

int mx_rows_colormap(mx_ctx *ctx, const mx_rows *rows, int64_t first, int64_t count, float k, uint8_t *rgb_out) {
  return mx_guard([&]() -> int {
    int rc = rows_span_ok(ctx, rows, first, count, rgb_out);
    if (rc || count == 0) return rc;
    // the rows are where they stay: each chunk of the span is re-coloured into the texel staging buffer
    const size_t row = (size_t)(rows->N / 2);
    const StagedBatch b{rows->N, count, nullptr, nullptr, nullptr, rgb_out, rows->d + (size_t)first * row};
    return staged_batch(ctx, b, [&](int64_t, int64_t c, const int32_t *, float *d_mags, mx_pitch *, uint8_t *d_rgb) {
      HIP_TRY(launch_colormap(d_mags, d_rgb, (int64_t)c * (int64_t)row, k, ctx->stream));
      return MX_OK;
    });
  });
}

int mx_colormap_dev(mx_ctx *ctx, const float *d_mags, int64_t nbins_total, float k, uint8_t *d_rgb) {
  return mx_guard([&]() -> int {
    if (!ctx || nbins_total < 0 || (nbins_total > 0 && (!d_mags || !d_rgb))) return fail(MX_ERR_INVALID, "bad argument");
    if (nbins_total % 4) return fail(MX_ERR_INVALID, "bin count must be a multiple of 4 (whole rows)");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_colormap(d_mags, d_rgb, nbins_total, k, ctx->stream));
    return MX_OK;
  });
}

}  // extern "C"
