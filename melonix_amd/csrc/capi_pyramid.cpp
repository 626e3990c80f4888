// capi_pyramid.cpp — the waveform min/max pyramid (App::calcPicks, app.cpp:347-378).
// One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  There is no CPU compute path:
// every transform entry point needs a live gfx950 device and fails with MX_ERR_DEVICE otherwise.
#include "capi_internal.h"

using namespace mx;

extern "C" {

// ---- waveform pyramid ---------------------------------------------------------------------
int mx_minmax_pyramid_dev(mx_ctx *ctx, const mx_audio *a, float *d_picks, int64_t *counts_out, int *nlevels) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || !counts_out || !nlevels || (a->n > 2 && !d_picks)) return fail(MX_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_picks(a->d_padded, a->n, d_picks, counts_out, nlevels, ctx->stream));
    return MX_OK;
  });
}

int mx_minmax_pyramid(mx_ctx *ctx, const mx_audio *a, float *picks_out, int64_t *counts_out, int *nlevels) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || !counts_out || !nlevels || (a->n > 2 && !picks_out)) return fail(MX_ERR_INVALID, "bad argument");
    *nlevels = 0;
    if (a->n <= 2) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceArray<float> d;
    HIP_TRY(d.alloc(ctx->stream, (size_t)a->n * 2));
    const int rc = mx_minmax_pyramid_dev(ctx, a, d.p, counts_out, nlevels);
    if (rc) return rc;
    int64_t pairs = 0;
    for (int l = 0; l < *nlevels; ++l) pairs += counts_out[l];
    hipError_t e = d.download(picks_out, (size_t)pairs * 2);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "pyramid download: %s", hipGetErrorString(e));
  });
}

void mx_minmax_range(const float *host_wav, int64_t n, const float *picks, const int64_t *counts, int nlevels, int start,
                     int end, float *mn, float *mx) {
  mx_guard_void([&] {
    float a = 0.f, b = 0.f;
    if (host_wav && picks && counts) minmax_from_range(host_wav, n, picks, counts, nlevels, start, end, a, b);
    if (mn) *mn = a;
    if (mx) *mx = b;
  });
}
}  // extern "C"
