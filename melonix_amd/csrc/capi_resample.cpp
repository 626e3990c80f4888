// capi_resample.cpp — sample-rate conversion (resample_kernels.hip; the table: resample_logic.cpp): BUILD-DEFINED, the reference
// has none of it.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  (The converted take
// as a new audio object, mx_audio_resample: capi_audio.cpp.)
#include "capi_internal.h"
#include "resample_core.h"
#include "resample_logic.h"

using namespace mx;

namespace mx {

int resample_plan_check(int inRate, int outRate, mx_resample_plan &p) {
  if (const int rc = step_rate_check(inRate)) return rc;
  if (const int rc = step_rate_check(outRate)) return rc;
  if (rs::plan_for(inRate, outRate, &p)) return MX_OK;
  const int64_t g = rs::gcd(inRate, outRate), L = outRate / g, M = inRate / g;
  if (L > rs::kMaxPhases)
    return fail(MX_ERR_INVALID, "%d -> %d needs %lld phases, more than %d", inRate, outRate, (long long)L, rs::kMaxPhases);
  return fail(MX_ERR_INVALID, "%d -> %d (%lld / %lld) needs more than %d taps", inRate, outRate, (long long)L, (long long)M, rs::kMaxTaps);
}

int resample_table_dev(mx_ctx *ctx, const mx_resample_plan &p, const float **out) {
  *out = nullptr;
  if (p.taps == 0) return MX_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const auto key = std::make_pair((int)p.L, (int)p.M);
  auto it = ctx->rtabs.find(key);
  if (it != ctx->rtabs.end()) {
    *out = it->second;
    return MX_OK;
  }
  std::vector<float> host((size_t)p.L * p.taps);
  resample_table_by_tap(p, host.data());
  float *d = nullptr;
  if (const int rc = upload_table(host, &d)) return rc;
  ctx->rtabs[key] = d;
  *out = d;
  return MX_OK;
}

hipError_t resample_enqueue(mx_ctx *ctx, const mx_audio *a, const mx_resample_plan &p, const float *d_table, int64_t first,
                            int64_t count, float *d_out) {
  if (count == 0) return hipSuccess;
  if (p.taps == 0)
    return hipMemcpyAsync(d_out, a->d_padded + MX_AUDIO_PAD + first, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
  ResampleArgs g{};
  g.image = a->d_padded;
  g.n = a->n;
  g.plan = p;
  g.table = d_table;
  g.first_out = first;
  g.count = count;
  g.out = d_out;
  return launch_resample(g, ctx->stream);
}

}  // namespace mx

namespace {

// the two range forms: the unit's own checks -> the plan, then the tail (an empty range asks nothing of a device pointer: it is
// refused for its alignment only where something would be written through it)
int range_call(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, int64_t first_out, int64_t count, float *out, bool device) {
  if (const int rc = handles_check(ctx, a)) return rc;
  mx_resample_plan p;
  if (const int rc = resample_plan_check(inRate, outRate, p)) return rc;
  return pcm_range(ctx, device, true, first_out, count, rs::out_length(a->n, p), count ? out : nullptr, nullptr, [&](float *d_out, int16_t *) {
    const float *d_table = nullptr;
    if (const int rc = resample_table_dev(ctx, p, &d_table)) return rc;
    HIP_TRY(resample_enqueue(ctx, a, p, d_table, first_out, count, d_out));
    return (int)MX_OK;
  });
}

}  // namespace

extern "C" {

int mx_resample_plan_for(int inRate, int outRate, mx_resample_plan *out) {
  return mx_guard([&]() -> int {
    if (!out) return fail(MX_ERR_INVALID, "null output");
    mx_resample_plan p;
    if (const int rc = resample_plan_check(inRate, outRate, p)) return rc;
    *out = p;
    return MX_OK;
  });
}

int64_t mx_resample_length(int64_t n, int inRate, int outRate) {
  return mx_guard([&]() -> int64_t {
    if (n < 0) return fail(MX_ERR_INVALID, "negative length");
    mx_resample_plan p;
    if (const int rc = resample_plan_check(inRate, outRate, p)) return rc;
    return rs::out_length(n, p);
  });
}

int mx_resample_taps(int inRate, int outRate, float *out) {
  return mx_guard([&]() -> int {
    if (!out) return fail(MX_ERR_INVALID, "null output");
    mx_resample_plan p;
    if (const int rc = resample_plan_check(inRate, outRate, p)) return rc;
    if (p.taps > 0) resample_table(p, out);
    return MX_OK;
  });
}

int mx_resample_dev(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, int64_t first_out, int64_t count, float *d_out) {
  return mx_guard([&]() -> int { return range_call(ctx, a, inRate, outRate, first_out, count, d_out, true); });
}

int mx_resample(mx_ctx *ctx, const mx_audio *a, int inRate, int outRate, int64_t first_out, int64_t count, float *out) {
  return mx_guard([&]() -> int { return range_call(ctx, a, inRate, outRate, first_out, count, out, false); });
}

}  // extern "C"
