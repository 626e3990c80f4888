// capi_compress.cpp — the dynamics compressor and its gain-reduction curve (compress_kernels.hip; the checks, the plan and the
// curve's table: compress_logic.cpp): BUILD-DEFINED, the reference has none of it.  One unit of the C-ABI implementation behind
// include/melonix_amd.h (see capi_internal.h).  (The compressed take as a new audio object, mx_audio_compress: capi_audio.cpp.)
#include "capi_internal.h"
#include "compress_core.h"
#include "compress_logic.h"

using namespace mx;

namespace {

// s_u of steps [u_lo, u_hi], inside [0, total), queued on the context's stream: the table to the device, the peaks of the groups
// that hold those steps and of their warm-ups into work memory, then the groups' recurrences.  Their own steps inside
// [out_first, out_end) land at out[u - out_first]; out null: in work memory, for every step of the groups, at
// (*curve)[u - *curve_first].  The caller holds `w`.
int curve_enqueue(Hold<kCompressSlots> &w, mx_ctx *ctx, const mx_audio *a, const mx_compress_params &p, const mx_compress_plan &plan,
                  int64_t u_lo, int64_t u_hi, int32_t *out, int64_t out_first, int64_t out_end, const int32_t **curve,
                  int64_t *curve_first) {
  const int64_t total = cp::curve_steps(a->n, plan.D, plan.K);
  const int64_t g0 = u_lo / cp::kGroup, g1 = u_hi / cp::kGroup + 1;
  const int64_t pk_first = cp::group_start(g0, plan.W), pk_end = cp::group_end(g1 - 1, total);
  int32_t table[cp::kCurve];
  compress_curve(p, table);
  int32_t *d_table = nullptr;
  float *d_peaks = nullptr;
  if (const int rc = w.get(kCompressTable, (size_t)cp::kCurve, &d_table, "compressor table")) return rc;
  if (const int rc = w.get(kCompressPeaks, (size_t)(pk_end - pk_first), &d_peaks, "compressor peaks")) return rc;
  if (!out) {
    int32_t *d_curve = nullptr;
    out_first = g0 * cp::kGroup, out_end = pk_end;
    if (const int rc = w.get(kCompressCurve, (size_t)(out_end - out_first), &d_curve, "compressor gain curve")) return rc;
    out = d_curve;
    *curve = d_curve;
    *curve_first = out_first;
  }
  // (behind whatever launch still reads the buffer: the same stream)
  HIP_TRY(hipMemcpyAsync(d_table, table, sizeof table, hipMemcpyHostToDevice, ctx->stream));
  CompressPeaksArgs k{};
  k.image = a->d_padded;
  k.n = a->n;
  k.D = plan.D;
  k.first_step = pk_first;
  k.nsteps = pk_end - pk_first;
  k.out = d_peaks;
  HIP_TRY(launch_compress_peaks(k, ctx->stream));
  CompressCurveArgs c{};
  c.peaks = d_peaks;
  c.peaks_first = pk_first;
  c.table = d_table;
  c.c_att = plan.c_att;
  c.c_rel = plan.c_rel;
  c.W = plan.W;
  c.g0 = g0;
  c.groups = g1 - g0;
  c.total = total;
  c.out = out;
  c.out_first = out_first;
  c.out_end = out_end;
  HIP_TRY(launch_compress_curve(c, ctx->stream));
  return MX_OK;
}

// what the two curve forms check of their arguments
int gain_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first_step, int64_t nsteps,
               const void *out, mx_compress_params &p, mx_compress_plan &plan) {
  if (const int rc = handles_check(ctx, a)) return rc;
  if (const int rc = compress_check(sampleRate, params, p, plan)) return rc;
  return unit_span("steps", first_step, nsteps, cp::steps_of(a->n, plan.D), out);
}

int gain_enqueue(mx_ctx *ctx, const mx_audio *a, const mx_compress_params &p, const mx_compress_plan &plan, int64_t first_step,
                 int64_t nsteps, int32_t *d_gain) {
  Hold w(ctx, ctx->compress);
  return curve_enqueue(w, ctx, a, p, plan, first_step, first_step + nsteps - 1, d_gain, first_step, first_step + nsteps, nullptr,
                       nullptr);
}

}  // namespace

namespace mx {

int compress_check(int sampleRate, const mx_compress_params *params, mx_compress_params &p, mx_compress_plan &plan) {
  if (const int rc = step_rate_check(sampleRate)) return rc;
  p = params_or(params, compress_defaults());
  if (const char *why = compress_params_error(p)) return fail(MX_ERR_INVALID, "%s", why);
  plan = compress_plan(sampleRate, p);
  return MX_OK;
}

int compress_enqueue(mx_ctx *ctx, const mx_audio *a, const mx_compress_params &p, const mx_compress_plan &plan, int64_t first,
                     int64_t count, float *d_f32, int16_t *d_i16) {
  if (count == 0) return MX_OK;
  Hold w(ctx, ctx->compress);
  CompressApplyArgs g{};
  if (const int rc = curve_enqueue(w, ctx, a, p, plan, cp::gain_lo(first, plan.D, plan.K), cp::gain_hi(first, count, plan.D, plan.K),
                                   nullptr, 0, 0, &g.curve, &g.curve_first))
    return rc;
  g.image = a->d_padded;
  g.n = a->n;
  g.D = plan.D;
  g.K = plan.K;
  g.makeup = p.makeup_amp;
  g.first = first;
  g.count = count;
  g.f32 = d_f32;
  g.i16 = d_i16;
  HIP_TRY(launch_compress_apply(g, ctx->stream));
  return MX_OK;
}

}  // namespace mx

namespace {

// the two range forms: the unit's own checks -> the parameters in force and their plan, then the tail
int range_call(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first, int64_t count,
               float *f32, int16_t *i16, bool device) {
  if (const int rc = handles_check(ctx, a)) return rc;
  mx_compress_params p;
  mx_compress_plan plan;
  if (const int rc = compress_check(sampleRate, params, p, plan)) return rc;
  return pcm_range(ctx, device, false, first, count, a->n, f32, i16, [&](float *d_f32, int16_t *d_i16) {
    return compress_enqueue(ctx, a, p, plan, first, count, d_f32, d_i16);
  });
}

}  // namespace

extern "C" {

int mx_compress_params_default(int sampleRate, mx_compress_params *p) {
  return mx_guard([&]() -> int {
    if (const int rc = step_rate_check(sampleRate)) return rc;
    if (!p) return fail(MX_ERR_INVALID, "null output");
    *p = compress_defaults();
    return MX_OK;
  });
}

int mx_compress_plan_for(int sampleRate, const mx_compress_params *params, mx_compress_plan *plan) {
  return mx_guard([&]() -> int {
    if (!plan) return fail(MX_ERR_INVALID, "null output");
    mx_compress_params p;
    mx_compress_plan q;
    if (const int rc = compress_check(sampleRate, params, p, q)) return rc;
    *plan = q;
    return MX_OK;
  });
}

int mx_compress_curve(const mx_compress_params *params, int32_t *out) {
  return mx_guard([&]() -> int {
    if (!out) return fail(MX_ERR_INVALID, "null output");
    const mx_compress_params p = params_or(params, compress_defaults());
    if (const char *why = compress_params_error(p)) return fail(MX_ERR_INVALID, "%s", why);
    compress_curve(p, out);
    return MX_OK;
  });
}

int64_t mx_compress_steps(int64_t n, int sampleRate) {
  return mx_guard([&]() -> int64_t {
    if (n < 0) return fail(MX_ERR_INVALID, "negative length");
    if (const int rc = step_rate_check(sampleRate)) return rc;
    return cp::steps_of(n, cp::step_samples(sampleRate));
  });
}

int mx_compress_peaks_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, float *d_peaks) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_check(ctx, a)) return rc;
    if (const int rc = step_rate_check(sampleRate)) return rc;
    const int D = cp::step_samples(sampleRate);
    if (const int rc = unit_span("steps", first_step, nsteps, cp::steps_of(a->n, D), d_peaks)) return rc;
    if (const int rc = align_check(d_peaks, 4, "device peaks")) return rc;
    if (nsteps == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CompressPeaksArgs k{};
    k.image = a->d_padded;
    k.n = a->n;
    k.D = D;
    k.first_step = first_step;
    k.nsteps = nsteps;
    k.out = d_peaks;
    HIP_TRY(launch_compress_peaks(k, ctx->stream));
    return MX_OK;
  });
}

int mx_compress_gain_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first_step,
                         int64_t nsteps, int32_t *d_gain) {
  return mx_guard([&]() -> int {
    mx_compress_params p;
    mx_compress_plan plan;
    if (const int rc = gain_parse(ctx, a, sampleRate, params, first_step, nsteps, d_gain, p, plan)) return rc;
    if (const int rc = align_check(d_gain, 4, "a device gain curve")) return rc;
    if (nsteps == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return gain_enqueue(ctx, a, p, plan, first_step, nsteps, d_gain);
  });
}

int mx_compress_gain(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first_step,
                     int64_t nsteps, int32_t *gain) {
  return mx_guard([&]() -> int {
    mx_compress_params p;
    mx_compress_plan plan;
    if (const int rc = gain_parse(ctx, a, sampleRate, params, first_step, nsteps, gain, p, plan)) return rc;
    if (nsteps == 0) return MX_OK;
    return array_to_host(ctx, nsteps, gain, "device gain curve", "gain curve download",
                         [&](int32_t *d_gain) { return gain_enqueue(ctx, a, p, plan, first_step, nsteps, d_gain); });
  });
}

int mx_compress_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first, int64_t count,
                    float *d_f32, int16_t *d_i16) {
  return mx_guard([&]() -> int { return range_call(ctx, a, sampleRate, params, first, count, d_f32, d_i16, true); });
}

int mx_compress(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_compress_params *params, int64_t first, int64_t count,
                float *f32_out, int16_t *i16_out) {
  return mx_guard([&]() -> int { return range_call(ctx, a, sampleRate, params, first, count, f32_out, i16_out, false); });
}

}  // extern "C"
