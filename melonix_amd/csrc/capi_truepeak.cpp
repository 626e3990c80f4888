// capi_truepeak.cpp — true-peak records (truepeak_kernels.hip): BUILD-DEFINED, the reference has none of it.  One unit of the C-ABI
// implementation behind include/melonix_amd.h (see capi_internal.h).  (The look-ahead limiter makes a new audio object:
// capi_audio.cpp.  The loudness range and the export gain under a true-peak ceiling are host logic over the loudness records:
// capi_loudness.cpp.)
#include "capi_internal.h"
#include "truepeak_core.h"

using namespace mx;

namespace {

int steps_launch(const StepsCall &q, mx_tp_step *d_steps) {
  if (q.count == 0) return MX_OK;
  if (const int rc = align_check(d_steps, 8, "device records")) return rc;
  HIP_TRY(hipSetDevice(q.ctx->device));
  TruePeakArgs g{};
  g.image = q.a->d_padded;
  g.n = q.a->n;
  g.S = tp::step_samples(q.sampleRate);
  g.L = tp::oversampling(q.sampleRate);
  g.first_step = q.first;
  g.nsteps = q.count;
  g.out = d_steps;
  HIP_TRY(launch_true_peak_steps(g, q.ctx->stream));
  return MX_OK;
}

// the host form: the records pass through the context's staging buffer of the pitch records
int steps_host(const StepsCall &q, mx_tp_step *steps_out) {
  return staged_track(q.ctx, q.records, kStagePitch, "true-peak records", steps_out, [&](mx_tp_step *d_steps) { return steps_launch(q, d_steps); });
}

}  // namespace

extern "C" {

int mx_true_peak_oversampling(int sampleRate) {
  return mx_guard([&]() -> int { return step_rate_ok(sampleRate) ? tp::oversampling(sampleRate) : 0; });
}

int mx_true_peak_taps(float *out36) {
  return mx_guard([&]() -> int {
    if (!out36) return fail(MX_ERR_INVALID, "null output");
    constexpr float taps[3][tp::kTaps] = MX_TP_TAPS;
    std::memcpy(out36, taps, sizeof(taps));
    return MX_OK;
  });
}

int mx_true_peak_steps_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, mx_tp_step *d_steps) {
  return mx_guard([&]() -> int {
    StepsCall q;
    if (const int rc = steps_parse(ctx, a, sampleRate, "steps", tp::step_count, first_step, nsteps, d_steps, q)) return rc;
    return steps_launch(q, d_steps);
  });
}

int mx_true_peak_steps(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, mx_tp_step *steps_out) {
  return mx_guard([&]() -> int {
    StepsCall q;
    if (const int rc = steps_parse(ctx, a, sampleRate, "steps", tp::step_count, first_step, nsteps, steps_out, q)) return rc;
    return steps_host(q, steps_out);
  });
}

int mx_true_peak_measure(mx_ctx *ctx, const mx_audio *a, int sampleRate, float *true_peak, float *sample_peak) {
  return mx_guard([&]() -> int {
    if (!true_peak && !sample_peak) return fail(MX_ERR_INVALID, "null output");
    if (const int rc = handles_check(ctx, a)) return rc;
    if (const int rc = step_rate_check(sampleRate)) return rc;
    const int64_t steps = tp::step_count(a->n, sampleRate);
    return whole_take<StepsCall, mx_tp_step>(
        steps, [&](mx_tp_step *rec, StepsCall &q) { return steps_parse(ctx, a, sampleRate, "steps", tp::step_count, 0, steps, rec, q); }, steps_host,
        [&](const mx_tp_step *rec) -> int {
          float t = 0.f, s = 0.f;
          for (int64_t b = 0; b < steps; ++b) {
            if (rec[b].true_peak > t) t = rec[b].true_peak;
            if (rec[b].sample_peak > s) s = rec[b].sample_peak;
          }
          if (true_peak) *true_peak = t;
          if (sample_peak) *sample_peak = s;
          return MX_OK;
        });
  });
}

}  // extern "C"
