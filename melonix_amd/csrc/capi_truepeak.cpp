// capi_truepeak.cpp — true-peak records and the look-ahead limiter (truepeak_kernels.hip): BUILD-DEFINED, the reference has none
// of it.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  (The loudness range and the
// export gain under a true-peak ceiling are host logic over the loudness records: capi_loudness.cpp.)
#include <cmath>
#include <cstring>

#include "capi_internal.h"
#include "truepeak_core.h"

using namespace mx;

namespace {

bool rate_ok(int sr) { return sr >= tp::kMinRate && sr <= tp::kMaxRate; }
int rate_check(int sr) {
  return rate_ok(sr) ? MX_OK : fail(MX_ERR_INVALID, "sample rate %d outside [%d, %d]", sr, tp::kMinRate, tp::kMaxRate);
}
mx_limit_params limit_defaults(int sr) {
  const int a = (sr + 100) / 200;
  return mx_limit_params{0x1.c8520ap-1f /* (float)10^(-1/20) */, a < tp::kMaxLookahead ? a : tp::kMaxLookahead};
}

// What the two record entry points share: their arguments, checked
struct StepsCall {
  mx_ctx *ctx;
  const mx_audio *a;
  int sampleRate;
  int64_t first_step, nsteps;
};

int steps_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, const void *out, StepsCall &q) {
  if (!ctx || !a) return fail(MX_ERR_INVALID, "null context or audio handle");
  if (const int rc = rate_check(sampleRate)) return rc;
  const int64_t steps = tp::step_count(a->n, sampleRate);
  if (first_step < 0 || nsteps < 0 || first_step > steps || nsteps > steps - first_step)
    return fail(MX_ERR_INVALID, "steps [%lld, %lld) outside the file's %lld", (long long)first_step, (long long)(first_step + nsteps),
                (long long)steps);
  if (nsteps > 0 && !out) return fail(MX_ERR_INVALID, "null output");
  q = StepsCall{ctx, a, sampleRate, first_step, nsteps};
  return MX_OK;
}

int steps_launch(const StepsCall &q, mx_tp_step *d_steps) {
  if (q.nsteps == 0) return MX_OK;
  if (reinterpret_cast<uintptr_t>(d_steps) % 8) return fail(MX_ERR_INVALID, "device records must be 8-byte aligned");
  HIP_TRY(hipSetDevice(q.ctx->device));
  TruePeakArgs g{};
  g.image = q.a->d_padded;
  g.n = q.a->n;
  g.S = tp::step_samples(q.sampleRate);
  g.L = tp::oversampling(q.sampleRate);
  g.first_step = q.first_step;
  g.nsteps = q.nsteps;
  g.out = d_steps;
  HIP_TRY(launch_true_peak_steps(g, q.ctx->stream));
  return MX_OK;
}

// the host form: the records pass through the context's staging buffer of the pitch records
int steps_host(const StepsCall &q, mx_tp_step *steps_out) {
  const StagedSlot slots[] = {{kStagePitch, sizeof(mx_tp_step), nullptr, steps_out}};
  return staged_records(q.ctx, q.nsteps, slots, "true-peak records",
                        [&](void *const *d) { return steps_launch(q, static_cast<mx_tp_step *>(d[0])); });
}

// What the two limiter entry points share: their arguments, checked
struct LimitCall {
  mx_ctx *ctx;
  const mx_audio *a;
  int sampleRate;
  mx_limit_params p;
};

int limit_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out, LimitCall &q) {
  if (!ctx || !a || !out) return fail(MX_ERR_INVALID, "null context, audio handle or output");
  if (const int rc = rate_check(sampleRate)) return rc;
  const mx_limit_params p = params_or(params, limit_defaults(sampleRate));
  if (!std::isnormal(p.ceiling_amp) || !(p.ceiling_amp > 0.f && p.ceiling_amp <= 1.f))
    return fail(MX_ERR_INVALID, "ceiling amplitude %g: a normal number in (0, 1]", (double)p.ceiling_amp);
  if (p.lookahead < 1 || p.lookahead > tp::kMaxLookahead)
    return fail(MX_ERR_INVALID, "look-ahead of %d samples outside [1, %d]", p.lookahead, tp::kMaxLookahead);
  q = LimitCall{ctx, a, sampleRate, p};
  return MX_OK;
}

// A new audio object of a's length: zeroed pads, the samples a's through the limiter; d_pcm16 (may be null): their int16.
// Queued on the context's stream; nothing is left allocated where it fails.
int limited_audio(const LimitCall &q, mx_audio **out, int16_t *d_pcm16) {
  HIP_TRY(hipSetDevice(q.ctx->device));
  std::unique_ptr<mx_audio> b(new mx_audio());
  const size_t n = (size_t)q.a->n, pad = (size_t)MX_AUDIO_PAD;
  hipError_t e = hipMalloc(&b->d_padded, (n + 2 * pad) * sizeof(float));
  if (e != hipSuccess) return fail(MX_ERR_NOMEM, "audio buffer: %s", hipGetErrorString(e));
  e = hipMemsetAsync(b->d_padded, 0, pad * sizeof(float), q.ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(b->d_padded + pad + n, 0, pad * sizeof(float), q.ctx->stream);
  if (e == hipSuccess && n > 0) {
    LimitArgs g{};
    g.image = q.a->d_padded;
    g.n = q.a->n;
    g.L = tp::oversampling(q.sampleRate);
    g.ceiling = q.p.ceiling_amp;
    g.lookahead = q.p.lookahead;
    g.dst = b->d_padded + pad;
    g.pcm16 = d_pcm16;
    e = launch_audio_limit(g, q.ctx->stream);
  }
  if (e != hipSuccess) {
    hipStreamSynchronize(q.ctx->stream);
    hipFree(b->d_padded);
    return fail(MX_ERR_DEVICE, "audio limit: %s", hipGetErrorString(e));
  }
  b->n = q.a->n;
  b->owned = true;
  *out = b.release();
  return MX_OK;
}

}  // namespace

extern "C" {

int mx_true_peak_oversampling(int sampleRate) {
  return mx_guard([&]() -> int { return rate_ok(sampleRate) ? tp::oversampling(sampleRate) : 0; });
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
    if (const int rc = steps_parse(ctx, a, sampleRate, first_step, nsteps, d_steps, q)) return rc;
    return steps_launch(q, d_steps);
  });
}

int mx_true_peak_steps(mx_ctx *ctx, const mx_audio *a, int sampleRate, int64_t first_step, int64_t nsteps, mx_tp_step *steps_out) {
  return mx_guard([&]() -> int {
    StepsCall q;
    if (const int rc = steps_parse(ctx, a, sampleRate, first_step, nsteps, steps_out, q)) return rc;
    return steps_host(q, steps_out);
  });
}

int mx_true_peak_measure(mx_ctx *ctx, const mx_audio *a, int sampleRate, float *true_peak, float *sample_peak) {
  return mx_guard([&]() -> int {
    if (!true_peak && !sample_peak) return fail(MX_ERR_INVALID, "null output");
    if (!ctx || !a) return fail(MX_ERR_INVALID, "null context or audio handle");
    if (const int rc = rate_check(sampleRate)) return rc;
    const int64_t steps = tp::step_count(a->n, sampleRate);
    std::vector<mx_tp_step> rec((size_t)std::max<int64_t>(steps, 1));
    StepsCall q;
    if (const int rc = steps_parse(ctx, a, sampleRate, 0, steps, rec.data(), q)) return rc;
    if (const int rc = steps_host(q, rec.data())) return rc;
    float t = 0.f, s = 0.f;
    for (int64_t b = 0; b < steps; ++b) {
      if (rec[(size_t)b].true_peak > t) t = rec[(size_t)b].true_peak;
      if (rec[(size_t)b].sample_peak > s) s = rec[(size_t)b].sample_peak;
    }
    if (true_peak) *true_peak = t;
    if (sample_peak) *sample_peak = s;
    return MX_OK;
  });
}

int mx_limit_params_default(int sampleRate, mx_limit_params *p) {
  return mx_guard([&]() -> int {
    if (const int rc = rate_check(sampleRate)) return rc;
    if (!p) return fail(MX_ERR_INVALID, "null output");
    *p = limit_defaults(sampleRate);
    return MX_OK;
  });
}

int mx_audio_limit_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out,
                       int16_t *d_pcm16) {
  return mx_guard([&]() -> int {
    LimitCall q;
    if (const int rc = limit_parse(ctx, a, sampleRate, params, out, q)) return rc;
    return limited_audio(q, out, d_pcm16);
  });
}

int mx_audio_limit(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_limit_params *params, mx_audio **out, int16_t *pcm16_out) {
  return mx_guard([&]() -> int {
    LimitCall q;
    if (const int rc = limit_parse(ctx, a, sampleRate, params, out, q)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceArray<int16_t> d;  // (freed once the stream has drained)
    hipError_t e = d.alloc(ctx->stream, pcm16_out ? (size_t)a->n : 0);
    if (e != hipSuccess) return fail(MX_ERR_NOMEM, "device PCM buffer: %s", hipGetErrorString(e));
    mx_audio *b = nullptr;
    if (const int rc = limited_audio(q, &b, d.p)) return rc;
    e = d.download(pcm16_out);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
      hipFree(b->d_padded);
      delete b;
      return fail(MX_ERR_DEVICE, "audio limit: %s", hipGetErrorString(e));
    }
    *out = b;
    return MX_OK;
  });
}

}  // extern "C"
