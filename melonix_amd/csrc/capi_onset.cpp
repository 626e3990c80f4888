// capi_onset.cpp — onset strength (onset_kernels.hip), peak picking and tempo-grid timing markers (onset_logic.cpp):
// BUILD-DEFINED, the reference has no detector.  One unit of the C-ABI implementation behind include/melonix_amd.h (see
// capi_internal.h).
#include "capi_internal.h"
#include "onset_logic.h"

using namespace mx;

namespace {

const mx_onset_flux_params kFluxDefaults{100.f, 1, 0.f, 0.f};
const mx_onset_pick_params kPickDefaults{3, 3, 25, 1, 8, 2.0, 1.0};
const mx_timing_params kTimingDefaults{120.0, 4, 0.0, 1.0, 0.1, 2.0};

// What the two flux entry points share: their arguments, checked, with the parameters in force and the band they give
struct FluxCall : TrackCall {
  mx_onset_flux_params p;
  int kmin, kmax;
};

// the call's head (track_parse: `out`) and what is the detector's own: the flux parameters and their band
int flux_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
               const mx_onset_flux_params *params, const void *out, FluxCall &q) {
  if (const int rc = track_parse(ctx, a, sampleRate, hop, first_frame, count, out, q)) return rc;
  const mx_onset_flux_params &p = q.p = params_or(params, kFluxDefaults);
  if (!std::isfinite(p.compress) || !(p.compress > 0.f) || p.compress > 1e6f)
    return fail(MX_ERR_INVALID, "compress %g outside (0, 1e6]", (double)p.compress);
  if (p.lag < 1 || p.lag > 4) return fail(MX_ERR_INVALID, "lag %d outside [1, 4]", p.lag);
  if (!std::isfinite(p.fmin) || !std::isfinite(p.fmax) || p.fmin < 0.f || p.fmax < 0.f)
    return fail(MX_ERR_INVALID, "flux band [%g, %g] Hz: both ends must be finite and >= 0", (double)p.fmin, (double)p.fmax);
  const double sr = (double)sampleRate, fmax = p.fmax == 0.f ? sr / 2.0 : (double)p.fmax;
  q.kmin = (int)std::max(1.0, std::min(std::ceil((double)p.fmin * 1024.0 / sr), 1024.0));
  q.kmax = (int)std::min(511.0, std::floor(fmax * 1024.0 / sr));
  if (q.kmin > q.kmax)
    return fail(MX_ERR_INVALID, "empty band [%d, %d] for %g..%g Hz at %d Hz", q.kmin, q.kmax, (double)p.fmin, fmax, sampleRate);
  return MX_OK;
}

int flux_launch(const FluxCall &q, float *d_flux) {
  if (q.count == 0) return MX_OK;
  HIP_TRY(hipSetDevice(q.ctx->device));
  OnsetArgs g{};
  if (const int rc = onset_table(q.ctx, &g.tw)) return rc;
  g.audio = q.a->d_padded;
  g.hop = q.hop;
  g.first_frame = q.first_frame;
  g.count = q.count;
  g.lag = q.p.lag;
  g.kmin = q.kmin;
  g.kmax = q.kmax;
  g.compress = q.p.compress;
  g.flux = d_flux;
  g.run = pinned_run(q.ctx);
  HIP_TRY(launch_onset_flux(g, q.ctx->stream));
  return MX_OK;
}

// the host form: the values pass through the context's staging buffer of the pitch records
int flux_host(const FluxCall &q, float *flux_out) {
  return staged_track(q.ctx, q.count, kStagePitch, "flux", flux_out, [&](float *d_flux) { return flux_launch(q, d_flux); });
}

// the parameters in force (p null: the defaults), checked
int pick_params(const mx_onset_pick_params *p, mx_onset_pick_params &out) {
  out = params_or(p, kPickDefaults);
  for (const int32_t v : {out.pre_max, out.post_max, out.pre_avg, out.post_avg, out.wait})
    if (v < 0 || v > 4096) return fail(MX_ERR_INVALID, "pick window %d outside [0, 4096]", v);
  if (!std::isfinite(out.ratio) || !std::isfinite(out.delta) || out.ratio < 0.0 || out.delta < 0.0)
    return fail(MX_ERR_INVALID, "pick ratio %g / delta %g must be finite and >= 0", out.ratio, out.delta);
  return MX_OK;
}

}  // namespace

namespace mx {

// W1024^j = e^{-2 pi i j / 1024}, j < 1024, rounded from binary64: built on the context's first flux call, kept until it goes
int onset_table(mx_ctx *ctx, const float2 **out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->onset_tw) {
    std::vector<float2> tw(1024);
    for (int j = 0; j < 1024; ++j) {
      const double ang = -2.0 * M_PI * (double)j / 1024.0;
      tw[(size_t)j] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    if (const int rc = upload_table(tw, &ctx->onset_tw)) return rc;
  }
  *out = ctx->onset_tw;
  return MX_OK;
}

}  // namespace mx

extern "C" {

void mx_onset_flux_params_default(mx_onset_flux_params *p) {
  mx_guard_void([&] { params_default(p, kFluxDefaults); });
}

int mx_onset_flux_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                      const mx_onset_flux_params *params, float *d_flux) {
  return mx_guard([&]() -> int {
    FluxCall q;
    if (const int rc = flux_parse(ctx, a, sampleRate, hop, first_frame, count, params, d_flux, q)) return rc;
    return flux_launch(q, d_flux);
  });
}

int mx_onset_flux(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                  const mx_onset_flux_params *params, float *flux_out) {
  return mx_guard([&]() -> int {
    FluxCall q;
    if (const int rc = flux_parse(ctx, a, sampleRate, hop, first_frame, count, params, flux_out, q)) return rc;
    return flux_host(q, flux_out);
  });
}

void mx_onset_pick_params_default(mx_onset_pick_params *p) {
  mx_guard_void([&] { params_default(p, kPickDefaults); });
}

int mx_onset_pick(const float *flux, int64_t count, int hop, int64_t first_frame, const mx_onset_pick_params *params,
                  mx_onset **out, int64_t *nout) {
  return mx_guard([&]() -> int {
    mx_onset_pick_params p;
    if (const int rc = pick_params(params, p)) return rc;
    if (!out || !nout || (count > 0 && !flux)) return fail(MX_ERR_INVALID, "null argument");
    if (count < 0 || first_frame < 0) return fail(MX_ERR_INVALID, "negative frame range");
    if (hop < 1) return fail(MX_ERR_INVALID, "hop %d", hop);
    if (first_frame > INT32_MAX || count > INT32_MAX || (first_frame + count) * (int64_t)hop > INT32_MAX)
      return fail(MX_ERR_INVALID, "frame centres beyond int32 samples");
    return hand_over(pick_onsets(flux, count, hop, first_frame, p), out, nout);
  });
}

int mx_onsets_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_onset_flux_params *flux_params,
                     const mx_onset_pick_params *pick_params_in, mx_onset **out, int64_t *nout) {
  return mx_guard([&]() -> int {
    mx_onset_pick_params p;
    if (const int rc = pick_params(pick_params_in, p)) return rc;
    if (!out || !nout) return fail(MX_ERR_INVALID, "null argument");
    int64_t count = 0;  // (the whole file)
    if (const int rc = file_frames(ctx, a, hop, count)) return rc;
    if (count * (int64_t)hop > INT32_MAX) return fail(MX_ERR_INVALID, "frame centres beyond int32 samples");
    std::vector<float> flux((size_t)std::max<int64_t>(count, 1));
    FluxCall q;
    if (const int rc = flux_parse(ctx, a, sampleRate, hop, 0, count, flux_params, flux.data(), q)) return rc;
    if (const int rc = flux_host(q, flux.data())) return rc;
    return hand_over(pick_onsets(flux.data(), count, hop, 0, p), out, nout);
  });
}

void mx_timing_params_default(mx_timing_params *p) {
  mx_guard_void([&] { params_default(p, kTimingDefaults); });
}

int mx_timing_markers(const int32_t *anchors, int64_t nanchors, int64_t n, int sampleRate, const mx_timing_params *params,
                      const mx_marker *base, int nbase, mx_marker **out, int64_t *nout) {
  return mx_guard([&]() -> int {
    if (!out || !nout || (nanchors > 0 && !anchors) || (nbase > 0 && !base)) return fail(MX_ERR_INVALID, "null argument");
    if (nanchors < 0 || nbase < 0) return fail(MX_ERR_INVALID, "negative count");
    if (const int rc = rate_check(sampleRate)) return rc;
    if (n < 1 || n > INT32_MAX) return fail(MX_ERR_INVALID, "%lld samples outside [1, INT32_MAX]", (long long)n);
    const mx_timing_params p = params_or(params, kTimingDefaults);
    if (!(p.bpm >= 30.0 && p.bpm <= 250.0)) return fail(MX_ERR_INVALID, "bpm %g outside [30, 250]", p.bpm);
    if (p.division < 1 || p.division > 64) return fail(MX_ERR_INVALID, "division %d outside [1, 64]", p.division);
    if (!std::isfinite(p.offset)) return fail(MX_ERR_INVALID, "offset is not finite");
    if (!(p.strength >= 0.0 && p.strength <= 1.0)) return fail(MX_ERR_INVALID, "strength %g outside [0, 1]", p.strength);
    if (!(p.max_shift >= 0.0) || !std::isfinite(p.max_shift)) return fail(MX_ERR_INVALID, "max_shift %g must be finite and >= 0", p.max_shift);
    if (!(p.max_stretch >= 1.0 && p.max_stretch <= 4.0)) return fail(MX_ERR_INVALID, "max_stretch %g outside [1, 4]", p.max_stretch);
    for (int64_t i = 0; i < nanchors; ++i)
      if (anchors[i] < 0 || anchors[i] >= n || (i > 0 && anchors[i] <= anchors[i - 1]))
        return fail(MX_ERR_INVALID, "anchor %lld out of order or outside [0, n)", (long long)i);
    for (int i = 0; i < nbase; ++i) {
      if (base[i].sample < 1 || base[i].sample >= n || (i > 0 && base[i].sample <= base[i - 1].sample))
        return fail(MX_ERR_INVALID, "base marker %d out of order or outside [1, n)", i);
      if (base[i].dTime != 0.0) return fail(MX_ERR_INVALID, "base marker %d has a time shift of its own (dTime %g)", i, base[i].dTime);
      if (!std::isfinite(base[i].pitchBend) || !std::isfinite(base[i].note)) return fail(MX_ERR_INVALID, "base marker %d is not finite", i);
    }
    return hand_over(timing_markers(anchors, nanchors, n, sampleRate, p, base, nbase), out, nout);
  });
}

}  // extern "C"
