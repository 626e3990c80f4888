// capi_sibilant.cpp — sibilant features (sibilant_kernels.hip), segments, protected formant curves and balance points
// (sibilant_logic.cpp): BUILD-DEFINED, the reference has none of it.  One unit of the C-ABI implementation behind
// include/melonix_amd.h (see capi_internal.h).  (The source gain that takes the balance points: capi_audio.cpp.)
#include "capi_internal.h"
#include "sibilant_logic.h"

using namespace mx;

namespace {

const mx_sib_feature_params kFeatureDefaults{3500.f};
const mx_sibilant_params kSegmentDefaults{0.6, 0.4, 1e-3, 64, 2, 6};

// What the two feature entry points share: their arguments, checked, and the split bin
struct FeatureCall : TrackCall {
  int ks;
};

int feature_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                  const mx_sib_feature_params *params, const void *out, FeatureCall &q) {
  if (const int rc = track_parse(ctx, a, sampleRate, hop, first_frame, count, out, q)) return rc;
  const mx_sib_feature_params p = params_or(params, kFeatureDefaults);
  const double sr = (double)sampleRate;
  if (!std::isfinite(p.split_hz) || !(p.split_hz > 0.f) || (double)p.split_hz > sr / 2.0)
    return fail(MX_ERR_INVALID, "split %g Hz outside (0, %g]", (double)p.split_hz, sr / 2.0);
  q.ks = (int)std::max(1.0, std::min(std::ceil((double)p.split_hz * 1024.0 / sr), 512.0));
  return MX_OK;
}

int feature_launch(const FeatureCall &q, mx_sib_feat *d_feat) {
  if (q.count == 0) return MX_OK;
  HIP_TRY(hipSetDevice(q.ctx->device));
  SibArgs g{};
  if (const int rc = onset_table(q.ctx, &g.tw)) return rc;
  g.audio = q.a->d_padded;
  g.hop = q.hop;
  g.first_frame = q.first_frame;
  g.count = q.count;
  g.ks = q.ks;
  g.out = d_feat;
  g.run = pinned_run(q.ctx);
  HIP_TRY(launch_sib_features(g, q.ctx->stream));
  return MX_OK;
}

// the host form: the records pass through the context's staging buffer of the pitch records
int feature_host(const FeatureCall &q, mx_sib_feat *feat_out) {
  return staged_track(q.ctx, q.count, kStagePitch, "sibilant features", feat_out, [&](mx_sib_feat *d_feat) { return feature_launch(q, d_feat); });
}

// the parameters in force (p null: the defaults), checked
int segment_params(const mx_sibilant_params *p, mx_sibilant_params &out) {
  out = params_or(p, kSegmentDefaults);
  if (!(out.share_on >= 0.0 && out.share_on <= 1.0) || !(out.share_off >= 0.0 && out.share_off <= out.share_on))
    return fail(MX_ERR_INVALID, "shares on %g / off %g: both in [0, 1], off <= on", out.share_on, out.share_off);
  if (!std::isfinite(out.level_floor) || out.level_floor < 0.0) return fail(MX_ERR_INVALID, "level floor %g must be finite and >= 0", out.level_floor);
  if (out.zc_min < 0 || out.zc_min > 1023) return fail(MX_ERR_INVALID, "zc_min %d outside [0, 1023]", out.zc_min);
  if (out.merge_gap < 0 || out.merge_gap > 4096) return fail(MX_ERR_INVALID, "merge_gap %d outside [0, 4096]", out.merge_gap);
  if (out.min_frames < 1 || out.min_frames > 4096) return fail(MX_ERR_INVALID, "min_frames %d outside [1, 4096]", out.min_frames);
  return MX_OK;
}

// what mx_formant_protect and mx_sibilant_gain_points check of the sibilants, the ramp and the length
int span_args(const mx_sibilant *sibs, int64_t nsib, int32_t ramp, int64_t n) {
  if (nsib < 0 || (nsib > 0 && !sibs)) return fail(MX_ERR_INVALID, "bad sibilant list");
  if (n < 1 || n > INT32_MAX) return fail(MX_ERR_INVALID, "%lld samples outside [1, INT32_MAX]", (long long)n);
  if (ramp < 1 || ramp > (1 << 30)) return fail(MX_ERR_INVALID, "ramp of %d samples outside [1, 2^30]", ramp);
  if (const char *why = sibilant_list_error(sibs, nsib, n)) return fail(MX_ERR_INVALID, "%s", why);
  return MX_OK;
}

}  // namespace

extern "C" {

void mx_sib_feature_params_default(mx_sib_feature_params *p) {
  mx_guard_void([&] { params_default(p, kFeatureDefaults); });
}

int mx_sib_features_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                        const mx_sib_feature_params *params, mx_sib_feat *d_feat) {
  return mx_guard([&]() -> int {
    FeatureCall q;
    if (const int rc = feature_parse(ctx, a, sampleRate, hop, first_frame, count, params, d_feat, q)) return rc;
    return feature_launch(q, d_feat);
  });
}

int mx_sib_features(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                    const mx_sib_feature_params *params, mx_sib_feat *feat_out) {
  return mx_guard([&]() -> int {
    FeatureCall q;
    if (const int rc = feature_parse(ctx, a, sampleRate, hop, first_frame, count, params, feat_out, q)) return rc;
    return feature_host(q, feat_out);
  });
}

void mx_sibilant_params_default(mx_sibilant_params *p) {
  mx_guard_void([&] { params_default(p, kSegmentDefaults); });
}

int mx_sibilants(const mx_sib_feat *feat, int64_t count, int hop, int64_t first_frame, const mx_sibilant_params *params,
                 mx_sibilant **out, int64_t *nout) {
  return mx_guard([&]() -> int {
    mx_sibilant_params p;
    if (const int rc = segment_params(params, p)) return rc;
    if (!out || !nout || (count > 0 && !feat)) return fail(MX_ERR_INVALID, "null argument");
    if (count < 0 || first_frame < 0) return fail(MX_ERR_INVALID, "negative frame range");
    if (hop < 1) return fail(MX_ERR_INVALID, "hop %d", hop);
    if (first_frame > INT32_MAX || count > INT32_MAX || (first_frame + count) * (int64_t)hop > INT32_MAX)
      return fail(MX_ERR_INVALID, "frame centres beyond int32 samples");
    return hand_over(sibilant_segments(feat, count, hop, first_frame, p), out, nout);
  });
}

int mx_sibilants_detect(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_sib_feature_params *feature_params,
                        const mx_sibilant_params *params, mx_sibilant **out, int64_t *nout) {
  return mx_guard([&]() -> int {
    mx_sibilant_params p;
    if (const int rc = segment_params(params, p)) return rc;
    if (!out || !nout) return fail(MX_ERR_INVALID, "null argument");
    int64_t count = 0;  // (the whole file)
    if (const int rc = file_frames(ctx, a, hop, count)) return rc;
    if (count * (int64_t)hop > INT32_MAX) return fail(MX_ERR_INVALID, "frame centres beyond int32 samples");
    return whole_take<FeatureCall, mx_sib_feat>(
        count, [&](mx_sib_feat *feat, FeatureCall &q) { return feature_parse(ctx, a, sampleRate, hop, 0, count, feature_params, feat, q); },
        feature_host, [&](const mx_sib_feat *feat) { return hand_over(sibilant_segments(feat, count, hop, 0, p), out, nout); });
  });
}

int mx_formant_protect(const mx_formant_point *points, int npoints, const mx_sibilant *sibs, int64_t nsib, int32_t ramp_samples,
                       int64_t n, mx_formant_point **out, int64_t *nout) {
  return mx_guard([&]() -> int {
    if (!out || !nout || npoints < 0 || (npoints > 0 && !points)) return fail(MX_ERR_INVALID, "null argument or bad formant curve");
    if (const int rc = span_args(sibs, nsib, ramp_samples, n)) return rc;
    if (const char *why = formant_curve_error(points, npoints)) return fail(MX_ERR_INVALID, "%s", why);
    return hand_over(formant_protect(points, npoints, sibs, nsib, ramp_samples, n), out, nout);
  });
}

int mx_sibilant_gain_points(const mx_sibilant *sibs, int64_t nsib, double db, int32_t ramp_samples, int64_t n, mx_gain_point **out,
                            int64_t *nout) {
  return mx_guard([&]() -> int {
    if (!out || !nout) return fail(MX_ERR_INVALID, "null argument");
    if (const int rc = span_args(sibs, nsib, ramp_samples, n)) return rc;
    if (!(db >= -120.0 && db <= 40.0)) return fail(MX_ERR_INVALID, "balance of %g dB outside [-120, 40]", db);
    return hand_over(sibilant_gain_points(sibs, nsib, db, ramp_samples, n), out, nout);
  });
}

}  // extern "C"
