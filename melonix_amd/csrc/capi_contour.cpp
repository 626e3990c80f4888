// capi_contour.cpp — pitch drift and vibrato inside notes: the cents of a track and their split into smooth contour, vibrato and
// per-span statistics (contour_kernels.hip), the spans, vibrato figures and bend curve of contour_logic.cpp: BUILD-DEFINED, the
// reference has none of it.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).
#include "capi_internal.h"
#include "contour_core.h"
#include "contour_logic.h"

using namespace mx;

namespace {

// what the two cents forms check
int cents_check(const mx_ctx *ctx, const void *track, int64_t count, int sampleRate, float threshold, float rms_floor,
                const void *out) {
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  if (const int rc = frames_i32(count)) return rc;
  if (const int rc = rate_check(sampleRate)) return rc;
  if (!std::isfinite(threshold) || !std::isfinite(rms_floor)) return fail(MX_ERR_INVALID, "threshold / rms_floor is not finite");
  if (count > 0 && (!track || !out)) return fail(MX_ERR_INVALID, "null argument");
  return MX_OK;
}

// what the two split forms check alike: everything but the spans themselves
int split_check(const mx_ctx *ctx, const void *cents, int64_t count, const void *spans, int64_t nspans, const mx_contour_params *p) {
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  if (const int rc = frames_i32(count)) return rc;
  if (nspans < 0 || nspans > count) return fail(MX_ERR_INVALID, "%lld spans over %lld frames", (long long)nspans, (long long)count);
  if (!p) return fail(MX_ERR_INVALID, "null parameters");
  if (!contour::params_ok(*p))
    return fail(MX_ERR_INVALID, "contour parameters: half_width %d outside [0, 64] or lags [%d, %d] outside 1 <= min <= max <= 256",
                p->half_width, p->lag_min, p->lag_max);
  if ((count > 0 && !cents) || (nspans > 0 && !spans)) return fail(MX_ERR_INVALID, "null argument");
  return MX_OK;
}

// queues stage B on the context's stream; its work memory is the context's contour set.  d_rec null: the records go to work
// memory.  Nothing wanted: nothing queued.
int split_launch(mx_ctx *ctx, const int32_t *d_cents, int64_t count, const mx_contour_span *d_spans, int64_t nspans,
                 const mx_contour_params &p, mx_contour_rec *d_rec, mx_contour_stat *d_stat) {
  if (count == 0 || (!d_rec && (!d_stat || nspans == 0))) return MX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Hold work(ctx, ctx->contour);
  const char *what = "contour work memory";
  void *d_part = nullptr;
  if (const int rc = d_stat && nspans > 0 ? work.get(kContourPart, contour_part_bytes(count, nspans, p), &d_part, what) : MX_OK) return rc;
  if (const int rc = d_rec ? MX_OK : work.get(kContourRec, (size_t)count, &d_rec, what)) return rc;
  HIP_TRY(launch_contour_split(d_cents, count, d_spans, nspans, p, d_rec, d_stat, d_part, ctx->stream));
  return MX_OK;
}

// Stage B of a staged call (inside staged_records' run): the host spans up, the statistics back (job_pass; stat null: the
// records alone).  No spans: the smoothing alone.
int split_staged(mx_ctx *ctx, const int32_t *d_cents, int64_t count, const mx_contour_span *spans, int64_t nspans,
                 const mx_contour_params &p, mx_contour_rec *d_rec, mx_contour_stat *stat) {
  if (nspans == 0) return split_launch(ctx, d_cents, count, nullptr, 0, p, d_rec, nullptr);
  return job_pass(ctx, "contour spans", spans, nspans, 1, stat, [&](const mx_contour_span *d_spans, mx_contour_stat *d_stat) {
    return split_launch(ctx, d_cents, count, d_spans, nspans, p, d_rec, d_stat);
  });
}

}  // namespace

extern "C" {

int mx_contour_params_default(int sampleRate, int hop, mx_contour_params *p) {
  return mx_guard([&]() -> int {
    if (!p) return fail(MX_ERR_INVALID, "null argument");
    if (const int rc = rate_check(sampleRate)) return rc;
    if (const int rc = hop_check(hop)) return rc;
    *p = contour_params_default(sampleRate, hop);
    return MX_OK;
  });
}

int mx_contour_cents_dev(mx_ctx *ctx, const mx_f0 *d_track, int64_t count, int sampleRate, float threshold, float rms_floor,
                         int32_t *d_cents) {
  return mx_guard([&]() -> int {
    if (const int rc = cents_check(ctx, d_track, count, sampleRate, threshold, rms_floor, d_cents)) return rc;
    if (count == 0) return MX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_contour_cents(d_track, count, sampleRate, threshold, rms_floor, d_cents, ctx->stream));
    return MX_OK;
  });
}

int mx_contour_cents(mx_ctx *ctx, const mx_f0 *track, int64_t count, int sampleRate, float threshold, float rms_floor,
                     int32_t *cents) {
  return mx_guard([&]() -> int {
    if (const int rc = cents_check(ctx, track, count, sampleRate, threshold, rms_floor, cents)) return rc;
    const StagedSlot slots[] = {{kStagePitch, sizeof(mx_f0), track, nullptr}, {kStageRanges, sizeof(int32_t), nullptr, cents}};
    return staged_records(ctx, count, slots, "contour cents", [&](void *const *d) -> int {
      HIP_TRY(launch_contour_cents(static_cast<const mx_f0 *>(d[0]), count, sampleRate, threshold, rms_floor,
                                   static_cast<int32_t *>(d[1]), ctx->stream));
      return MX_OK;
    });
  });
}

int mx_contour_split_dev(mx_ctx *ctx, const int32_t *d_cents, int64_t count, const mx_contour_span *d_spans, int64_t nspans,
                         const mx_contour_params *p, mx_contour_rec *d_rec, mx_contour_stat *d_stat) {
  return mx_guard([&]() -> int {
    if (const int rc = split_check(ctx, d_cents, count, d_spans, nspans, p)) return rc;
    return split_launch(ctx, d_cents, count, d_spans, nspans, *p, d_rec, d_stat);
  });
}

int mx_contour_split(mx_ctx *ctx, const int32_t *cents, int64_t count, const mx_contour_span *spans, int64_t nspans,
                     const mx_contour_params *p, mx_contour_rec *rec, mx_contour_stat *stat) {
  return mx_guard([&]() -> int {
    if (const int rc = split_check(ctx, cents, count, spans, nspans, p)) return rc;
    if (const char *why = contour_spans_error(spans, nspans, count, cents)) return fail(MX_ERR_INVALID, "spans: %s", why);
    const StagedSlot slots[] = {{kStageRanges, sizeof(int32_t), cents, nullptr}, {kStageMags, sizeof(mx_contour_rec), nullptr, rec}};
    return staged_records(ctx, count, slots, "contour split", [&](void *const *d) {
      return split_staged(ctx, static_cast<const int32_t *>(d[0]), count, spans, nspans, *p, static_cast<mx_contour_rec *>(d[1]), stat);
    });
  });
}

int mx_contour_spans(const mx_note *notes, int64_t nnotes, int64_t first_frame, mx_contour_span *spans) {
  return mx_guard([&]() -> int {
    if (nnotes < 0 || (nnotes > 0 && (!notes || !spans))) return fail(MX_ERR_INVALID, "null argument or negative count");
    contour_spans(notes, nnotes, first_frame, spans);
    return MX_OK;
  });
}

int mx_contour_vibrato(const mx_contour_stat *stat, int32_t frames, int sampleRate, int hop, mx_vibrato *out) {
  return mx_guard([&]() -> int {
    if (!stat || !out) return fail(MX_ERR_INVALID, "null argument");
    if (const int rc = rate_check(sampleRate)) return rc;
    if (const int rc = hop_check(hop)) return rc;
    if (frames < 1 || stat->lag < 0 || frames <= stat->lag)
      return fail(MX_ERR_INVALID, "a span of %d frames with lag %d", frames, stat->lag);
    *out = contour_vibrato(*stat, frames, sampleRate, hop);
    return MX_OK;
  });
}

void mx_bend_params_default(mx_bend_params *p) {
  mx_guard_void([&] { params_default(p, kBendDefaults); });
}

int mx_contour_bend(const mx_contour_rec *rec, int64_t count, const mx_note *notes, const mx_contour_span *spans, int64_t nnotes,
                    const double *shift, const mx_bend_params *p, float *bend_out) {
  return mx_guard([&]() -> int {
    if (count < 0 || nnotes < 0 || nnotes > count) return fail(MX_ERR_INVALID, "%lld notes over %lld frames", (long long)nnotes, (long long)count);
    if ((count > 0 && (!rec || !bend_out)) || (nnotes > 0 && (!notes || !spans))) return fail(MX_ERR_INVALID, "null argument");
    const mx_bend_params q = params_or(p, kBendDefaults);
    if (const char *why = bend_params_error(q)) return fail(MX_ERR_INVALID, "bend parameters: %s", why);
    if (const char *why = contour_spans_error(spans, nnotes, count, nullptr)) return fail(MX_ERR_INVALID, "spans: %s", why);
    if (const int rc = notes_check(notes, nnotes, /*finite=*/true, /*ordered=*/false)) return rc;
    if (shift && !std::all_of(shift, shift + nnotes, [](double v) { return std::isfinite(v); }))
      return fail(MX_ERR_INVALID, "a note's shift is not finite");
    contour_bend(rec, count, notes, spans, nnotes, shift, q, bend_out);
    return MX_OK;
  });
}

int mx_pitch_contour(mx_ctx *ctx, const mx_f0 *track, int64_t count, int sampleRate, int hop, int64_t first_frame,
                     const mx_note *notes, int64_t nnotes, float threshold, float rms_floor, const mx_contour_params *params,
                     mx_contour_rec *rec_out, mx_contour_stat *stat_out) {
  return mx_guard([&]() -> int {
    if (const int rc = cents_check(ctx, track, count, sampleRate, threshold, rms_floor, track)) return rc;
    if (const int rc = hop_check(hop)) return rc;
    if (nnotes < 0 || nnotes > count || (nnotes > 0 && !notes)) return fail(MX_ERR_INVALID, "%lld notes over %lld frames", (long long)nnotes, (long long)count);
    const mx_contour_params p = params_or(params, contour_params_default(sampleRate, hop));
    std::vector<mx_contour_span> spans((size_t)nnotes);
    contour_spans(notes, nnotes, first_frame, spans.data());
    if (const int rc = split_check(ctx, track, count, spans.data(), nnotes, &p)) return rc;
    if (const char *why = contour_spans_error(spans.data(), nnotes, count, nullptr)) return fail(MX_ERR_INVALID, "notes: %s", why);
    // an unvoiced frame inside a note is what stage A would turn into MX_CONTOUR_NONE: refused here, before any launch
    for (const mx_contour_span &s : spans)
      for (int64_t f = s.first; f < (int64_t)s.first + s.frames; ++f)
        if (contour::cents_of(track[f], sampleRate, threshold, rms_floor) == MX_CONTOUR_NONE)
          return fail(MX_ERR_INVALID, "frame %lld inside a note is unvoiced", (long long)f);
    const StagedSlot slots[] = {{kStagePitch, sizeof(mx_f0), track, nullptr},
                                {kStageRanges, sizeof(int32_t), nullptr, nullptr},
                                {kStageMags, sizeof(mx_contour_rec), nullptr, rec_out}};
    return staged_records(ctx, count, slots, "pitch contour", [&](void *const *d) -> int {
      int32_t *d_cents = static_cast<int32_t *>(d[1]);
      HIP_TRY(launch_contour_cents(static_cast<const mx_f0 *>(d[0]), count, sampleRate, threshold, rms_floor, d_cents, ctx->stream));
      return split_staged(ctx, d_cents, count, spans.data(), nnotes, p, static_cast<mx_contour_rec *>(d[2]), stat_out);
    });
  });
}

}  // extern "C"
