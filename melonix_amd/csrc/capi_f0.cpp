// capi_f0.cpp — the YIN f0 tracker and its candidate ladder (f0_kernels.hip), the Viterbi decode over the ladder
// (f0_decode.hip), notes and correction markers (f0_notes.cpp): BUILD-DEFINED, the reference has no detector.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).
#include "capi_internal.h"
#include "f0_notes.h"

using namespace mx;

namespace {

constexpr int kF0W = 2048;

// the search range of (sr, fmin, fmax), or a failed status
int f0_range(int sampleRate, float fmin, float fmax, int &tmin, int &tmax) {
  if (const int rc = rate_check(sampleRate)) return rc;
  if (!(fmin > 0.f) || !(fmax > 0.f) || !std::isfinite(fmin) || !std::isfinite(fmax))
    return fail(MX_ERR_INVALID, "f0 band [%g, %g] Hz: both ends must be positive and finite", (double)fmin, (double)fmax);
  const double lo = std::floor((double)sampleRate / (double)fmax), hi = std::ceil((double)sampleRate / (double)fmin);
  tmin = (int)std::max(2.0, std::min(lo, 1e9));
  tmax = (int)std::min((double)(kF0W - 1), hi);
  if (tmin > tmax)
    return fail(MX_ERR_INVALID, "empty lag range [%d, %d] for %g..%g Hz at %d Hz", tmin, tmax, (double)fmin, (double)fmax,
                sampleRate);
  return MX_OK;
}

// What the tracker-side entry points share: their arguments, checked, with the search range they give
struct F0Call : TrackCall {
  int tmin, tmax;
  float threshold;
};

// the frame span (frame_span: `out`) and what is the tracker's own: the threshold and the lag range, which checks the sample
// rate — behind the threshold, so not track_parse's order
int f0_parse(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count, float fmin,
             float fmax, float threshold, const void *out, F0Call &q) {
  if (const int rc = frame_span(ctx, a, hop, first_frame, count, out)) return rc;
  if (!std::isfinite(threshold)) return fail(MX_ERR_INVALID, "threshold is not finite");
  q = F0Call{{ctx, a, sampleRate, hop, first_frame, count}, 0, 0, threshold};
  return f0_range(sampleRate, fmin, fmax, q.tmin, q.tmax);
}

// d_cands set: the ladder instantiation (d_out may then be null)
int f0_launch(const F0Call &q, mx_f0 *d_out, mx_f0_cand *d_cands) {
  if (q.count == 0) return MX_OK;
  HIP_TRY(hipSetDevice(q.ctx->device));
  NTables t;
  if (const int rc = get_tables(q.ctx, 4096, t)) return rc;
  F0Args g{};
  g.audio = q.a->d_padded;
  g.hop = q.hop;
  g.first_frame = q.first_frame;
  g.count = q.count;
  g.tau_min = q.tmin;
  g.tau_max = q.tmax;
  g.threshold = q.threshold;
  g.tw2 = t.tw2;
  g.tw3 = t.tw3;
  g.ubase = t.ubase;
  g.out = d_out;
  g.cands = d_cands;
  g.sample_rate = q.sampleRate;
  HIP_TRY(launch_f0(g, q.ctx->stream));
  return MX_OK;
}

const mx_f0_decode_params kDecodeDefaults{0.3f, 0.1f, 0.5f, 1200};
const mx_note_params kNoteDefaults{0.15f, 1e-3f, 0.5, 0.75, 8};

// the parameters in force (p null: the defaults), checked
int decode_params(const mx_f0_decode_params *p, mx_f0_decode_params &out) {
  out = params_or(p, kDecodeDefaults);
  for (const float c : {out.unvoiced_cost, out.jump_cost, out.switch_cost})
    if (!std::isfinite(c) || c < 0.f || c > 16.f) return fail(MX_ERR_INVALID, "decode cost %g outside [0, 16]", (double)c);
  if (out.max_jump_cents < 0 || out.max_jump_cents > 12000)
    return fail(MX_ERR_INVALID, "max_jump_cents %d outside [0, 12000]", out.max_jump_cents);
  return MX_OK;
}

// what the two decode forms check; -> the parameters in force
int decode_parse(mx_ctx *ctx, const void *track, const void *cands, int64_t count, const mx_f0_decode_params *p, const void *out,
                 mx_f0_decode_params &dp) {
  if (const int rc = decode_params(p, dp)) return rc;
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  if (count < 0) return fail(MX_ERR_INVALID, "negative frame count");
  if (count > 0 && (!track || !cands || !out)) return fail(MX_ERR_INVALID, "null argument");
  return MX_OK;
}

int64_t q16(float x) { return (int64_t)std::rint((double)x * 65536.0); }

// queues the decode of `count` frames on the context's stream; its work buffers are the context's f0dec set
int decode_launch(mx_ctx *ctx, const mx_f0 *d_track, const mx_f0_cand *d_cands, int64_t count, const mx_f0_decode_params &p,
                  mx_f0 *d_out, uint8_t *d_state) {
  if (count == 0) return MX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Hold work(ctx, ctx->f0dec);
  F0DecodeArgs g{};
  g.track = d_track;
  g.cands = d_cands;
  g.count = count;
  g.q_unvoiced = q16(p.unvoiced_cost);
  g.q_jump = q16(p.jump_cost);
  g.q_switch = q16(p.switch_cost);
  g.max_jump_cents = p.max_jump_cents;
  g.chunk = ctx->f0_chunk > 0 ? ctx->f0_chunk : f0_decode_default_chunk(count);
  const F0DecodeScratch need = f0_decode_scratch(count, g.chunk);
  void *bp = nullptr, *prod = nullptr, *map = nullptr;  // (f0_decode_scratch counts bytes)
  if (const int rc = work.get(kF0DecBp, need.bp, &bp, "f0 decode work buffers")) return rc;
  if (const int rc = work.get(kF0DecProd, need.prod, &prod, "f0 decode work buffers")) return rc;
  if (const int rc = work.get(kF0DecMap, need.map, &map, "f0 decode work buffers")) return rc;
  g.bp = static_cast<uint16_t *>(bp);
  g.prod = static_cast<int64_t *>(prod);
  g.map = static_cast<uint16_t *>(map);
  g.out = d_out;
  g.state = d_state;
  HIP_TRY(launch_f0_decode(g, ctx->stream));
  return MX_OK;
}

// The host-pointer forms with candidates (staged_records; the plain track is a staged_track): the track — decoded in place —
// passes through the staging buffer of the pitch records, the candidates through the magnitude rows', the states through the texels'.
// `in`: upload the caller's track and candidates; `run(d_track, d_cands, d_state)` queues the device form; the outputs that
// are set come back.
template <class F>
int f0_staged(mx_ctx *ctx, int64_t count, const mx_f0 *track_in, const mx_f0_cand *cands_in, mx_f0 *track_out,
              mx_f0_cand *cands_out, uint8_t *state_out, F &&run) {
  const StagedSlot slots[] = {{kStagePitch, sizeof(mx_f0), track_in, track_out},
                              {kStageMags, MX_F0_CANDS * sizeof(mx_f0_cand), cands_in, cands_out},
                              {kStageTexels, state_out ? 1u : 0u, nullptr, state_out}};
  return staged_records(ctx, count, slots, "f0", [&](void *const *d) {
    return run(static_cast<mx_f0 *>(d[0]), static_cast<mx_f0_cand *>(d[1]), static_cast<uint8_t *>(d[2]));
  });
}

}  // namespace

extern "C" {

int mx_f0_track_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                    float fmin, float fmax, float threshold, mx_f0 *d_out) {
  return mx_guard([&]() -> int {
    F0Call q;
    if (const int rc = f0_parse(ctx, a, sampleRate, hop, first_frame, count, fmin, fmax, threshold, d_out, q)) return rc;
    return f0_launch(q, d_out, nullptr);
  });
}

int mx_f0_track(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count, float fmin,
                float fmax, float threshold, mx_f0 *out) {
  return mx_guard([&]() -> int {
    F0Call q;
    if (const int rc = f0_parse(ctx, a, sampleRate, hop, first_frame, count, fmin, fmax, threshold, out, q)) return rc;
    return staged_track(q.ctx, q.count, kStagePitch, "f0", out, [&](mx_f0 *d_track) { return f0_launch(q, d_track, nullptr); });
  });
}

int mx_f0_candidates_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                         float fmin, float fmax, float threshold, mx_f0 *d_track, mx_f0_cand *d_cands) {
  return mx_guard([&]() -> int {
    F0Call q;
    if (const int rc = f0_parse(ctx, a, sampleRate, hop, first_frame, count, fmin, fmax, threshold, d_cands, q)) return rc;
    return f0_launch(q, d_track, d_cands);
  });
}

int mx_f0_candidates(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                     float fmin, float fmax, float threshold, mx_f0 *track, mx_f0_cand *cands) {
  return mx_guard([&]() -> int {
    F0Call q;
    if (const int rc = f0_parse(ctx, a, sampleRate, hop, first_frame, count, fmin, fmax, threshold, cands, q)) return rc;
    return f0_staged(ctx, count, nullptr, nullptr, track, cands, nullptr,
                     [&](mx_f0 *d_track, mx_f0_cand *d_cands, uint8_t *) { return f0_launch(q, d_track, d_cands); });
  });
}

void mx_f0_decode_params_default(mx_f0_decode_params *p) {
  mx_guard_void([&] { params_default(p, kDecodeDefaults); });
}

int mx_f0_decode_dev(mx_ctx *ctx, const mx_f0 *d_track, const mx_f0_cand *d_cands, int64_t count,
                     const mx_f0_decode_params *p, mx_f0 *d_out, uint8_t *d_state) {
  return mx_guard([&]() -> int {
    mx_f0_decode_params dp;
    if (const int rc = decode_parse(ctx, d_track, d_cands, count, p, d_out, dp)) return rc;
    return decode_launch(ctx, d_track, d_cands, count, dp, d_out, d_state);
  });
}

int mx_f0_decode(mx_ctx *ctx, const mx_f0 *track, const mx_f0_cand *cands, int64_t count, const mx_f0_decode_params *p,
                 mx_f0 *out, uint8_t *state) {
  return mx_guard([&]() -> int {
    mx_f0_decode_params dp;
    if (const int rc = decode_parse(ctx, track, cands, count, p, out, dp)) return rc;
    return f0_staged(ctx, count, track, cands, out, nullptr, state, [&](mx_f0 *d_track, mx_f0_cand *d_cands, uint8_t *d_state) {
      return decode_launch(ctx, d_track, d_cands, count, dp, d_track, d_state);
    });
  });
}

int mx_f0_track_decoded(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, int64_t first_frame, int64_t count,
                        float fmin, float fmax, float threshold, const mx_f0_decode_params *p, mx_f0 *out) {
  return mx_guard([&]() -> int {
    mx_f0_decode_params dp;
    if (const int rc = decode_params(p, dp)) return rc;
    F0Call q;
    if (const int rc = f0_parse(ctx, a, sampleRate, hop, first_frame, count, fmin, fmax, threshold, out, q)) return rc;
    return f0_staged(ctx, count, nullptr, nullptr, out, nullptr, nullptr, [&](mx_f0 *d_track, mx_f0_cand *d_cands, uint8_t *) {
      if (const int rc = f0_launch(q, d_track, d_cands)) return rc;
      return decode_launch(ctx, d_track, d_cands, count, dp, d_track, nullptr);
    });
  });
}

int mx_f0_decode_set_chunk(mx_ctx *ctx, int64_t frames) {
  return mx_guard([&]() -> int {
    if (!ctx || frames < 0) return fail(MX_ERR_INVALID, "bad argument");
    Hold work(ctx, ctx->f0dec);
    ctx->f0_chunk = frames;
    return MX_OK;
  });
}

void mx_note_params_default(mx_note_params *p) {
  mx_guard_void([&] { params_default(p, kNoteDefaults); });
}

int mx_detect_notes(const mx_f0 *track, int64_t count, int sampleRate, int hop, int64_t first_frame,
                    const mx_note_params *params, mx_note **notes, int64_t *nnotes) {
  return mx_guard([&]() -> int {
    if (!params || !notes || !nnotes || (count > 0 && !track)) return fail(MX_ERR_INVALID, "null argument");
    if (count < 0 || first_frame < 0) return fail(MX_ERR_INVALID, "negative frame range");
    if (sampleRate <= 0 || hop < 1) return fail(MX_ERR_INVALID, "sample rate %d / hop %d", sampleRate, hop);
    if ((first_frame + count) * (int64_t)hop > INT32_MAX) return fail(MX_ERR_INVALID, "frame centres beyond int32 samples");
    const mx_note_params &p = *params;
    if (p.min_frames < 2) return fail(MX_ERR_INVALID, "min_frames %d < 2", p.min_frames);
    if (!std::isfinite(p.threshold) || !std::isfinite(p.rms_floor) || !(p.max_jump >= 0.0) || !(p.max_dev >= 0.0))
      return fail(MX_ERR_INVALID, "note parameters must be finite, the deviations >= 0");
    return hand_over(detect_notes(track, count, sampleRate, hop, first_frame, p), notes, nnotes, /*null_if_empty=*/true);
  });
}

int mx_correction_markers(const mx_note *notes, int64_t count, double strength, int scale_mask, mx_marker *out) {
  return mx_guard([&]() -> int {
    if (count < 0 || (count > 0 && (!notes || !out))) return fail(MX_ERR_INVALID, "null argument");
    if (!(strength >= 0.0 && strength <= 1.0)) return fail(MX_ERR_INVALID, "strength %g outside [0, 1]", strength);
    if (scale_mask < 0 || scale_mask > 0xFFF) return fail(MX_ERR_INVALID, "scale mask 0x%x beyond the twelve classes", scale_mask);
    if (const int rc = notes_check(notes, count, /*finite=*/true, /*ordered=*/true)) return rc;
    correction_markers(notes, count, strength, scale_mask, out);
    return MX_OK;
  });
}

}  // extern "C"
