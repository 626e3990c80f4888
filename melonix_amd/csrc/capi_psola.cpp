// capi_psola.cpp — the PSOLA renderer (psola_plan.cpp plans on the host, psola_kernels.hip adds the grains up): BUILD-DEFINED, the
// reference has no counterpart.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).
#include "capi_internal.h"
#include "psola_plan.h"

using namespace mx;

namespace {

// What the plan and render entry points hand on; no points: the plain records and the plain kernel; no bend: the markers' alone
struct PsolaCall {
  int64_t n;
  int sampleRate, hop;
  const mx_f0 *track;
  int64_t count;
  const mx_psola_params *params;
  const mx_marker *markers;
  int nmarkers;
  const mx_formant_point *points;
  int npoints;
  const float *bend = nullptr;
};

int psola_build(const PsolaCall &c, const mx_psola_params &p, std::vector<mx_psola_grain> &v, int64_t &m, std::string &err) {
  return build_psola_plan(c.n, c.sampleRate, c.hop, c.track, c.count, p, c.markers, c.nmarkers, v, m, err, c.bend);
}
int psola_build(const PsolaCall &c, const mx_psola_params &p, std::vector<mx_psola_fgrain> &v, int64_t &m, std::string &err) {
  return build_psola_plan(c.n, c.sampleRate, c.hop, c.track, c.count, p, c.markers, c.nmarkers, c.points, c.npoints, v, m, err, c.bend);
}

// the plan of a call's host arguments, or a failed status
template <class Rec>
int psola_plan(const PsolaCall &c, std::vector<Rec> &v, int64_t &m) {
  if (c.nmarkers < 0 || (c.nmarkers > 0 && !c.markers)) return fail(MX_ERR_INVALID, "bad marker list");
  std::string err;
  const int rc = psola_build(c, params_or(c.params, kPsolaDefaults), v, m, err);
  return rc ? fail(rc, "%s", err.c_str()) : MX_OK;
}

// ... handed to the caller for mx_free
template <class Rec>
int psola_plan_out(const PsolaCall &c, Rec **grains, int64_t *ngrains, int64_t *nsamples) {
  if (!grains || !ngrains || !nsamples) return fail(MX_ERR_INVALID, "null output");
  std::vector<Rec> v;
  int64_t m = 0;
  if (const int rc = psola_plan(c, v, m)) return rc;
  if (const int rc = hand_over(v, grains, ngrains)) return rc;
  *nsamples = m;
  return MX_OK;
}

bool no_output(int64_t nsamples, const float *f, const int16_t *i) { return nsamples == 0 || (!f && !i); }

int psola_parse(mx_ctx *ctx, const mx_audio *a, const void *grains, int64_t ngrains, int64_t nsamples) {
  if (const int rc = handles_check(ctx, a)) return rc;
  if (ngrains < 0 || nsamples < 0 || nsamples > INT32_MAX) return fail(MX_ERR_INVALID, "grain or sample count out of range");
  if (ngrains > 0 && !grains) return fail(MX_ERR_INVALID, "null grain records");
  return MX_OK;
}

// queues the overlap-add (no grains: the zero fill) on the context's stream.  Rec: mx_psola_grain or mx_psola_fgrain
template <class Rec>
int psola_launch(mx_ctx *ctx, const mx_audio *a, const Rec *d_grains, int64_t ngrains, int64_t nsamples, float *d_f,
                 int16_t *d_i) {
  if (no_output(nsamples, d_f, d_i)) return MX_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (ngrains == 0) {
    if (d_f) HIP_TRY(hipMemsetAsync(d_f, 0, (size_t)nsamples * sizeof(float), ctx->stream));
    if (d_i) HIP_TRY(hipMemsetAsync(d_i, 0, (size_t)nsamples * sizeof(int16_t), ctx->stream));
    return MX_OK;
  }
  PsolaArgsT<Rec> g{};
  g.audio = a->d_padded;
  g.n = a->n;
  g.grains = d_grains;
  g.ngrains = ngrains;
  g.nsamples = nsamples;
  g.pcm_f32 = d_f;
  g.pcm_i16 = d_i;
  HIP_TRY(launch_psola(g, ctx->stream));
  return MX_OK;
}

// the same from host records: uploaded for the call, released once the stream has drained
template <class Rec>
int psola_launch_host(mx_ctx *ctx, const mx_audio *a, const Rec *grains, int64_t ngrains, int64_t nsamples, float *d_f,
                      int16_t *d_i) {
  HIP_TRY(hipSetDevice(ctx->device));
  DeviceArray<Rec> d;
  if (d.alloc(ctx->stream, (size_t)ngrains) != hipSuccess) return fail(MX_ERR_NOMEM, "device grain records");
  if (ngrains) HIP_TRY(hipMemcpyAsync(d.p, grains, (size_t)ngrains * sizeof(Rec), hipMemcpyHostToDevice, ctx->stream));
  const int rc = psola_launch(ctx, a, d.p, ngrains, nsamples, d_f, d_i);
  const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the upload read the caller's memory)
  if (rc) return rc;
  return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "PSOLA synthesis: %s", hipGetErrorString(e));
}

// ... with the PCM brought to the host
template <class Rec>
int psola_to_host(mx_ctx *ctx, const mx_audio *a, const Rec *grains, int64_t ngrains, int64_t nsamples, float *pcm_f32_out,
                  int16_t *pcm_i16_out) {
  if (no_output(nsamples, pcm_f32_out, pcm_i16_out)) return MX_OK;
  return pcm_to_host(ctx, nsamples, pcm_f32_out, pcm_i16_out, [&](float *d_f, int16_t *d_i) {
    return psola_launch_host(ctx, a, grains, ngrains, nsamples, d_f, d_i);
  });
}

// the synthesis entry points: device records as they are, host records checked first
template <class Rec>
int psola_synth_dev(mx_ctx *ctx, const mx_audio *a, const Rec *d_grains, int64_t ngrains, int64_t nsamples, float *d_f,
                    int16_t *d_i) {
  if (const int rc = psola_parse(ctx, a, d_grains, ngrains, nsamples)) return rc;
  return psola_launch(ctx, a, d_grains, ngrains, nsamples, d_f, d_i);
}

template <class Rec>
int psola_synth(mx_ctx *ctx, const mx_audio *a, const Rec *grains, int64_t ngrains, int64_t nsamples, float *pcm_f32_out,
                int16_t *pcm_i16_out) {
  if (const int rc = psola_parse(ctx, a, grains, ngrains, nsamples)) return rc;
  std::string err;
  if (const int rc = check_psola_grains(grains, ngrains, nsamples, a->n, err)) return fail(rc, "%s", err.c_str());
  return psola_to_host(ctx, a, grains, ngrains, nsamples, pcm_f32_out, pcm_i16_out);
}

// plan and synthesis in one call, the PCM brought to the host or left on the device
template <class Rec>
int psola_render_as(mx_ctx *ctx, const mx_audio *a, const PsolaCall &c, float *pcm_f32, int16_t *pcm_i16, bool to_host) {
  std::vector<Rec> v;
  int64_t m = 0;
  if (const int rc = psola_plan(c, v, m)) return rc;
  return to_host ? psola_to_host(ctx, a, v.data(), (int64_t)v.size(), m, pcm_f32, pcm_i16)
                 : psola_launch_host(ctx, a, v.data(), (int64_t)v.size(), m, pcm_f32, pcm_i16);
}

// ... for the record kind the call asks for (c.n: filled in here, once the handles are known to be there)
int psola_render(mx_ctx *ctx, const mx_audio *a, PsolaCall c, float *pcm_f32, int16_t *pcm_i16, bool to_host) {
  if (const int rc = handles_check(ctx, a)) return rc;
  c.n = a->n;
  return c.npoints == 0 ? psola_render_as<mx_psola_grain>(ctx, a, c, pcm_f32, pcm_i16, to_host)
                        : psola_render_as<mx_psola_fgrain>(ctx, a, c, pcm_f32, pcm_i16, to_host);
}

}  // namespace

extern "C" {

void mx_psola_params_default(mx_psola_params *p) {
  mx_guard_void([&] { params_default(p, kPsolaDefaults); });
}

int mx_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                  const mx_marker *markers, int nmarkers, mx_psola_grain **grains, int64_t *ngrains, int64_t *nsamples) {
  return mx_guard([&] {
    const PsolaCall c{n, sampleRate, hop, track, count, params, markers, nmarkers, nullptr, 0};
    return psola_plan_out(c, grains, ngrains, nsamples);
  });
}

int mx_psola_synth_dev(mx_ctx *ctx, const mx_audio *a, const mx_psola_grain *d_grains, int64_t ngrains, int64_t nsamples,
                       float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&] { return psola_synth_dev(ctx, a, d_grains, ngrains, nsamples, d_pcm_f32, d_pcm_i16); });
}

int mx_psola_synth(mx_ctx *ctx, const mx_audio *a, const mx_psola_grain *grains, int64_t ngrains, int64_t nsamples,
                   float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&] { return psola_synth(ctx, a, grains, ngrains, nsamples, pcm_f32_out, pcm_i16_out); });
}

int mx_psola_render_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                        const mx_psola_params *params, const mx_marker *markers, int nmarkers, float *d_pcm_f32,
                        int16_t *d_pcm_i16) {
  return mx_guard([&] {
    const PsolaCall c{0, sampleRate, hop, track, count, params, markers, nmarkers, nullptr, 0};
    return psola_render(ctx, a, c, d_pcm_f32, d_pcm_i16, false);
  });
}

int mx_psola_render(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                    const mx_psola_params *params, const mx_marker *markers, int nmarkers, float *pcm_f32_out,
                    int16_t *pcm_i16_out) {
  return mx_guard([&] {
    const PsolaCall c{0, sampleRate, hop, track, count, params, markers, nmarkers, nullptr, 0};
    return psola_render(ctx, a, c, pcm_f32_out, pcm_i16_out, true);
  });
}

int mx_psola_plan_formant(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                          const mx_marker *markers, int nmarkers, const mx_formant_point *points, int npoints,
                          mx_psola_fgrain **fgrains, int64_t *ngrains, int64_t *nsamples) {
  return mx_guard([&] {
    const PsolaCall c{n, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints};
    return psola_plan_out(c, fgrains, ngrains, nsamples);
  });
}

int mx_psola_synth_formant_dev(mx_ctx *ctx, const mx_audio *a, const mx_psola_fgrain *d_fgrains, int64_t ngrains,
                               int64_t nsamples, float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&] { return psola_synth_dev(ctx, a, d_fgrains, ngrains, nsamples, d_pcm_f32, d_pcm_i16); });
}

int mx_psola_synth_formant(mx_ctx *ctx, const mx_audio *a, const mx_psola_fgrain *fgrains, int64_t ngrains, int64_t nsamples,
                           float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&] { return psola_synth(ctx, a, fgrains, ngrains, nsamples, pcm_f32_out, pcm_i16_out); });
}

// (no points: these two ARE mx_psola_render_dev / mx_psola_render)
int mx_psola_render_formant_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                                const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                                const mx_formant_point *points, int npoints, float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&] {
    const PsolaCall c{0, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints};
    return psola_render(ctx, a, c, d_pcm_f32, d_pcm_i16, false);
  });
}

int mx_psola_render_formant(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                            const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                            const mx_formant_point *points, int npoints, float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&] {
    const PsolaCall c{0, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints};
    return psola_render(ctx, a, c, pcm_f32_out, pcm_i16_out, true);
  });
}

// ---- the same with a bend curve over the source's frames (include/melonix_amd.h "PSOLA follows a bend curve") ----
int mx_psola_plan_bend(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                       const mx_marker *markers, int nmarkers, const float *bend, mx_psola_grain **grains, int64_t *ngrains,
                       int64_t *nsamples) {
  return mx_guard([&] {
    const PsolaCall c{n, sampleRate, hop, track, count, params, markers, nmarkers, nullptr, 0, bend};
    return psola_plan_out(c, grains, ngrains, nsamples);
  });
}

int mx_psola_plan_formant_bend(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                               const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                               const mx_formant_point *points, int npoints, const float *bend, mx_psola_fgrain **fgrains,
                               int64_t *ngrains, int64_t *nsamples) {
  return mx_guard([&] {
    const PsolaCall c{n, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints, bend};
    return psola_plan_out(c, fgrains, ngrains, nsamples);
  });
}

int mx_psola_render_bend_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                             const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                             const mx_formant_point *points, int npoints, const float *bend, float *d_pcm_f32,
                             int16_t *d_pcm_i16) {
  return mx_guard([&] {
    const PsolaCall c{0, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints, bend};
    return psola_render(ctx, a, c, d_pcm_f32, d_pcm_i16, false);
  });
}

int mx_psola_render_bend(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                         const mx_psola_params *params, const mx_marker *markers, int nmarkers, const mx_formant_point *points,
                         int npoints, const float *bend, float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&] {
    const PsolaCall c{0, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints, bend};
    return psola_render(ctx, a, c, pcm_f32_out, pcm_i16_out, true);
  });
}

}  // extern "C"
