// capi_psola.cpp — the PSOLA renderer (psola_plan.cpp plans on the host, psola_kernels.hip adds the grains up): BUILD-DEFINED, the
// reference has no counterpart.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).
#include "capi_internal.h"
#include "psola_plan.h"

using namespace mx;

namespace {

// the plan of a call's host arguments, or a failed status
int psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
               const mx_marker *markers, int nmarkers, std::vector<mx_psola_grain> &grains, int64_t &nsamples) {
  if (nmarkers < 0 || (nmarkers > 0 && !markers)) return fail(MX_ERR_INVALID, "bad marker list");
  std::string err;
  const int rc = build_psola_plan(n, sampleRate, hop, track, count, params ? *params : kPsolaDefaults, markers, nmarkers, grains,
                                  nsamples, err);
  return rc ? fail(rc, "%s", err.c_str()) : MX_OK;
}

// ... and the formant form's
int psola_fplan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                const mx_marker *markers, int nmarkers, const mx_formant_point *points, int npoints,
                std::vector<mx_psola_fgrain> &fgrains, int64_t &nsamples) {
  if (nmarkers < 0 || (nmarkers > 0 && !markers)) return fail(MX_ERR_INVALID, "bad marker list");
  std::string err;
  const int rc = build_psola_fplan(n, sampleRate, hop, track, count, params ? *params : kPsolaDefaults, markers, nmarkers, points,
                                   npoints, fgrains, nsamples, err);
  return rc ? fail(rc, "%s", err.c_str()) : MX_OK;
}

int psola_parse(mx_ctx *ctx, const mx_audio *a, const void *grains, int64_t ngrains, int64_t nsamples) {
  if (!ctx || !a) return fail(MX_ERR_INVALID, "null context or audio handle");
  if (ngrains < 0 || nsamples < 0 || nsamples > INT32_MAX) return fail(MX_ERR_INVALID, "grain or sample count out of range");
  if (ngrains > 0 && !grains) return fail(MX_ERR_INVALID, "null grain records");
  return MX_OK;
}

// queues the overlap-add (no grains: the zero fill) on the context's stream.  Rec: mx_psola_grain or mx_psola_fgrain
template <class Rec>
int psola_launch(mx_ctx *ctx, const mx_audio *a, const Rec *d_grains, int64_t ngrains, int64_t nsamples, float *d_f,
                 int16_t *d_i) {
  if (nsamples == 0 || (!d_f && !d_i)) return MX_OK;
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

// What the four render entry points hand on; no points: the plain records and the plain kernel
struct PsolaCall {
  mx_ctx *ctx;
  const mx_audio *a;
  int sampleRate, hop;
  const mx_f0 *track;
  int64_t count;
  const mx_psola_params *params;
  const mx_marker *markers;
  int nmarkers;
  const mx_formant_point *points;
  int npoints;
};

int psola_plan(const PsolaCall &c, std::vector<mx_psola_grain> &v, int64_t &m) {
  return psola_plan(c.a->n, c.sampleRate, c.hop, c.track, c.count, c.params, c.markers, c.nmarkers, v, m);
}
int psola_plan(const PsolaCall &c, std::vector<mx_psola_fgrain> &v, int64_t &m) {
  return psola_fplan(c.a->n, c.sampleRate, c.hop, c.track, c.count, c.params, c.markers, c.nmarkers, c.points, c.npoints, v, m);
}

// plan and synthesis in one call, the PCM left on the device ...
template <class Rec>
int psola_render_dev(const PsolaCall &c, float *d_pcm_f32, int16_t *d_pcm_i16) {
  if (!c.ctx || !c.a) return fail(MX_ERR_INVALID, "null context or audio handle");
  std::vector<Rec> v;
  int64_t m = 0;
  if (const int rc = psola_plan(c, v, m)) return rc;
  return psola_launch_host(c.ctx, c.a, v.data(), (int64_t)v.size(), m, d_pcm_f32, d_pcm_i16);
}

// ... or brought to the host
template <class Rec>
int psola_render(const PsolaCall &c, float *pcm_f32_out, int16_t *pcm_i16_out) {
  if (!c.ctx || !c.a) return fail(MX_ERR_INVALID, "null context or audio handle");
  std::vector<Rec> v;
  int64_t m = 0;
  if (const int rc = psola_plan(c, v, m)) return rc;
  if (m == 0 || (!pcm_f32_out && !pcm_i16_out)) return MX_OK;
  return pcm_to_host(c.ctx, m, pcm_f32_out, pcm_i16_out, [&](float *d_f, int16_t *d_i) {
    return psola_launch_host(c.ctx, c.a, v.data(), (int64_t)v.size(), m, d_f, d_i);
  });
}

}  // namespace

extern "C" {

void mx_psola_params_default(mx_psola_params *p) {
  mx_guard_void([&] {
    if (p) *p = kPsolaDefaults;
  });
}

int mx_psola_plan(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                  const mx_marker *markers, int nmarkers, mx_psola_grain **grains, int64_t *ngrains, int64_t *nsamples) {
  return mx_guard([&]() -> int {
    if (!grains || !ngrains || !nsamples) return fail(MX_ERR_INVALID, "null output");
    std::vector<mx_psola_grain> v;
    int64_t m = 0;
    if (const int rc = psola_plan(n, sampleRate, hop, track, count, params, markers, nmarkers, v, m)) return rc;
    HandOver h;
    h.add(grains, v.data(), v.size());
    if (const int rc = h.give()) return rc;
    *ngrains = (int64_t)v.size();
    *nsamples = m;
    return MX_OK;
  });
}

int mx_psola_synth_dev(mx_ctx *ctx, const mx_audio *a, const mx_psola_grain *d_grains, int64_t ngrains, int64_t nsamples,
                       float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    if (const int rc = psola_parse(ctx, a, d_grains, ngrains, nsamples)) return rc;
    return psola_launch(ctx, a, d_grains, ngrains, nsamples, d_pcm_f32, d_pcm_i16);
  });
}

int mx_psola_synth(mx_ctx *ctx, const mx_audio *a, const mx_psola_grain *grains, int64_t ngrains, int64_t nsamples,
                   float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    if (const int rc = psola_parse(ctx, a, grains, ngrains, nsamples)) return rc;
    std::string err;
    if (const int rc = check_psola_grains(grains, ngrains, nsamples, a->n, err)) return fail(rc, "%s", err.c_str());
    if (nsamples == 0 || (!pcm_f32_out && !pcm_i16_out)) return MX_OK;
    return pcm_to_host(ctx, nsamples, pcm_f32_out, pcm_i16_out, [&](float *d_f, int16_t *d_i) {
      return psola_launch_host(ctx, a, grains, ngrains, nsamples, d_f, d_i);
    });
  });
}

int mx_psola_render_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                        const mx_psola_params *params, const mx_marker *markers, int nmarkers, float *d_pcm_f32,
                        int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    const PsolaCall c{ctx, a, sampleRate, hop, track, count, params, markers, nmarkers, nullptr, 0};
    return psola_render_dev<mx_psola_grain>(c, d_pcm_f32, d_pcm_i16);
  });
}

int mx_psola_render(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                    const mx_psola_params *params, const mx_marker *markers, int nmarkers, float *pcm_f32_out,
                    int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    const PsolaCall c{ctx, a, sampleRate, hop, track, count, params, markers, nmarkers, nullptr, 0};
    return psola_render<mx_psola_grain>(c, pcm_f32_out, pcm_i16_out);
  });
}

int mx_psola_plan_formant(int64_t n, int sampleRate, int hop, const mx_f0 *track, int64_t count, const mx_psola_params *params,
                          const mx_marker *markers, int nmarkers, const mx_formant_point *points, int npoints,
                          mx_psola_fgrain **fgrains, int64_t *ngrains, int64_t *nsamples) {
  return mx_guard([&]() -> int {
    if (!fgrains || !ngrains || !nsamples) return fail(MX_ERR_INVALID, "null output");
    std::vector<mx_psola_fgrain> v;
    int64_t m = 0;
    if (const int rc = psola_fplan(n, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints, v, m)) return rc;
    HandOver h;
    h.add(fgrains, v.data(), v.size());
    if (const int rc = h.give()) return rc;
    *ngrains = (int64_t)v.size();
    *nsamples = m;
    return MX_OK;
  });
}

int mx_psola_synth_formant_dev(mx_ctx *ctx, const mx_audio *a, const mx_psola_fgrain *d_fgrains, int64_t ngrains,
                               int64_t nsamples, float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    if (const int rc = psola_parse(ctx, a, d_fgrains, ngrains, nsamples)) return rc;
    return psola_launch(ctx, a, d_fgrains, ngrains, nsamples, d_pcm_f32, d_pcm_i16);
  });
}

int mx_psola_synth_formant(mx_ctx *ctx, const mx_audio *a, const mx_psola_fgrain *fgrains, int64_t ngrains, int64_t nsamples,
                           float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    if (const int rc = psola_parse(ctx, a, fgrains, ngrains, nsamples)) return rc;
    std::string err;
    if (const int rc = check_psola_fgrains(fgrains, ngrains, nsamples, a->n, err)) return fail(rc, "%s", err.c_str());
    if (nsamples == 0 || (!pcm_f32_out && !pcm_i16_out)) return MX_OK;
    return pcm_to_host(ctx, nsamples, pcm_f32_out, pcm_i16_out, [&](float *d_f, int16_t *d_i) {
      return psola_launch_host(ctx, a, fgrains, ngrains, nsamples, d_f, d_i);
    });
  });
}

// (no points: these two ARE mx_psola_render_dev / mx_psola_render)
int mx_psola_render_formant_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                                const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                                const mx_formant_point *points, int npoints, float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    const PsolaCall c{ctx, a, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints};
    return npoints == 0 ? psola_render_dev<mx_psola_grain>(c, d_pcm_f32, d_pcm_i16)
                        : psola_render_dev<mx_psola_fgrain>(c, d_pcm_f32, d_pcm_i16);
  });
}

int mx_psola_render_formant(mx_ctx *ctx, const mx_audio *a, int sampleRate, int hop, const mx_f0 *track, int64_t count,
                            const mx_psola_params *params, const mx_marker *markers, int nmarkers,
                            const mx_formant_point *points, int npoints, float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    const PsolaCall c{ctx, a, sampleRate, hop, track, count, params, markers, nmarkers, points, npoints};
    return npoints == 0 ? psola_render<mx_psola_grain>(c, pcm_f32_out, pcm_i16_out) : psola_render<mx_psola_fgrain>(c, pcm_f32_out, pcm_i16_out);
  });
}

}  // extern "C"
