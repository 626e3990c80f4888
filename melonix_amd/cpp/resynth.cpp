#include "resynth.hpp"

#include "capi-glue.hpp"
#include "save-wav.hpp"

namespace melonix {

Resynth::Resynth(std::span<const float> wav, int sampleRate, int device)
    : nsrc(wav.size()), sampleRate(sampleRate) {
  if (mx_ctx_create(device, &ctx) != MX_OK) {
    ctx = nullptr;
    return;
  }
  if (mx_audio_upload(ctx, wav.data(), (int64_t)wav.size(), &audio) != MX_OK) {
    audio = nullptr;
    return;
  }
  // App::preproc's grain scan (app.cpp:153-235), chain and all, on the device: the grain table comes back
  int32_t *s = nullptr, *l = nullptr;
  float *f = nullptr;
  int64_t n = 0;
  if (mx_grain_table_dev(ctx, audio, &s, &l, &f, &n) == MX_OK) {
    starts = glue::taken<int32_t>(s, n);
    lens = glue::taken<int32_t>(l, n);
    firsts = glue::taken<float>(f, n);
  }
}

Resynth::~Resynth() {
  if (audio) mx_audio_free(ctx, audio);
  if (ctx) mx_ctx_destroy(ctx);
}

bool Resynth::run(const std::vector<Marker> &markers, std::vector<float> *f32, std::vector<int16_t> *i16,
                  double cursor0, int64_t need, double *cursorEnd) const {
  if (!ok()) return false;
  mx_step *steps = nullptr;
  int64_t nsteps = 0, nsamples = 0;
  const mx_marker *mk = reinterpret_cast<const mx_marker *>(markers.data());
  if (mx_schedule_build_table((int64_t)nsrc, sampleRate, starts.data(), lens.data(), firsts.data(), (int64_t)starts.size(), mk,
                              (int)markers.size(), cursor0, need, &steps, &nsteps, &nsamples, cursorEnd) != MX_OK)
    return false;
  if (f32) f32->resize((size_t)nsamples);
  if (i16) i16->resize((size_t)nsamples);
  const int rc = mx_resynth(ctx, audio, steps, nsteps, nsamples, f32 ? f32->data() : nullptr, i16 ? i16->data() : nullptr);
  mx_free(steps);
  return rc == MX_OK;
}

std::vector<float> Resynth::render(const std::vector<Marker> &markers) const {
  std::vector<float> pcm;
  if (!run(markers, &pcm, nullptr)) pcm.clear();
  return pcm;
}

std::vector<int16_t> Resynth::render16(const std::vector<Marker> &markers) const {
  std::vector<int16_t> pcm;
  if (!run(markers, nullptr, &pcm)) pcm.clear();
  return pcm;
}

std::vector<float> Resynth::refill(const std::vector<Marker> &markers, double cursor, std::size_t need,
                                   double *cursorEnd) const {
  std::vector<float> pcm;
  if (!run(markers, &pcm, nullptr, cursor, (int64_t)need, cursorEnd)) pcm.clear();
  return pcm;
}

std::vector<float> Resynth::phaseVocoder(double semitones) const {
  std::vector<float> pcm;
  if (!ok()) return pcm;
  pcm.resize(nsrc);
  if (mx_pv_pitch_shift(ctx, audio, semitones, pcm.data(), nullptr) != MX_OK) pcm.clear();
  return pcm;
}

// mx_psola_render_formant over a track and a curve, as rendered() calls it
static auto psolaCall(mx_ctx *ctx, const mx_audio *audio, int sampleRate, const std::vector<mx_f0> &track, int hop,
                      const std::vector<mx_formant_point> &formant, const mx_psola_params *params) {
  return [=, &track, &formant](const mx_marker *mk, int n, float *f, int16_t *i) {
    return mx_psola_render_formant(ctx, audio, sampleRate, hop, track.data(), (int64_t)track.size(), params, mk, n, formant.data(),
                                   (int)formant.size(), f, i);
  };
}

// A marker-driven render (phase vocoder, PSOLA): the warped length, buffers of that length, and one C call
// (mx_marker *, count, f32 | null, int16 | null) -> status.  False: not ok(), nothing to render, or the call failed.
template <class Call>
bool Resynth::rendered(const std::vector<Marker> &markers, std::vector<float> *f32, std::vector<int16_t> *i16, Call call) const {
  if (!ok()) return false;
  const mx_marker *mk = reinterpret_cast<const mx_marker *>(markers.data());
  const int64_t m = mx_pv_render_length((int64_t)nsrc, sampleRate, mk, (int)markers.size());
  if (m <= 0) return false;
  if (f32) f32->resize((size_t)m);
  if (i16) i16->resize((size_t)m);
  return call(mk, (int)markers.size(), f32 ? f32->data() : nullptr, i16 ? i16->data() : nullptr) == MX_OK;
}

std::vector<float> Resynth::renderPV(const std::vector<Marker> &markers) const {
  std::vector<float> pcm;
  if (!rendered(markers, &pcm, nullptr, [&](auto... a) { return mx_pv_render(ctx, audio, sampleRate, a...); })) pcm.clear();
  return pcm;
}

bool Resynth::exportWavPV(const std::string &fileName, const std::vector<Marker> &markers) const {
  std::vector<int16_t> pcm16;
  if (!rendered(markers, nullptr, &pcm16, [&](auto... a) { return mx_pv_render(ctx, audio, sampleRate, a...); })) return false;
  saveWav(fileName, pcm16, sampleRate);
  return true;
}

std::vector<float> Resynth::renderPSOLA(const std::vector<Marker> &markers, const std::vector<mx_f0> &track, int hop,
                                        const mx_psola_params *params) const {
  return renderPSOLA(markers, track, hop, std::vector<mx_formant_point>(), params);  // (no points: mx_psola_render itself)
}

bool Resynth::exportWavPSOLA(const std::string &fileName, const std::vector<Marker> &markers, const std::vector<mx_f0> &track,
                             int hop, const mx_psola_params *params) const {
  return exportWavPSOLA(fileName, markers, track, hop, std::vector<mx_formant_point>(), params);
}

std::vector<float> Resynth::renderPSOLA(const std::vector<Marker> &markers, const std::vector<mx_f0> &track, int hop,
                                        const std::vector<mx_formant_point> &formant, const mx_psola_params *params) const {
  std::vector<float> pcm;
  if (!rendered(markers, &pcm, nullptr, psolaCall(ctx, audio, sampleRate, track, hop, formant, params))) pcm.clear();
  return pcm;
}

bool Resynth::exportWavPSOLA(const std::string &fileName, const std::vector<Marker> &markers, const std::vector<mx_f0> &track,
                             int hop, const std::vector<mx_formant_point> &formant, const mx_psola_params *params) const {
  std::vector<int16_t> pcm16;
  if (!rendered(markers, nullptr, &pcm16, psolaCall(ctx, audio, sampleRate, track, hop, formant, params))) return false;
  saveWav(fileName, pcm16, sampleRate);
  return true;
}

bool Resynth::exportWav(const std::string &fileName, const std::vector<Marker> &markers) const {
  if (!ok()) return false;
  // schedule on the host, then resynthesis + int16 + saveWav (app.cpp:1209-1214) with the PCM streamed from the device
  // into the file in pieces; same bytes as render16() + saveWav()
  mx_step *steps = nullptr;
  int64_t nsteps = 0, nsamples = 0;
  const mx_marker *mk = reinterpret_cast<const mx_marker *>(markers.data());
  if (mx_schedule_build_table((int64_t)nsrc, sampleRate, starts.data(), lens.data(), firsts.data(), (int64_t)starts.size(), mk,
                              (int)markers.size(), 0., -1, &steps, &nsteps, &nsamples, nullptr) != MX_OK)
    return false;
#ifdef MELONIX_CORRECT_WAV_HEADER
  const int strict = 0;
#else
  const int strict = 1;
#endif
  const int rc = mx_resynth_to_wav(ctx, audio, steps, nsteps, nsamples, fileName.c_str(), sampleRate, strict);
  mx_free(steps);
  return rc == MX_OK;
}

}  // namespace melonix
