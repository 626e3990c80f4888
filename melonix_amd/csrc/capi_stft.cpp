// capi_stft.cpp — STFT + pitch entry points: bulk hop mode, ranges mode, host-staged and texel variants.
// One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h).  There is no CPU compute path:
// every transform entry point needs a live gfx950 device and fails with MX_ERR_DEVICE otherwise.
#include "capi_internal.h"

using namespace mx;

extern "C" {

int mx_stft_run_length(int N, int hop, int64_t count) {
  return mx_guard([&]() -> int {
    if ((N != 4096 && N != 16384 && N != 32768) || hop <= 0 || count < 0) return fail(MX_ERR_INVALID, "bad argument");
    return default_frames_per_block(N, (hop & 1) ? kBulkAny : kBulkAligned, hop, count);
  });
}

// ---- STFT ---------------------------------------------------------------------
void mx_pitch_band(int N, int sampleRate, int *kmin, int *kmax) {
  mx_guard_void([&] {
    // notes 24..84 of the default view (app.hpp:45-46): f = 55*2^((note-24)/12), bin = f*N/sr (app.cpp:499-516)
    const double lo = 55.0 * N / sampleRate, hi = 1760.0 * N / sampleRate;
    int a = (int)lo;
    if ((double)a < lo) ++a;
    if (kmin) *kmin = a;
    if (kmax) *kmax = (int)hi;
  });
}

double mx_bin_note(int bin, int N, int sampleRate) {
  return mx_guard_or<double>(std::nan(""), [&]() -> double {
    if (bin <= 0 || N <= 0 || sampleRate <= 0) return -HUGE_VAL;
    return 24. + 12. * std::log2((double)bin * sampleRate / N / 55.);
  });
}
double mx_note_bin(double note, int N, int sampleRate) {
  return mx_guard_or<double>(std::nan(""), [&]() -> double {
    if (N <= 0 || sampleRate <= 0) return 0.;
    return 55. * std::pow(2., (note - 24.) / 12.) * N / sampleRate;  // app.cpp:498
  });
}

int64_t mx_frame_count(int64_t n, int hop) {
  return mx_guard([&]() -> int64_t {
    return hop > 0 && n >= 0 ? (n + hop - 1) / hop : -1;
  });
}

// hop mode's argument checks, check_common's among them: once per call, host-staged or not
static int stft_hop_check(mx_ctx *ctx, const mx_audio *a, int N, int hop, int64_t first_frame, int64_t count, int &kmin,
                          int &kmax) {
  int rc = check_common(ctx, a, N, count, kmin, kmax);
  if (rc) return rc;
  if (hop <= 0 || hop > MX_AUDIO_PAD) return fail(MX_ERR_INVALID, "hop %d out of range [1,%d]", hop, MX_AUDIO_PAD);
  if (first_frame < 0 || (count > 0 && (first_frame + count - 1) * (int64_t)hop >= a->n))
    return fail(MX_ERR_INVALID, "frames [%lld,%lld) exceed ceil(n/hop)", (long long)first_frame,
                (long long)(first_frame + count));
  return MX_OK;
}
// hop mode's kernel variant
static int bulk_mode(int hop) { return (hop % 2 == 0) ? kBulkAligned : kBulkAny; }

int mx_stft_hop_dev(mx_ctx *ctx, const mx_audio *a, int N, int hop, int64_t first_frame, int64_t count,
                    int kmin, int kmax, float *d_mags, mx_pitch *d_pitch) {
  return mx_guard([&]() -> int {
    int rc = stft_hop_check(ctx, a, N, hop, first_frame, count, kmin, kmax);
    if (rc) return rc;
    return stft_launch(ctx, a, N, bulk_mode(hop), hop, first_frame, nullptr, count, kmin, kmax, d_mags, d_pitch, nullptr, 0.f);
  });
}

int mx_stft_ranges_dev(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *d_ranges, int64_t count, int kmin,
                       int kmax, float *d_mags, mx_pitch *d_pitch) {
  return mx_guard([&]() -> int {
    int rc = check_common(ctx, a, N, count, kmin, kmax);
    if (rc) return rc;
    if (count > 0 && !d_ranges) return fail(MX_ERR_INVALID, "ranges is null");
    return stft_launch(ctx, a, N, kRanges, 0, 0, d_ranges, count, kmin, kmax, d_mags, d_pitch, nullptr, 0.f);
  });
}

int mx_stft_hop(mx_ctx *ctx, const mx_audio *a, int N, int hop, int64_t first_frame, int64_t count, int kmin,
                int kmax, float *mags_out, mx_pitch *pitch_out) {
  return mx_guard([&]() -> int {
    int rc = stft_hop_check(ctx, a, N, hop, first_frame, count, kmin, kmax);
    if (rc || count == 0) return rc;
    // one run length for the whole call, whatever its staging chunks are (chunks are multiples of 32 frames): the rows
    // are those of a single launch of `count` frames
    const int mode = bulk_mode(hop), run = default_frames_per_block(N, mode, hop, count);
    const StagedBatch b{N, count, nullptr, mags_out, pitch_out};
    return staged_batch(ctx, b, [&](int64_t done, int64_t c, const int32_t *, float *d_mags, mx_pitch *d_pitch, uint8_t *) {
      return stft_launch(ctx, a, N, mode, hop, first_frame + done, nullptr, c, kmin, kmax, d_mags, d_pitch, nullptr, 0.f, run);
    });
  });
}

int mx_stft_ranges(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count, int kmin, int kmax,
                   float *mags_out, mx_pitch *pitch_out) {
  return mx_guard([&]() -> int {
    if (count > 0 && !ranges) return fail(MX_ERR_INVALID, "ranges is null");
    int rc = check_common(ctx, a, N, count, kmin, kmax);
    if (rc || count == 0) return rc;
    const StagedBatch b{N, count, ranges, mags_out, pitch_out};
    return staged_batch(ctx, b, [&](int64_t, int64_t c, const int32_t *d_ranges, float *d_mags, mx_pitch *d_pitch, uint8_t *) {
      return mx_stft_ranges_dev(ctx, a, N, d_ranges, c, kmin, kmax, d_mags, d_pitch);
    });
  });
}

int mx_stft_ranges_rgb_dev(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *d_ranges, int64_t count, float k,
                           float *d_mags, uint8_t *d_rgb) {
  return mx_guard([&]() -> int {
    int kmin = -1, kmax = -1;
    int rc = check_common(ctx, a, N, count, kmin, kmax);
    if (rc) return rc;
    if (count > 0 && (!d_ranges || !d_rgb)) return fail(MX_ERR_INVALID, "ranges / rgb is null");
    if (count == 0) return MX_OK;
    // one launch: the STFT kernel's epilogue writes the texels (and, if asked, the magnitudes as well)
    return stft_launch(ctx, a, N, kRanges, 0, 0, d_ranges, count, kmin, kmax, d_mags, nullptr, d_rgb, k);
  });
}

int mx_stft_ranges_rgb_mags(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count, float k,
                            float *mags_out, uint8_t *rgb_out) {
  return mx_guard([&]() -> int {
    int kmin = -1, kmax = -1;
    int rc = check_common(ctx, a, N, count, kmin, kmax);
    if (rc || count == 0) return rc;
    if (!ranges || !rgb_out) return fail(MX_ERR_INVALID, "ranges / rgb_out is null");
    const StagedBatch b{N, count, ranges, mags_out, nullptr, rgb_out};
    return staged_batch(ctx, b, [&](int64_t, int64_t c, const int32_t *d_ranges, float *d_mags, mx_pitch *, uint8_t *d_rgb) {
      return mx_stft_ranges_rgb_dev(ctx, a, N, d_ranges, c, k, d_mags, d_rgb);
    });
  });
}

int mx_stft_ranges_rgb(mx_ctx *ctx, const mx_audio *a, int N, const int32_t *ranges, int64_t count, float k,
                       uint8_t *rgb_out) {
  return mx_guard([&]() -> int {
    return mx_stft_ranges_rgb_mags(ctx, a, N, ranges, count, k, nullptr, rgb_out);
  });
}

}  // extern "C"
