// denoise_emu.cpp — the noise-reduction kernels' per-lane functions (melonix_amd/csrc/denoise_core.h on onset_core.h's transform)
// run lane by lane on the CPU in the kernels' lane mapping and tile walk (melonix_amd/csrc/denoise_kernels.hip): a loop over the
// 64 lanes where the kernel has a barrier or a lane exchange, the same three frames of gains, middle spectrum and 16 accumulators
// per lane, the same stores.  Every index the kernel forms outside the image — samples of the padded take, power rows, outputs —
// is checked against the staged sizes and counted; the image is an array of exactly its size (the stand-alone form runs under
// AddressSanitizer).  The pads of the take hold NaN here: the definition takes zeros whatever they hold.  The host logic is the
// library's own unit, denoise_logic.cpp, compiled beside this file.  tests/test_denoise_host.py compares with tests/denoise_ref.py.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared denoise_emu.cpp ../../melonix_amd/csrc/denoise_logic.cpp -o libdenoise_emu.so
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../melonix_amd/csrc/denoise_core.h"
#include "../../melonix_amd/csrc/denoise_logic.h"
#include "../../melonix_amd/csrc/pcm16.h"

using namespace mx::dn;

namespace {

struct Wave {
  std::vector<float2> tw, img;
  std::vector<LaneConsts> lc;
  const float *wav;
  long long n, bad = 0;
  Wave(const float *wav_, long long n_) : tw(1024), img(kImage), lc(kLanes), wav(wav_), n(n_) {
    for (int j = 0; j < 1024; ++j) {
      const double ang = -2.0 * M_PI * (double)j / 1024.0;
      tw[(size_t)j].x = (float)std::cos(ang);
      tw[(size_t)j].y = (float)std::sin(ang);
    }
    for (int l = 0; l < kLanes; ++l) lane_consts(l, tw.data(), lc[(size_t)l]);
  }
  // the padded image's element MX_AUDIO_PAD + s: inside the allocation, NaN in the pads
  float image(long long s) {
    bad += s + MX_AUDIO_PAD < 0 || s + MX_AUDIO_PAD >= n + 2 * (long long)MX_AUDIO_PAD;
    return s >= 0 && s < n ? wav[s] : NAN;
  }
  void load(long long f, float2 (&x)[kLanes][8]) {
    for (int l = 0; l < kLanes; ++l)
      for (int r = 0; r < 8; ++r) {
        const long long s = (f - kLead) * kHop + 2 * l + 128 * r;
        x[l][r].x = masked(image(s), s, n);
        x[l][r].y = masked(image(s + 1), s + 1, n);
      }
  }
  // onset_walk.h's transform, then the split: the lanes' spectra and powers
  void analyse(float2 (&x)[kLanes][8], Spec (&u)[kLanes], float (&p)[kLanes][8], float (&p512)[kLanes]) {
    float2 v[kLanes][8];
    for (int l = 0; l < kLanes; ++l) pass1(l, lc[(size_t)l], x[l], img.data());
    for (int l = 0; l < kLanes; ++l) pass2(l, lc[(size_t)l], img.data(), v[l]);
    for (int l = 0; l < kLanes; ++l) store2(l, v[l], img.data());
    for (int l = 0; l < kLanes; ++l) pass3(l, img.data(), v[l]);
    for (int l = 0; l < kLanes; ++l) store3(l, v[l], img.data());
    for (int l = 0; l < kLanes; ++l) split(l, lc[(size_t)l], v[l], img.data(), u[l], p[l], p512[l]);
  }
};

}  // namespace

extern "C" long long emu_denoise_frames(long long n) { return frames_of(n); }
extern "C" void emu_denoise_factors(const mx_denoise_params *p, float *out) {
  const mx::DenoiseFactors f = mx::denoise_factors(*p);
  out[0] = f.floor, out[1] = f.sens;
}
extern "C" int emu_denoise_refuses(const mx_denoise_params *p, const float *print) {
  return (p && mx::denoise_params_error(*p) ? 1 : 0) | (print && mx::noise_print_error(print) ? 2 : 0);
}
extern "C" int emu_noise_region(long long n, long long begin, long long end, long long *first_frame, long long *count) {
  int64_t f = -1, c = -1;
  const bool ok = mx::noise_region_frames(n, begin, end, &f, &c);
  *first_frame = f, *count = c;
  return ok;
}
// the launch geometry of outputs [first, first + count) at `run` blocks a wavefront: tiles, and tile `index`
extern "C" long long emu_denoise_tiles(long long first, long long count, int run) { return tiles_of(first, count, run); }
extern "C" void emu_denoise_tile(long long first, long long count, long long n, long long index, int run, long long *out4) {
  const Tile t = tile_of(first, count, n, index, run);
  out4[0] = t.b0, out4[1] = t.b1, out4[2] = t.fa, out4[3] = t.F;
}

// Outputs [first, first + count) the kernel's way, `run` blocks a wavefront -> the number of indices that left what is staged
// (0: none).  f32, i16: count elements each, or null.
extern "C" long long emu_denoise(const float *wav, long long n, const float *print, float floor, float sens, long long first,
                                 long long count, int run, float *f32, int16_t *i16) {
  Wave w(wav, n);
  const long long out_end = first + count;
  const long long tiles = tiles_of(first, count, run);
  static float2 x[kLanes][8];
  static Spec um[kLanes], uc[kLanes];
  static float gA[kLanes][9], gB[kLanes][9], gC[kLanes][9], theta[kLanes][9];
  static Ola ola[kLanes];
  for (long long ti = 0; ti < tiles; ++ti) {
    const Tile t = tile_of(first, count, n, ti, run);
    if (t.b0 >= t.b1) {
      ++w.bad;  // (the grid has no idle tile)
      continue;
    }
    for (int l = 0; l < kLanes; ++l) {
      for (int r = 0; r < 8; ++r) theta[l][r] = sens * print[l + 64 * r];
      theta[l][8] = sens * print[kM];
      for (int r = 0; r < 9; ++r) gA[l][r] = gB[l][r] = gC[l][r] = 0.f;
      um[l] = uc[l] = Spec{};
      ola_clear(ola[l]);
    }
    const long long last = t.b1 + 3;
    w.bad += t.b1 + 2 > t.F - 1;  // (the last frame a tile synthesises exists)
    w.load(t.fa, x);
    for (long long f = t.fa; f <= last; ++f) {
      if (f < t.F) {
        float p[kLanes][8], p512[kLanes];
        w.analyse(x, uc, p, p512);
        if (f + 1 <= last && f + 1 < t.F) w.load(f + 1, x);  // (the kernel's prefetch, behind pass 1)
        for (int l = 0; l < kLanes; ++l) {
          for (int r = 0; r < 8; ++r) gC[l][r] = raw_gain(p[l][r], theta[l][r], floor);
          gC[l][8] = raw_gain(p512[l], theta[l][8], floor);
        }
      }
      if (f == t.fa)
        for (int l = 0; l < kLanes; ++l)
          for (int r = 0; r < 9; ++r) gB[l][r] = gC[l][r];
      if (f - 1 >= t.b0) {
        float tt[kLanes][8], tt512[kLanes], g[kLanes][8], g512[kLanes];
        for (int l = 0; l < kLanes; ++l) {
          for (int r = 0; r < 8; ++r) tt[l][r] = s121(gA[l][r], gB[l][r], gC[l][r]);
          tt512[l] = s121(gA[l][8], gB[l][8], gC[l][8]);
        }
        for (int l = 0; l < kLanes; ++l) {  // the lane exchange
          float up[8], dw[8];
          const int lu = (l + 1) & (kLanes - 1), ld = (l - 1) & (kLanes - 1);
          for (int r = 0; r < 8; ++r) {
            up[r] = pub_up(lu, tt[lu], tt512[lu], r);
            dw[r] = pub_dn(ld, tt[ld], r);
          }
          smooth_bins(l, tt[l], tt512[l], up, dw, tt[kLanes - 1][7], g[l], g512[l]);
        }
        float2 v[kLanes][8], c[kLanes][8];
        for (int l = 0; l < kLanes; ++l) scaled(l, um[l], g[l], g512[l], w.img.data(), v[l]);
        for (int l = 0; l < kLanes; ++l) unsplit(l, w.lc[(size_t)l], v[l], w.img.data(), c[l]);
        for (int l = 0; l < kLanes; ++l) ipass1(l, w.lc[(size_t)l], c[l], w.img.data());
        for (int l = 0; l < kLanes; ++l) pass2(l, w.lc[(size_t)l], w.img.data(), c[l]);
        for (int l = 0; l < kLanes; ++l) store2(l, c[l], w.img.data());
        for (int l = 0; l < kLanes; ++l) pass3(l, w.img.data(), c[l]);
        const long long b = f - 1 - kLead;
        for (int l = 0; l < kLanes; ++l) {
          float2 y[8];
          windowed(w.lc[(size_t)l], c[l], y);
          ola_add(ola[l], y);
          if (b >= t.b0 && b < t.b1)
            for (int h = 0; h < 2; ++h)
              for (int e = 0; e < 2; ++e) {
                const long long s = b * kHop + 128 * h + 2 * l + e;
                const float o = e ? ola[l].s[0][h].y : ola[l].s[0][h].x;
                if (s >= first && s < out_end) {
                  w.bad += s - first < 0 || s - first >= count || s >= n;
                  if (f32) f32[s - first] = o;
                  if (i16) i16[s - first] = mx::pcm16_clamped(o);
                }
              }
          ola_shift(ola[l]);
        }
      }
      for (int l = 0; l < kLanes; ++l) {
        for (int r = 0; r < 9; ++r) gA[l][r] = gB[l][r], gB[l][r] = gC[l][r];
        um[l] = uc[l];
      }
    }
  }
  return w.bad;
}

// The power rows of frames [first_frame, first_frame + count), `run` frames a wavefront -> the number of indices that left what
// is staged; rows: 513 count floats.
extern "C" long long emu_noise_rows(const float *wav, long long n, long long first_frame, long long count, int run, float *rows) {
  Wave w(wav, n);
  static float2 x[kLanes][8];
  static Spec u[kLanes];
  for (long long i0 = 0; i0 < count; i0 += run) {
    const long long i1 = i0 + run < count ? i0 + run : count;
    for (long long i = i0; i < i1; ++i) {
      w.load(first_frame + i, x);
      float p[kLanes][8], p512[kLanes];
      w.analyse(x, u, p, p512);
      for (int l = 0; l < kLanes; ++l) {
        for (int r = 0; r < 8; ++r) {
          const long long at = i * kBins + l + 64 * r;
          w.bad += at < 0 || at >= count * kBins;
          rows[at] = p[l][r];
        }
        if (l == 0) rows[i * kBins + kM] = p512[0];
      }
    }
  }
  return w.bad;
}
// the print kernel: one lane per bin walks the rows in ascending frame order in binary64
extern "C" void emu_noise_print(const float *rows, long long count, float *print) {
  for (int k = 0; k < kBins; ++k) {
    double s = 0.0;
    for (long long f = 0; f < count; ++f) s += (double)rows[f * kBins + k];
    print[k] = (float)(s / (double)count);
  }
}

#ifdef DENOISE_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_denoise_host.py): the walk over the smallest lengths, every run
// length and ranges cut anywhere must give the same bytes and leave no staged size; the rows and both forms of the print; the
// refusals of the host logic.
#include <cstdio>
#include <cstring>

int main() {
  long long bad = 0;
  const mx_denoise_params prm{24.f, 6.f};
  const mx::DenoiseFactors fc = mx::denoise_factors(prm);
  for (long long n : {0LL, 1LL, 255LL, 256LL, 257LL, 1023LL, 1024LL, 1025LL, 3001LL}) {
    std::vector<float> x((size_t)n + 1), print((size_t)kBins, 2e-6f);
    for (long long i = 0; i < n; ++i) x[(size_t)i] = 0.01f * (float)std::sin(0.37 * (double)i) * (float)((i * 7919) % 13 - 6) + (i % 97 == 0 ? 0.5f : 0.f);
    if (n > 600) x[(size_t)(n / 2)] = NAN, x[(size_t)(n - 1)] = INFINITY;
    std::vector<float> a((size_t)n + 1), b((size_t)n + 1);
    std::vector<int16_t> ia((size_t)n + 1), ib((size_t)n + 1);
    bad += emu_denoise(x.data(), n, print.data(), fc.floor, fc.sens, 0, n, 32, a.data(), ia.data());
    for (int run : {1, 5}) {
      bad += emu_denoise(x.data(), n, print.data(), fc.floor, fc.sens, 0, n, run, b.data(), ib.data());
      bad += std::memcmp(a.data(), b.data(), (size_t)n * sizeof(float)) != 0 || std::memcmp(ia.data(), ib.data(), (size_t)n * 2) != 0;
    }
    const long long cut = n / 3 + (n > 40 ? 37 : 0);
    if (cut <= n) {
      bad += emu_denoise(x.data(), n, print.data(), fc.floor, fc.sens, 0, cut, 5, b.data(), nullptr);
      bad += emu_denoise(x.data(), n, print.data(), fc.floor, fc.sens, cut, n - cut, 32, b.data() + cut, nullptr);
      bad += std::memcmp(a.data(), b.data(), (size_t)n * sizeof(float)) != 0;
    }
    const long long F = frames_of(n);
    std::vector<float> rows((size_t)(F * kBins)), rows2((size_t)(F * kBins)), p1((size_t)kBins), p2((size_t)kBins);
    bad += emu_noise_rows(x.data(), n, 0, F, 1, rows.data());
    bad += emu_noise_rows(x.data(), n, 0, F, 7, rows2.data());
    bad += std::memcmp(rows.data(), rows2.data(), rows.size() * sizeof(float)) != 0;
    emu_noise_print(rows.data(), F, p1.data());
    mx::noise_print_of_rows(rows.data(), F, p2.data());
    bad += std::memcmp(p1.data(), p2.data(), (size_t)kBins * sizeof(float)) != 0;
  }
  int64_t f0 = 0, cnt = 0;
  bad += !(mx::noise_region_frames(5000, 0, 1024, &f0, &cnt) && f0 == 3 && cnt == 1);
  bad += !(mx::noise_region_frames(5000, 1, 1024 + 256, &f0, &cnt) && f0 == 4 && cnt == 1);
  bad += mx::noise_region_frames(5000, 0, 1023, &f0, &cnt) || mx::noise_region_frames(5000, 10, 5001, &f0, &cnt) ||
         mx::noise_region_frames(5000, -1, 2000, &f0, &cnt) || mx::noise_region_frames(5000, 3000, 2000, &f0, &cnt);
  bad += !(mx::noise_region_frames(1024 + 8191 * 256, 0, 1024 + 8191 * 256, &f0, &cnt) && cnt == 8192);
  bad += mx::noise_region_frames(1024 + 8192 * 256, 0, 1024 + 8192 * 256, &f0, &cnt);
  const mx_denoise_params bads[] = {{-0.1f, 0.f}, {60.1f, 0.f}, {NAN, 0.f}, {10.f, -12.1f}, {10.f, 24.1f}, {10.f, NAN}};
  for (const mx_denoise_params &p : bads) bad += mx::denoise_params_error(p) == nullptr;
  bad += mx::denoise_params_error(mx_denoise_params{0.f, -12.f}) != nullptr || mx::denoise_params_error(mx_denoise_params{60.f, 24.f}) != nullptr;
  std::vector<float> pr((size_t)kBins, 0.f);
  bad += mx::noise_print_error(pr.data()) != nullptr;
  for (float v : {-1e-30f, NAN, INFINITY}) {
    pr[512] = v;
    bad += mx::noise_print_error(pr.data()) == nullptr;
  }
  printf(bad ? "denoise_emu FAILED %lld\n" : "denoise_emu ok\n", bad);
  return bad != 0;
}
#endif
