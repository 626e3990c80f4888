// compress_emu.cpp — the compressor kernels' arithmetic (melonix_amd/csrc/compress_core.h) run on the CPU in the kernels' lane
// mapping and launch geometry (melonix_amd/csrc/compress_kernels.hip): P lanes a step and a shuffle maximum for the peaks, a
// wavefront a group with 64 targets at a time for the curve, a lane an aligned quad for the product; and the sizing of the work
// memory as capi_compress.cpp does it.  Every index the kernels form — quads of the padded take, peaks, the table, the curve,
// outputs — is checked against the staged sizes and counted; the buffers are arrays of exactly those sizes (the stand-alone form
// runs under AddressSanitizer).  The pads of the take hold NaN here: the definition takes no sample outside the file.  The host
// logic is the library's own unit, compress_logic.cpp, compiled beside this file.  tests/test_compress_host.py compares with
// tests/compress_ref.py.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared compress_emu.cpp ../../melonix_amd/csrc/compress_logic.cpp -o libcompress_emu.so
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../melonix_amd/csrc/compress_core.h"
#include "../../melonix_amd/csrc/compress_logic.h"
#include "../../melonix_amd/csrc/pcm16.h"

using namespace mx::cp;

namespace {

constexpr int kThreads = 256, kWave = 64;

struct Quad {
  float v[4];
};
// the padded image of a take, NaN in the pads, and image_quads.h's load_quad on it
struct Image {
  std::vector<float> img;
  long long n, bad = 0;
  Image(const float *wav, long long n_) : img((size_t)n_ + 2 * MX_AUDIO_PAD, NAN), n(n_) {
    if (n) std::memcpy(img.data() + MX_AUDIO_PAD, wav, (size_t)n * sizeof(float));
  }
  Quad load_quad(long long quad) {
    Quad q{};
    if (quad < 0 || 4 * quad + 3 >= (long long)img.size()) {
      ++bad;
      return q;
    }
    const long long i = 4 * quad - MX_AUDIO_PAD;
    for (int e = 0; e < 4; ++e) q.v[e] = i + e < 0 || i + e >= n ? 0.f : img[(size_t)(4 * quad + e)];
    return q;
  }
};

long long peaks_launch(Image &im, int D, long long first_step, long long nsteps, float *out) {
  long long bad = 0;
  if (nsteps <= 0) return 0;
  const int P = lanes_per_step(D);
  bad += P < 2 || P > kWave || kWave % P != 0;
  const long long blocks = (nsteps * P + kThreads - 1) / kThreads;
  for (long long w0 = 0; w0 < blocks * kThreads; w0 += kWave) {  // a wavefront
    float peak[kWave];
    long long slot[kWave];
    for (int l = 0; l < kWave; ++l) {
      slot[l] = (w0 + l) / P;
      const int sub = (int)((w0 + l) % P);
      peak[l] = 0.f;
      const long long b = first_step + slot[l];
      const long long a0 = b * D, a1 = a0 + D < im.n ? a0 + D : im.n;
      if (slot[l] < nsteps && b >= 0 && a0 < im.n) {
        const long long ka = (a0 + MX_AUDIO_PAD) / 4, kb = (a1 - 1 + MX_AUDIO_PAD) / 4;
        for (long long k = ka + sub; k <= kb; k += P) {
          const Quad q = im.load_quad(k);
          const long long i0 = 4 * k - MX_AUDIO_PAD;
          for (int e = 0; e < 4; ++e) {
            if (i0 + e < a0 || i0 + e >= a1) continue;
            const float m = magnitude(q.v[e]);
            peak[l] = m > peak[l] ? m : peak[l];
          }
        }
      }
    }
    for (int d = P / 2; d > 0; d >>= 1) {  // __shfl_xor
      float o[kWave];
      for (int l = 0; l < kWave; ++l) o[l] = peak[l ^ d];
      for (int l = 0; l < kWave; ++l) peak[l] = o[l] > peak[l] ? o[l] : peak[l];
    }
    for (int l = 0; l < kWave; ++l)
      if (slot[l] < nsteps && (w0 + l) % P == 0) {
        bad += slot[l] < 0 || slot[l] >= nsteps;
        out[slot[l]] = peak[l];
      }
  }
  return bad + im.bad;
}

long long curve_launch(const float *peaks, long long peaks_first, long long npeaks, const int32_t *table, int c_att, int c_rel, int W,
                       long long g0, long long groups, long long total, int32_t *out, long long out_first, long long out_end) {
  long long bad = 0;
  for (long long gi = 0; gi < groups; ++gi) {
    const long long g = g0 + gi;
    const long long start = group_start(g, W), end = group_end(g, total), own = g * kGroup;
    bad += end <= own;  // (the grid has no idle group)
    int32_t s = kUnity;
    for (long long c0 = start; c0 < end; c0 += kWave) {
      int32_t q[kWave], mine[kWave];
      for (int l = 0; l < kWave; ++l) {
        const long long b = c0 + l;
        float p = 0.f;
        if (b < end) {
          bad += b - peaks_first < 0 || b - peaks_first >= npeaks;
          p = peaks[b - peaks_first];
        }
        bad += !(p >= 0.f);
        q[l] = target(table, p);
        mine[l] = 0;
      }
      const int cnt = end - c0 < kWave ? (int)(end - c0) : kWave;
      for (int i = 0; i < cnt; ++i) {
        s = smoothed(s, q[i], c_att, c_rel);
        mine[i] = s;
      }
      for (int l = 0; l < kWave; ++l) {
        const long long b = c0 + l;
        if (b < end && b >= own && b >= out_first && b < out_end) out[b - out_first] = mine[l];
      }
    }
  }
  return bad;
}

long long apply_launch(Image &im, int D, int K, float makeup, const int32_t *curve, long long curve_first, long long ncurve,
                       long long first, long long count, float *f32, int16_t *i16) {
  long long bad = 0;
  if (count <= 0) return 0;
  const long long last = first + count;
  const long long quads = (first + count - 1 + MX_AUDIO_PAD) / 4 - (first + MX_AUDIO_PAD) / 4 + 1;
  const long long threads = (quads + kThreads - 1) / kThreads * kThreads;
  const long long lo = gain_lo(first, D, K), hi = gain_hi(first, count, D, K);
  auto gain = [&](long long u) {
    if (u < lo || u > hi) return kUnity;
    if (u - curve_first < 0 || u - curve_first >= ncurve) {
      ++bad;
      return kUnity;
    }
    return curve[u - curve_first];
  };
  for (long long t = 0; t < threads; ++t) {
    const long long k = (first + MX_AUDIO_PAD) / 4 + t, i0 = 4 * k - MX_AUDIO_PAD;
    if (i0 >= last) continue;
    bad += i0 < 0 || i0 > first + 4 * t;
    const Quad x = im.load_quad(k);
    long long u = i0 / D;
    int o = (int)(i0 - u * D);
    u += K;
    int32_t s0 = gain(u - 1), s1 = gain(u);
    for (int e = 0; e < 4; ++e) {
      if (o == D) {
        o = 0;
        ++u;
        s0 = s1;
        s1 = gain(u);
      }
      const float y = compressed(x.v[e], makeup, gain_product(s0, s1, D, o), D);
      ++o;
      const long long i = i0 + e;
      if (i >= first && i < last) {
        bad += i - first < 0 || i - first >= count || i >= im.n;
        if (f32) f32[i - first] = y;
        if (i16) i16[i - first] = mx::pcm16_clamped(y);
      }
    }
  }
  return bad + im.bad;
}

// capi_compress.cpp's curve_enqueue: the peaks and the curve of the groups that hold steps [u_lo, u_hi]
struct Curve {
  std::vector<float> peaks;
  std::vector<int32_t> work;
  long long first = 0, bad = 0;
};
void curve_of(Image &im, const mx_compress_params &p, const mx_compress_plan &plan, long long u_lo, long long u_hi, int32_t *out,
              long long out_first, long long out_end, Curve &c) {
  const long long total = curve_steps(im.n, plan.D, plan.K);
  const long long g0 = u_lo / kGroup, g1 = u_hi / kGroup + 1;
  const long long pk_first = group_start(g0, plan.W), pk_end = group_end(g1 - 1, total);
  std::vector<int32_t> table((size_t)kCurve);
  mx::compress_curve(p, table.data());
  c.bad += u_lo < 0 || u_hi >= total || u_hi < u_lo || pk_end <= pk_first;
  c.peaks.assign((size_t)(pk_end - pk_first), NAN);
  c.bad += peaks_launch(im, plan.D, pk_first, pk_end - pk_first, c.peaks.data());
  if (!out) {
    out_first = g0 * kGroup, out_end = pk_end;
    c.work.assign((size_t)(out_end - out_first), 0);
    out = c.work.data();
    c.first = out_first;
  }
  c.bad += curve_launch(c.peaks.data(), pk_first, pk_end - pk_first, table.data(), plan.c_att, plan.c_rel, plan.W, g0, g1 - g0, total,
                        out, out_first, out_end);
}

}  // namespace

extern "C" int emu_compress_refuses(const mx_compress_params *p) { return mx::compress_params_error(*p) != nullptr; }
extern "C" void emu_compress_plan(int sr, const mx_compress_params *p, mx_compress_plan *out) { *out = mx::compress_plan(sr, *p); }
extern "C" void emu_compress_table(const mx_compress_params *p, int32_t *out) { mx::compress_curve(*p, out); }
extern "C" long long emu_compress_steps(long long n, int sr) { return steps_of(n, step_samples(sr)); }

// p_b of steps [first_step, first_step + nsteps) -> the number of indices that left what is staged (0: none)
extern "C" long long emu_compress_peaks(const float *wav, long long n, int sr, long long first_step, long long nsteps, float *out) {
  Image im(wav, n);
  return peaks_launch(im, step_samples(sr), first_step, nsteps, out);
}
// s_b of steps [first_step, first_step + nsteps) of [0, B), as mx_compress_gain_dev
extern "C" long long emu_compress_gain(const float *wav, long long n, int sr, const mx_compress_params *p, long long first_step,
                                       long long nsteps, int32_t *out) {
  if (nsteps <= 0) return 0;
  Image im(wav, n);
  Curve c;
  curve_of(im, *p, mx::compress_plan(sr, *p), first_step, first_step + nsteps - 1, out, first_step, first_step + nsteps, c);
  return c.bad;
}
// outputs [first, first + count), as mx_compress_dev; f32, i16: count elements each, or null
extern "C" long long emu_compress(const float *wav, long long n, int sr, const mx_compress_params *p, long long first, long long count,
                                  float *f32, int16_t *i16) {
  if (count <= 0) return 0;
  Image im(wav, n);
  const mx_compress_plan plan = mx::compress_plan(sr, *p);
  Curve c;
  curve_of(im, *p, plan, gain_lo(first, plan.D, plan.K), gain_hi(first, count, plan.D, plan.K), nullptr, 0, 0, c);
  return c.bad + apply_launch(im, plan.D, plan.K, p->makeup_amp, c.work.data(), c.first, (long long)c.work.size(), first, count, f32, i16);
}

#ifdef COMPRESS_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_compress_host.py): the three launches over the smallest lengths, at
// four rates, ranges cut anywhere must give the same bytes and leave no staged size; the refusals of the host logic.
#include <cstdio>

int main() {
  long long bad = 0;
  const mx_compress_params dflt = mx::compress_defaults();
  mx_compress_params look = dflt, slow = dflt;
  look.lookahead_ms = 20.f, look.makeup_amp = 2.f;
  slow.attack_ms = 50.f, slow.release_ms = 2000.f, slow.lookahead_ms = 5.f;
  for (int sr : {48000, 44100, 8000, 384000}) {
    const int D = step_samples(sr);
    for (long long n : {0LL, 1LL, (long long)D - 1, (long long)D, (long long)D + 1, 3001LL, (long long)kGroup * D + 5}) {
      if (sr == 384000 && n > 4000) continue;
      std::vector<float> x((size_t)n + 1);
      for (long long i = 0; i < n; ++i)
        x[(size_t)i] = 0.3f * (float)std::sin(0.37 * (double)i) * (float)((i / 700) % 5) * 0.5f + (i % 977 == 0 ? 1.5f : 0.f);
      if (n > 600) x[(size_t)(n / 2)] = NAN, x[(size_t)(n - 1)] = INFINITY;
      const mx_compress_params *sets[] = {&dflt, &look, &slow};
      for (const mx_compress_params *pp : sets) {
        if (n > 4000 && pp == &slow && sr != 48000) continue;
        const mx_compress_params &p = *pp;
        std::vector<float> a((size_t)n + 1), b((size_t)n + 1);
        std::vector<int16_t> ia((size_t)n + 1), ib((size_t)n + 1);
        bad += emu_compress(x.data(), n, sr, &p, 0, n, a.data(), ia.data());
        const long long cut = n / 3 + (n > 120 ? 37 : 0);
        bad += emu_compress(x.data(), n, sr, &p, 0, cut, b.data(), ib.data());
        bad += emu_compress(x.data(), n, sr, &p, cut, n - cut, b.data() + cut, ib.data() + cut);
        bad += std::memcmp(a.data(), b.data(), (size_t)n * sizeof(float)) != 0 || std::memcmp(ia.data(), ib.data(), (size_t)n * 2) != 0;
        const long long B = emu_compress_steps(n, sr);
        std::vector<int32_t> g((size_t)B + 1), h((size_t)B + 1);
        std::vector<float> pk((size_t)B + 1);
        bad += emu_compress_gain(x.data(), n, sr, &p, 0, B, g.data());
        bad += emu_compress_gain(x.data(), n, sr, &p, 0, B / 2, h.data());
        bad += emu_compress_gain(x.data(), n, sr, &p, B / 2, B - B / 2, h.data() + B / 2);
        bad += std::memcmp(g.data(), h.data(), (size_t)B * sizeof(int32_t)) != 0;
        bad += emu_compress_peaks(x.data(), n, sr, 0, B, pk.data());
        for (long long s = 0; s < B; ++s) bad += g[(size_t)s] < 1 || g[(size_t)s] > kUnity || !(pk[(size_t)s] >= 0.f);
      }
    }
  }
  const mx_compress_params bads[] = {{-60.1f, 4, 6, 5, 100, 0, 1},  {0.1f, 4, 6, 5, 100, 0, 1},   {-18, 0.9f, 6, 5, 100, 0, 1},
                                     {-18, 100.5f, 6, 5, 100, 0, 1}, {-18, 4, -0.1f, 5, 100, 0, 1}, {-18, 4, 24.1f, 5, 100, 0, 1},
                                     {-18, 4, 6, -1, 100, 0, 1},     {-18, 4, 6, 501, 100, 0, 1},   {-18, 4, 6, 5, -1, 0, 1},
                                     {-18, 4, 6, 5, 2001, 0, 1},     {-18, 4, 6, 5, 100, -1, 1},    {-18, 4, 6, 5, 100, 20.1f, 1},
                                     {-18, 4, 6, 5, 100, 0, 0.06f},  {-18, 4, 6, 5, 100, 0, 16.1f}, {-18, 4, 6, 5, 100, 0, 0},
                                     {NAN, 4, 6, 5, 100, 0, 1},      {-18, NAN, 6, 5, 100, 0, 1},   {-18, 4, NAN, 5, 100, 0, 1},
                                     {-18, 4, 6, NAN, 100, 0, 1},    {-18, 4, 6, 5, NAN, 0, 1},     {-18, 4, 6, 5, 100, NAN, 1},
                                     {-18, 4, 6, 5, 100, 0, NAN},    {-18, 4, 6, 5, 100, 0, INFINITY}};
  for (const mx_compress_params &p : bads) bad += mx::compress_params_error(p) == nullptr;
  bad += mx::compress_params_error(mx_compress_params{-60, 1, 0, 0, 0, 0, 0.0625f}) != nullptr;
  bad += mx::compress_params_error(mx_compress_params{0, 100, 24, 500, 2000, 20, 16}) != nullptr;
  const mx_compress_plan q = mx::compress_plan(48000, dflt);
  bad += !(q.D == 48 && q.K == 0 && q.W == 1616 && q.Gc == kGroup);
  printf(bad ? "compress_emu FAILED %lld\n" : "compress_emu ok\n", bad);
  return bad != 0;
}
#endif
