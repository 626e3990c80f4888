// sibilant_emu.cpp — the sibilant-feature kernel's per-lane functions (melonix_amd/csrc/sibilant_core.h on onset_core.h's
// transform, onset_walk_emu.h) run lane by lane on the CPU, in the walker's order: a run of consecutive frames, the wavefront's sums in the
// kernel's exchange order, the neighbour's sign mask where the kernel's lane exchange brings it.  And the source gain's
// arithmetic (gain_core.h) sample by sample.  tests/test_sibilant_host.py compares both with tests/sibilant_ref.py.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared sibilant_emu.cpp -o libsibilant_emu.so
#include "../../melonix_amd/csrc/gain_core.h"
#include "../../melonix_amd/csrc/sibilant_core.h"
#include "onset_walk_emu.h"

using namespace mx::sib;

extern "C" void emu_sib_features(const float *wav, long n, int hop, long first_frame, long count, int ks, int run, mx_sib_feat *out) {
  emu::Walk walk(wav, n);
  for (long f0 = 0; f0 < count; f0 += run) {
    const long f1 = f0 + run < count ? f0 + run : count;
    for (long h = first_frame + f0; h < first_frame + f1; ++h) {
      float2 v[kLanes][8];
      uint32_t first[kLanes], second[kLanes];
      walk.frame(h, hop, v, [&](int l, const float2(&x)[8]) { sign_masks(x, first[l], second[l]); });  // (of the raw samples)
      float low[kLanes], high[kLanes], moment[kLanes];
      int zc = 0;  // (an integer sum: any order)
      for (int l = 0; l < kLanes; ++l) {
        float P[8];
        powers(l, walk.lc[(size_t)l], v[l], walk.img.data(), P);
        const LaneSums s = lane_sums(l, P, ks);
        low[l] = s.low, high[l] = s.high, moment[l] = s.moment;
        zc += lane_crossings(l, first[l], second[l], first[(l + 1) & (kLanes - 1)]);
      }
      mx_sib_feat rec;
      rec.low = wave_sum_host(low);
      rec.high = wave_sum_host(high);
      rec.centroid = centroid_of(rec.low, rec.high, wave_sum_host(moment));
      rec.zero_crossings = zc;
      out[h - first_frame] = rec;
    }
  }
}

extern "C" void emu_audio_gain(const float *x, long n, const mx_gain_point *pts, long npts, float *out) {
  long j = 0;  // the number of points whose sample is <= i
  mx::gain::Segment seg = mx::gain::segment_at(pts, npts, j);
  for (long i = 0; i < n; ++i) {
    if (i >= seg.next) {
      do ++j;
      while (j < npts && (long)pts[j].sample <= i);
      seg = mx::gain::segment_at(pts, npts, j);
    }
    out[i] = mx::gain::gained(x[i], mx::gain::gain_at(seg, i));
  }
}

#ifdef SIBILANT_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_sibilant_host.py): the emulation and the library's host logic
// (melonix_amd/csrc/sibilant_logic.cpp, compiled beside this file) over the smallest shapes and the edges of every list.
#include <cstdio>

#include "../../melonix_amd/csrc/sibilant_logic.h"

int main() {
  int bad = 0;
  for (long n : {1L, 255L, 767L, 1500L}) {
    std::vector<float> w((size_t)n);
    for (long i = 0; i < n; ++i) w[(size_t)i] = 0.1f * (float)std::sin(1.9 * (double)i) * (i % 3 ? 1.f : -1.f);
    for (int hop : {1, 255, 256}) {
      const long frames = (n + hop - 1) / hop;
      std::vector<mx_sib_feat> a((size_t)frames), b((size_t)frames);
      emu_sib_features(w.data(), n, hop, 0, frames, 75, 1, a.data());
      emu_sib_features(w.data(), n, hop, 0, frames, 75, 5, b.data());
      for (long f = 0; f < frames; ++f)
        bad += a[(size_t)f].low != b[(size_t)f].low || a[(size_t)f].zero_crossings != b[(size_t)f].zero_crossings;
      const mx_sibilant_params p{0.6, 0.4, 1e-3, 64, 2, 1};
      const std::vector<mx_sibilant> s = mx::sibilant_segments(a.data(), frames, hop, 0, p);
      for (size_t i = 1; i < s.size(); ++i) bad += s[i].start_sample <= s[i - 1].end_sample;
    }
  }
  // runs at frame 0 and at the last frame, a gap of merge_gap and of merge_gap + 1, NaN / Inf records, counts 0 and 1
  std::vector<mx_sib_feat> f(40, mx_sib_feat{1e-3f, 1e-5f, 10.f, 20});
  const mx_sib_feat hiss{1e-5f, 1e-3f, 300.f, 300};
  for (int i : {0, 1, 2, 5, 6, 10, 11, 37, 38, 39}) f[(size_t)i] = hiss;
  f[20] = mx_sib_feat{NAN, 1.f, NAN, 300};
  f[21] = mx_sib_feat{INFINITY, INFINITY, NAN, 300};
  const mx_sibilant_params p{0.6, 0.4, 1e-3, 64, 2, 2};
  const std::vector<mx_sibilant> s = mx::sibilant_segments(f.data(), 40, 256, 3, p);
  bad += !(s.size() == 3 && s[0].first_frame == 3 && s[0].frames == 7 && s[1].first_frame == 13 && s[2].frames == 3);
  bad += !mx::sibilant_segments(nullptr, 0, 256, 0, p).empty();
  bad += mx::sibilant_segments(&hiss, 1, 256, 0, p).size() != 0;
  // spans: clipped at 0 and at n - 1, overlapping ramps, a sibilant on a curve point, an empty curve
  const mx_sibilant sibs[] = {{0, 50, 0, 1, 0.9f, 0.1f}, {300, 400, 0, 1, 0.9f, 0.1f}, {560, 600, 0, 1, 0.9f, 0.1f}, {990, 999, 0, 1, 0.9f, 0.1f}};
  const mx_formant_point curve[] = {{-5, 1.f}, {300, 4.f}, {700, 2.f}, {5000, 0.f}};
  bad += mx::sibilant_list_error(sibs, 4, 1000) != nullptr || mx::sibilant_list_error(sibs, 4, 999) == nullptr;
  const std::vector<mx_formant_point> g = mx::formant_protect(curve, 4, sibs, 4, 80, 1000);
  bad += mx::formant_curve_error(g.data(), (int64_t)g.size()) != nullptr || g.front().sample != -5 || g.back().sample != 5000;
  bad += !mx::formant_protect(curve, 0, sibs, 4, 80, 1000).empty();
  const std::vector<mx_gain_point> gp = mx::sibilant_gain_points(sibs, 4, -6.0, 80, 1000);
  bad += mx::gain_points_error(gp.data(), (int64_t)gp.size()) != nullptr || gp.front().sample != 0 || gp.back().sample != 999;
  std::vector<float> x(1000, 0.5f), y(1000);
  emu_audio_gain(x.data(), 1000, gp.data(), (long)gp.size(), y.data());
  bad += !(y[0] == 0.5f * gp[0].amp && y[200] == 0.5f && y[999] == 0.5f * gp.back().amp);
  emu_audio_gain(x.data(), 1, gp.data(), 1, y.data());
  printf(bad ? "sibilant_emu FAILED %d\n" : "sibilant_emu ok\n", bad);
  return bad != 0;
}
#endif
