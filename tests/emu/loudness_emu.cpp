// loudness_emu.cpp — the loudness kernel's per-lane functions (melonix_amd/csrc/loudness_core.h) run group by group on the CPU, in
// the lane's order: W warm-up samples from zero state, zeros before the file, then the group's steps up to the end of the file.
// tests/test_loudness_host.py compares the records with tests/loudness_ref.py byte for byte.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared loudness_emu.cpp -o libloudness_emu.so
#include "../../melonix_amd/csrc/loudness_core.h"

using namespace mx::loud;

// the records of steps [G*first_group, min(G*(first_group + ngroups), steps)) -> out; k: mx_loudness_coeffs' ten values
extern "C" void emu_loudness_steps(const float *wav, long n, int sr, long first_group, long ngroups, const double *k, mx_loud_step *out) {
  const Geometry q = geometry(n, sr);
  const Coeffs c{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9]};
  for (long g = first_group; g < first_group + ngroups; ++g) {
    const long gstart = g * kGroupSteps * q.S, end = gstart + kGroupSteps * q.S < n ? gstart + kGroupSteps * q.S : n;
    mx_loud_step *rec = out + (g - first_group) * kGroupSteps;
    Lane l = lane_zero();
    int in_step = 0;
    for (long i = gstart - q.W; i < end; ++i) {
      const float x = i < 0 ? 0.f : wav[i];
      const double z = filter(c, l, x);
      if (i < gstart) continue;
      accumulate(l, x, z);
      if (++in_step == q.S || i == end - 1) {
        *rec++ = record(l, in_step);
        step_zero(l);
        in_step = 0;
      }
    }
  }
}

#ifdef LOUDNESS_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_loudness_host.py): the emulation and the library's host logic
// (melonix_amd/csrc/loudness_logic.cpp, compiled beside this file) over the smallest shapes and the edges of every list.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../melonix_amd/csrc/loudness_logic.h"

int main() {
  int bad = 0;
  for (int sr : {8000, 44100}) {
    double k[10];
    mx::loudness_coeffs(sr, k);
    const int S = geometry(0, sr).S;
    for (long n : {1L, (long)S - 1, (long)S, (long)S + 1, 10L * S, 10L * S + 1, 47L * S + 5}) {
      std::vector<float> w((size_t)n);
      for (long i = 0; i < n; ++i) w[(size_t)i] = 0.3f * (float)std::sin(0.07 * (double)i);
      const Geometry q = geometry(n, sr);
      std::vector<mx_loud_step> a((size_t)q.steps), b((size_t)q.steps);
      emu_loudness_steps(w.data(), n, sr, 0, q.groups, k, a.data());
      for (long g = 0; g < q.groups; ++g) emu_loudness_steps(w.data(), n, sr, g, 1, k, b.data() + g * kGroupSteps);  // group by group
      for (long s = 0; s < q.steps; ++s) bad += a[(size_t)s].energy != b[(size_t)s].energy || a[(size_t)s].samples != b[(size_t)s].samples;
      bad += a.back().samples != (int)(n - (q.steps - 1) * S) || mx::loud_steps_error(a.data(), q.steps, S) != nullptr;
      // every window length against a list shorter and longer than it; notes at both ends, one shorter than a step
      std::vector<double> curve((size_t)q.steps);
      for (int window : {1, 40, 300}) mx::loudness_curve(a.data(), q.steps, S, window, curve.data());
      mx_loudness m;
      mx::loudness_integrated(a.data(), q.steps, S, &m);
      bad += m.blocks != (q.steps - (a.back().samples != S) >= 40 ? (q.steps - (a.back().samples != S) - 40) / 10 + 1 : 0);
      mx_note notes[2] = {};
      notes[0].start_sample = 0, notes[0].end_sample = (int32_t)(n - 1);
      notes[1].start_sample = (int32_t)(n - 1), notes[1].end_sample = (int32_t)(n - 1);
      double lufs[2];
      int64_t at = 0;
      bad += !mx::note_loudness(a.data(), q.steps, S, notes, 2, lufs, &at);
      notes[1].end_sample = (int32_t)(n + S);
      notes[1].start_sample = (int32_t)n;
      bad += mx::note_loudness(a.data(), q.steps, S, notes, 2, lufs, &at) || at != 1;
    }
  }
  bad += mx::loud_steps_error(nullptr, 0, 480) != nullptr;
  mx_loudness none;
  mx::loudness_integrated(nullptr, 0, 480, &none);
  bad += !(none.blocks == 0 && none.integrated < 0 && std::isinf(none.integrated) && none.peak == 0.f);
  const mx_note notes[3] = {{100, 200, 0, 1, 45.0, 0.f, 0.f}, {300, 400, 1, 1, 45.0, 0.f, 0.f}, {500, 600, 2, 1, 45.0, 0.f, 0.f}};
  const double lufs[3] = {-20.0, NAN, -30.0};
  mx_gain_point pts[6];
  const double ref = mx::level_gain_points(notes, 3, lufs, mx_level_params{1.0, 1.0, 3.0}, pts);
  bad += !(ref == -25.0 && pts[2].amp == 1.f && pts[0].amp < 1.f && pts[5].amp > 1.f && pts[5].sample == 600);
  bad += !std::isnan(mx::level_gain_points(notes, 0, lufs, mx_level_params{1.0, 1.0, 3.0}, pts));
  bad += !(mx::normalize_amp(-20.0, 0.5, -23.0, -1.0) < 1.0);
  printf(bad ? "loudness_emu FAILED %d\n" : "loudness_emu ok\n", bad);
  return bad != 0;
}
#endif
