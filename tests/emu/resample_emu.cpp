// resample_emu.cpp — the sample-rate conversion's arithmetic (melonix_amd/csrc/resample_core.h) run on the CPU, twice: output by
// output the plain way (the 64-bit index map, a window read sample by sample with zeros outside the file, the table with a row
// per phase), and tile by tile the way resample_kernels.hip walks (the launch's geometry, one 64-bit map per tile and the 32-bit
// one per output, the window staged as aligned quads of a padded image, the table with a row per tap index), where every index the
// kernel would form is checked against the staged sizes.  The table is the library's own unit, resample_logic.cpp, compiled
// beside this file.  tests/test_resample_host.py compares both with tests/resample_ref.py byte for byte.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared resample_emu.cpp ../../melonix_amd/csrc/resample_logic.cpp -o libresample_emu.so
#include <vector>

#include "../../melonix_amd/csrc/resample_core.h"
#include "../../melonix_amd/csrc/resample_logic.h"

using namespace mx::rs;

extern "C" int emu_resample_plan(int in, int out, mx_resample_plan *p) { return plan_for(in, out, p) ? 0 : -1; }
extern "C" long long emu_resample_length(long long n, const mx_resample_plan *p) { return out_length(n, *p); }
extern "C" void emu_resample_table(const mx_resample_plan *p, float *out) { mx::resample_table(*p, out); }
extern "C" double emu_resample_i0(double x) { return mx::resample_bessel_i0(x); }
// (i_j, phi_j) of output j by the 64-bit map
extern "C" void emu_resample_at(long long j, const mx_resample_plan *p, long long *i, int *phase) {
  const At a = at(j, *p);
  *i = a.i;
  *phase = a.phase;
}
// ... and by the tile's map: base = at(j0), then at_offset(base, o); -> whether it is at(j0 + o)
extern "C" int emu_resample_at_offset_agrees(long long j0, int o, const mx_resample_plan *p) {
  const At a = at_offset(at(j0, *p), o, *p), b = at(j0 + o, *p);
  return a.i == b.i && a.phase == b.phase;
}
extern "C" void emu_resample_geometry(const mx_resample_plan *p, int *tile, int *win_quads, int *lds_table) {
  const Geometry g = geometry(*p);
  *tile = g.tile, *win_quads = g.win_quads, *lds_table = g.lds_table;
}

// outputs [first, first + count) -> out, output by output; table: h[phi][k]
extern "C" void emu_resample(const float *wav, long long n, const mx_resample_plan *pp, const float *table, long long first, long long count,
                             float *out) {
  const mx_resample_plan p = *pp;
  if (p.taps == 0) {
    for (long long j = 0; j < count; ++j) out[j] = wav[first + j];
    return;
  }
  std::vector<float> w((size_t)p.taps);
  for (long long j = first; j < first + count; ++j) {
    const At a = at(j, p);
    for (int k = 0; k < p.taps; ++k) {
      const long long s = a.i - (p.half - 1) + k;
      w[(size_t)k] = s >= 0 && s < n ? wav[s] : 0.f;
    }
    const int xo[1] = {0}, ho[1] = {a.phase * p.taps};
    float y[1];
    dots<1>(w.data(), xo, table, ho, 1, p.taps, y);
    out[j - first] = y[0];
  }
}

// The same outputs the kernel's way -> the number of indices that left what a workgroup stages (0: none).  pad: the samples of
// padding either side of the image the quads are cut from (a multiple of 4, at least 256); by_tap: h[k][phi].
extern "C" long long emu_resample_tiled(const float *wav, long long n, const mx_resample_plan *pp, const float *by_tap, long long first,
                                        long long count, float *out) {
  const mx_resample_plan p = *pp;
  const long long pad = MX_AUDIO_PAD;
  const Geometry g = geometry(p);
  long long bad = 0;
  bad += (long long)g.win_quads * 16 + (g.lds_table ? (long long)p.L * p.taps * 4 : 0) > kLdsBytes;
  bad += g.tile < 256 || g.tile > kMaxTile || g.tile % 256;
  std::vector<float> stage((size_t)g.win_quads * 4);
  for (long long t0 = 0; t0 < count; t0 += g.tile) {
    const int cnt = (int)(count - t0 < g.tile ? count - t0 : g.tile);
    const At base = at(first + t0, p), last = at_offset(base, cnt - 1, p);
    const long long lo = base.i - (p.half - 1), hi = last.i + p.half;
    const long long q0 = (lo + pad) >> 2;
    const int nq = (int)(((hi + pad) >> 2) - q0) + 1;
    bad += lo + pad < 0 || nq > g.win_quads || 4 * (q0 + nq) > n + 2 * pad;
    for (int k = 0; k < 4 * nq && k < 4 * g.win_quads; ++k) {
      const long long s = 4 * q0 - pad + k;
      stage[(size_t)k] = s >= 0 && s < n ? wav[s] : 0.f;
    }
    const int x0 = (int)(lo - (4 * q0 - pad));
    for (int o = 0; o < cnt; ++o) {
      const At a = at_offset(base, o, p);
      const int xo[1] = {x0 + (int)(a.i - base.i)}, ho[1] = {a.phase};
      bad += xo[0] < 0 || xo[0] + p.taps > 4 * nq || a.phase < 0 || a.phase >= p.L;
      float y[1] = {0.f};
      if (xo[0] >= 0 && xo[0] + p.taps <= 4 * g.win_quads) dots<1>(stage.data(), xo, by_tap, ho, p.L, p.taps, y);
      out[t0 + o] = y[0];
    }
  }
  return bad;
}

#ifdef RESAMPLE_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_resample_host.py): the table of every ratio class, and both walks over
// the smallest lengths, a length of several tiles and ranges cut anywhere; they must agree bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>

int main() {
  long long bad = 0;
  const int pairs[][2] = {{48000, 44100}, {44100, 48000}, {96000, 48000}, {48000, 96000}, {8000, 48000}, {8000, 44100}, {192000, 44100},
                          {44100, 8000}, {8000, 8192}, {384000, 48000}};
  for (const auto &pr : pairs) {
    mx_resample_plan p;
    if (!plan_for(pr[0], pr[1], &p)) {
      ++bad;
      continue;
    }
    std::vector<float> rows((size_t)p.L * p.taps), by_tap((size_t)p.L * p.taps);
    mx::resample_table(p, rows.data());
    mx::resample_table_by_tap(p, by_tap.data());
    for (long long n : {0LL, 1LL, 2LL, (long long)p.M - 1, (long long)p.M, (long long)p.M + 1, (long long)p.taps, 30011LL}) {
      std::vector<float> w((size_t)n);
      for (long long i = 0; i < n; ++i) w[(size_t)i] = 0.7f * (float)std::sin(0.37 * (double)i) + (i % 97 == 0 ? 0.9f : 0.f);
      if (n > 2) w[(size_t)(n / 2)] = NAN, w[(size_t)(n - 1)] = INFINITY;
      const long long m = out_length(n, p);
      std::vector<float> a((size_t)m + 1), b((size_t)m + 1);
      emu_resample(w.data(), n, &p, rows.data(), 0, m, a.data());
      bad += emu_resample_tiled(w.data(), n, &p, by_tap.data(), 0, m, b.data());
      bad += std::memcmp(a.data(), b.data(), (size_t)m * sizeof(float)) != 0;
      const long long cut = m / 3;
      bad += emu_resample_tiled(w.data(), n, &p, by_tap.data(), 0, cut, b.data());
      bad += emu_resample_tiled(w.data(), n, &p, by_tap.data(), cut, m - cut, b.data() + cut);
      bad += std::memcmp(a.data(), b.data(), (size_t)m * sizeof(float)) != 0;
    }
  }
  mx_resample_plan p;
  bad += plan_for(384000, 44100, &p) || plan_for(44100, 48001, &p) || plan_for(7999, 48000, &p) || plan_for(48000, 384001, &p);
  bad += !(plan_for(48000, 48000, &p) && p.L == 1 && p.M == 1 && p.taps == 0);
  printf(bad ? "resample_emu FAILED %lld\n" : "resample_emu ok\n", bad);
  return bad != 0;
}
#endif
