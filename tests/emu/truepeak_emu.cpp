// truepeak_emu.cpp — the true-peak kernels' per-sample functions (melonix_amd/csrc/truepeak_core.h) run sample by sample on the
// CPU: the window of every sample with zeros outside the file, its peak, the Q30 quotient, then the limiter's window minima and
// their sums the plain way (a loop over every window, a loop over every sum: no sparse table, no prefix sums), and the final
// product.
// tests/test_truepeak_host.py compares records and limited samples with tests/truepeak_ref.py byte for byte.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared truepeak_emu.cpp -o libtruepeak_emu.so
#include <vector>

#include "../../melonix_amd/csrc/pcm16.h"
#include "../../melonix_amd/csrc/truepeak_core.h"

using namespace mx::tp;

// p_i of sample i: the window x[i - 5 .. i + 6], zeros outside [0, n)
static float peak_at(const float *wav, long n, long i, int L) {
  float w[kTaps];
  for (int k = 0; k < kTaps; ++k) {
    const long j = i - kBefore + k;
    w[k] = j >= 0 && j < n ? wav[j] : 0.f;
  }
  return sample_peak(w, L);
}

// the records of steps [first_step, first_step + nsteps) -> out
extern "C" void emu_true_peak_steps(const float *wav, long n, int sr, long first_step, long nsteps, mx_tp_step *out) {
  const int S = step_samples(sr), L = oversampling(sr);
  for (long b = first_step; b < first_step + nsteps; ++b) {
    const long end = (b + 1) * S < n ? (b + 1) * S : n;
    mx_tp_step r{0.f, 0.f};
    for (long i = b * S; i < end; ++i) {
      const float p = peak_at(wav, n, i, L), m = sample_magnitude(wav[i]);
      r.true_peak = p > r.true_peak ? p : r.true_peak;
      r.sample_peak = m > r.sample_peak ? m : r.sample_peak;
    }
    out[b - first_step] = r;
  }
}

// the limiter over the whole take: out (n float32), pcm (n int16, may be null)
extern "C" void emu_limit(const float *wav, long n, int sr, float ceiling, int A, float *out, int16_t *pcm) {
  const int L = oversampling(sr);
  // q[j + A] = q_j for j in [-A, n + A): unity outside the file;  m[t + A] = m_t for t in [-A, n)
  std::vector<int32_t> q((size_t)(n + 2L * A), kUnity), m((size_t)(n + A), kUnity);
  for (long j = 0; j < n; ++j) q[(size_t)(j + A)] = required_gain(peak_at(wav, n, j, L), ceiling);
  for (long t = -A; t < n; ++t)
    for (long j = t; j <= t + A; ++j) m[(size_t)(t + A)] = q[(size_t)(j + A)] < m[(size_t)(t + A)] ? q[(size_t)(j + A)] : m[(size_t)(t + A)];
  for (long i = 0; i < n; ++i) {
    int64_t s = 0;
    for (long t = i - A; t <= i; ++t) s += m[(size_t)(t + A)];
    out[i] = limited(wav[i], s, A);
    if (pcm) pcm[i] = mx::pcm16_clamped(out[i]);
  }
}

#ifdef TRUEPEAK_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_truepeak_host.py): the emulation over the smallest shapes, and the
// library's loudness range and export gain (melonix_amd/csrc/loudness_logic.cpp, compiled beside this file) at the edges of
// their lists.
#include <cmath>
#include <cstdio>

#include "../../melonix_amd/csrc/loudness_logic.h"

int main() {
  int bad = 0;
  for (int sr : {8000, 44100, 96000, 192000}) {
    const int S = step_samples(sr);
    for (long n : {1L, 5L, 6L, 7L, (long)S - 1, (long)S, (long)S + 1, 3L * S + 5}) {
      std::vector<float> w((size_t)n);
      for (long i = 0; i < n; ++i) w[(size_t)i] = 1.2f * (float)std::sin(0.9 * (double)i);
      if (n > 2) w[(size_t)(n / 2)] = NAN, w[(size_t)(n - 1)] = INFINITY;
      const long steps = step_count(n, sr);
      std::vector<mx_tp_step> a((size_t)steps), b((size_t)steps);
      emu_true_peak_steps(w.data(), n, sr, 0, steps, a.data());
      for (long s = 0; s < steps; ++s) emu_true_peak_steps(w.data(), n, sr, s, 1, b.data() + s);  // step by step
      for (long s = 0; s < steps; ++s) bad += !(a[(size_t)s].true_peak == b[(size_t)s].true_peak && a[(size_t)s].true_peak >= a[(size_t)s].sample_peak);
      for (int A : {1, 2, 65}) {
        std::vector<float> out((size_t)n);
        std::vector<int16_t> pcm((size_t)n);
        emu_limit(w.data(), n, sr, 0.5f, A, out.data(), pcm.data());
        emu_limit(w.data(), n, sr, 0.5f, A, out.data(), nullptr);
        for (long i = 0; i < n; ++i) bad += std::isfinite(w[(size_t)i]) && !(std::fabs(out[(size_t)i]) <= 0.5f) && !std::isnan(out[(size_t)i]);
      }
    }
  }
  // the loudness range: no records, fewer than one window, exactly one, a partial last step, a NaN energy
  const int S = 480;
  mx_loudness_range_result r;
  mx::loudness_range(nullptr, 0, S, &r);
  bad += !(r.values == 0 && r.gated == 0 && r.lra == 0.0);
  for (long steps : {299L, 300L, 301L, 310L, 650L}) {
    std::vector<mx_loud_step> st((size_t)steps);
    for (long b = 0; b < steps; ++b) st[(size_t)b] = mx_loud_step{(b < 400 ? 1e-2 : 1e-4) * S, 0.5f, S};
    mx::loudness_range(st.data(), steps, S, &r);
    bad += r.values != (steps >= 300 ? (steps - 300) / 10 + 1 : 0) || r.gated != r.values || r.bad != 0;
    st.back().samples = S - 1;
    mx::loudness_range(st.data(), steps, S, &r);
    bad += r.values != (steps - 1 >= 300 ? (steps - 1 - 300) / 10 + 1 : 0);
    st.back().samples = S;
    st[0].energy = NAN;
    mx::loudness_range(st.data(), steps, S, &r);
    bad += r.bad != (steps >= 300 ? 1 : 0);
    if (steps == 650) bad += !(r.lra > 0.0 && r.high_lufs > r.low_lufs);
  }
  bad += !(mx::normalize_amp(-20.0, 0.9, -16.0, -1.0) < 1.0);
  printf(bad ? "truepeak_emu FAILED %d\n" : "truepeak_emu ok\n", bad);
  return bad != 0;
}
#endif
