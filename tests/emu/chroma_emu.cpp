// chroma_emu.cpp — the chroma kernel's per-thread functions (melonix_amd/csrc/chroma_core.h behind stft_core.h's Plan<4096,16>
// transform) run thread by thread on the CPU, in the walker's order: a run of consecutive frames per workgroup, the Hann
// table the C-ABI uploads, the three passes and the real-FFT split as chroma_kernels.hip calls them, the magnitudes into the
// padded image, the band maximum, the peak masks, the list in ascending bin order, forty columns walking it front to back.
// And the window sums' term.  tests/test_key_host.py compares both with tests/key_ref.py.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared chroma_emu.cpp -o libchroma_emu.so
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../melonix_amd/csrc/chroma_core.h"
#include "../../melonix_amd/csrc/stft_core.h"
#include "../../melonix_amd/csrc/stft_tables.h"

using namespace mx;
using namespace mx::chroma;

namespace {

using P = Plan<4096, 16>;
constexpr int E = P::E, T = P::T;

// wave_walk.h's root_powers7 (a device-only header): the seven pass-3 twiddles from gamma^{1, 2, 4}, the same four products
void root_powers7(const cpx (&b)[3], cpx *w) {
  w[0] = b[0];
  w[1] = b[1];
  w[3] = b[2];
  w[2] = pk_cmul2(b[1], b[0]);
  w[4] = pk_cmul2(b[2], b[0]);
  w[5] = pk_cmul2(b[2], b[1]);
  w[6] = pk_cmul2(b[2], w[2]);
}

struct Tables {
  std::vector<cpx_h> tw2 = make_tw2<P>(), tw3 = make_tw3<P>(), ub = make_ubase<P>();
  std::vector<float> hann = std::vector<float>((size_t)kN);
  Tables() {
    for (int j = 0; j < kN; ++j) hann[(size_t)j] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)j / (double)kN)) * (1.0f / 2048.0f);
  }
};

// one frame: x points at its first sample
void frame_record(const Tables &tb, const float *x, int kmin, int kmax, float floor_abs, float rel, float bin_hz, float *rec) {
  const cpx *tw2 = reinterpret_cast<const cpx *>(tb.tw2.data()), *tw3 = reinterpret_cast<const cpx *>(tb.tw3.data());
  const cpx *ub = reinterpret_cast<const cpx *>(tb.ub.data());
  std::vector<cpx> img((size_t)P::M), regs((size_t)T * E);
  auto V = [&](int t) -> cpx(&)[E] { return *reinterpret_cast<cpx(*)[E]>(&regs[(size_t)t * E]); };
  for (int t = 0; t < T; ++t) {
    cpx xr[E], Y[E];
    load_raw<P, false>(t, xr, x);
    apply_window<P, 1, false>(t, Y, xr, tb.hann.data());
    pass1<P>(Y, V(t));
  }
  for (int t = 0; t < T; ++t) store_t1<P>(t, V(t), img.data());
  std::vector<cpx> w2all((size_t)T * (P::R2 - 1));
  for (int t = 0; t < T; ++t) load_t1_tw2<P>(t, V(t), img.data(), tw2, *reinterpret_cast<cpx(*)[P::R2 - 1]>(&w2all[(size_t)t * (P::R2 - 1)]));
  for (int t = 0; t < T; ++t) {
    pass2_reg<P>(V(t), *reinterpret_cast<cpx(*)[P::R2 - 1]>(&w2all[(size_t)t * (P::R2 - 1)]));
    store_t2<P>(t, V(t), img.data());
  }
  std::vector<float> mag((size_t)kMagLen, 0.f);
  for (int t = 0; t < T; ++t) {
    load_t2<P>(t, V(t), img.data());
    const int col = t ? t : P::NS3 / 2;
    const cpx w3b[3] = {tw3[0 * P::NS3 + col], tw3[1 * P::NS3 + col], tw3[3 * P::NS3 + col]};
    cpx w3r[P::R3 - 1], lo, hi, u[P::R3], X[E];
    root_powers7(w3b, w3r);
    const bool wave0 = t < 64;
    if (wave0) pass3_reg<P, true>(t, V(t), w3r);
    else pass3_reg<P, false>(t, V(t), w3r);
    post_bases<P>(t, ub, lo, hi);
    PostFly<P, 0>::run(lo, wave0 ? hi : lo, u);
    if (wave0) post_cplx<P, true>(t, V(t), u, X);
    else post_cplx<P, false>(t, V(t), u, X);
    for (int o = 0; o < E; ++o) mag[(size_t)mag_idx(out_bin<P>(t, o))] = sqrtf(X[o].x * X[o].x + X[o].y * X[o].y);
  }
  float mv[T][18];
  uint32_t mbits = 0;
  for (int t = 0; t < T; ++t) {
    for (int j = 0; j < 18; ++j) {
      const int k = 16 * t - 1 + j;
      mv[t][j] = k >= 0 && k < kBins ? mag[(size_t)mag_idx(k)] : 0.f;
    }
    const uint32_t b = band_max_bits(16 * t, mv[t], kmin, kmax);
    mbits = b > mbits ? b : mbits;
  }
  std::vector<Peak> list;
  if (mbits < 0x7f800000u) {
    float band_max;
    std::memcpy(&band_max, &mbits, 4);
    const float thr = threshold_of(floor_abs, rel, band_max);
    for (int t = 0; t < T; ++t) {  // (the scan of the counts puts thread t's peaks behind those of the threads before it)
      uint32_t mask = peak_mask(16 * t, mv[t], kmin, kmax, thr);
      while (mask) {
        const int k = 16 * t + __builtin_ctz(mask);
        mask &= mask - 1;
        list.push_back(peak_of(k, mag[(size_t)mag_idx(k - 1)], mag[(size_t)mag_idx(k)], mag[(size_t)mag_idx(k + 1)], bin_hz));
      }
    }
  }
  for (int col = 0; col < kCols; ++col) {
    float acc = 0.f;
    for (const Peak &q : list) acc += column_term(col, q);
    rec[col] = acc;
  }
}

}  // namespace

extern "C" long emu_chroma(const float *wav, long n, int sr, int hop, long first_frame, long count, int kmin, int kmax, float floor_abs,
                           float rel, int run, float *out) {
  static const Tables tb;
  const long pad = 32768;
  std::vector<float> padded((size_t)(n + 2 * pad), 0.f);
  std::memcpy(padded.data() + pad, wav, sizeof(float) * (size_t)n);
  const float bin_hz = (float)sr / (float)kN;
  long most = 0;
  for (long f0 = 0; f0 < count; f0 += run) {
    const long f1 = f0 + run < count ? f0 + run : count;
    for (long f = f0; f < f1; ++f) {
      frame_record(tb, padded.data() + pad - kBins + (first_frame + f) * (long)hop, kmin, kmax, floor_abs, rel, bin_hz, out + f * kCols);
      most = (long)out[f * kCols + 39] > most ? (long)out[f * kCols + 39] : most;
    }
  }
  return most;  // the largest number of peaks a frame had (<= kMaxPeaks)
}

extern "C" void emu_chroma_sum(const float *rec, long first, long frames, double *out40) {
  for (int col = 0; col < kCols; ++col) {
    double acc = 0.0;
    for (long f = first; f < first + frames; ++f) acc += sum_term(rec[f * kCols + col]);
    out40[col] = acc;
  }
}

#ifdef CHROMA_EMU_MAIN
// The stand-alone form (AddressSanitizer + UBSan, tests/test_key_host.py): the emulation and the library's host logic
// (melonix_amd/csrc/key_logic.cpp and f0_notes.cpp, compiled beside this file) over the smallest shapes and the edges.
#include <cstdio>

#include "../../melonix_amd/csrc/key_logic.h"

int main() {
  int bad = 0;
  for (long n : {1L, 4095L, 4097L, 9000L}) {
    std::vector<float> w((size_t)n);
    for (long i = 0; i < n; ++i) w[(size_t)i] = 0.3f * (float)std::sin(0.0576 * (double)i) + 0.1f * (float)std::sin(1.9 * (double)i) * (i % 3 ? 1.f : -1.f);
    for (int hop : {1, 255, 2048, 16384}) {
      const long frames = std::min<long>((n + hop - 1) / hop, 12);
      std::vector<float> a((size_t)frames * kCols), b((size_t)frames * kCols);
      const long most = emu_chroma(w.data(), n, 48000, hop, 0, frames, 9, 426, 1e-4f, 0.05f, 1, a.data());
      emu_chroma(w.data(), n, 48000, hop, 0, frames, 9, 426, 1e-4f, 0.05f, 5, b.data());
      bad += most > kMaxPeaks || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0;
      for (float v : a) bad += !std::isfinite(v);
    }
  }
  {  // every other bin a peak: the widest band, no floor — the list at its longest
    std::vector<float> w(8192);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u >> 8) & 0xffff) / 65536.f - 0.5f;
    w[100] = INFINITY;
    std::vector<float> a(4 * kCols);
    bad += emu_chroma(w.data(), 8192, 48000, 2048, 0, 4, 2, 2046, 0.f, 0.f, 8, a.data()) > kMaxPeaks;
    for (int c = 0; c < kCols; ++c) bad += a[(size_t)c] != 0.f;  // frame 0 holds the Inf
    bad += !(a[3 * kCols + 39] > 100.f);
    double s[kCols];
    a[kCols + 3] = NAN;
    emu_chroma_sum(a.data(), 0, 4, s);
    for (double v : s) bad += !std::isfinite(v);
    const mx_key k = key_from_sum(s);
    bad += k.tonic < 0 || k.tonic > 11 || !std::isfinite(k.clarity);
  }
  const double zeros[kCols] = {};
  bad += key_from_sum(zeros).scale_mask != 0 || key_from_notes(nullptr, 0).scale_mask != 0;
  const mx_note notes[] = {{0, 100, 0, 10, 51.2, 0.f, 0.f}, {50, 150, 5, 10, 58.2, 0.f, 0.f}, {200, 300, 20, 0, -13.5, 0.f, 0.f}};
  const mx_key k = key_from_notes(notes, 3);
  bad += !(std::fabs(k.tuning_cents - 20.0) < 1e-9);
  bad += key_windows(10, 4, 3).size() != 4 || !key_windows(10, 0, 1).empty() || !key_windows(0, 4, 1).empty();
  mx_marker m[6];
  correction_markers_tuned(notes, 3, 1.0, k.scale_mask, k.tuning_cents, m);
  bad += !(std::fabs(m[0].pitchBend) < 1e-9);
  printf(bad ? "chroma_emu FAILED %d\n" : "chroma_emu ok\n", bad);
  return bad != 0;
}
#endif
