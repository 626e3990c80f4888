// contour_emu.cpp — the pitch-contour kernels on the CPU: the arithmetic of melonix_amd/csrc/contour_core.h run in the kernels'
// mapping (a smoothing tile with its two rows; the pieces of every statistics tile into slot tile + span; one pass per span
// over its slots), with the tile lengths as arguments so that a test can show the bytes do not depend on them.
// tests/test_contour_host.py compares every byte with tests/contour_ref.py.  With -DCONTOUR_EMU_MAIN it is a stand-alone
// program over the smallest shapes (for the sanitizers).
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared contour_emu.cpp ../../melonix_amd/csrc/contour_logic.cpp -o libcontour_emu.so
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../melonix_amd/csrc/contour_core.h"
#include "../../melonix_amd/csrc/contour_logic.h"

using namespace mx;
using namespace mx::contour;

extern "C" {

void emu_contour_cents(const mx_f0 *track, long count, int sr, float threshold, float rms_floor, int32_t *out) {
  for (long f = 0; f < count; ++f) out[f] = cents_of(track[f], sr, threshold, rms_floor);
}

// spans are not checked (as on the device); tile, stat_tile >= 1.  -1: parameters out of range
int emu_contour_split(const int32_t *cents, long count, const mx_contour_span *spans, long nspans, const mx_contour_params *p0,
                      int tile, int stat_tile, mx_contour_rec *rec, mx_contour_stat *stat) {
  if (!params_ok(*p0)) return -1;
  const mx_contour_params p = params_clamped(*p0);
  const int w = p.half_width;
  // the smoothing kernel, tile by tile
  std::vector<int32_t> c_row((size_t)(tile + 4 * w)), b_row((size_t)(tile + 2 * w));
  for (int64_t t0 = 0; t0 < count; t0 += tile) {
    const int64_t c0 = t0 - 2 * w, b0 = t0 - w;
    for (int i = 0; i < tile + 4 * w; ++i) c_row[(size_t)i] = c0 + i >= 0 && c0 + i < count ? cents[c0 + i] : MX_CONTOUR_NONE;
    for (int i = 0; i < tile + 2 * w; ++i) {
      int64_t lo, hi;
      b_row[(size_t)i] = span_of(spans, nspans, count, b0 + i, lo, hi) >= 0 ? box_mean(c_row.data(), c0, lo, hi, b0 + i, w) : 0;
    }
    for (int t = 0; t < tile && t0 + t < count; ++t) {
      int64_t lo, hi;
      mx_contour_rec r{MX_CONTOUR_NONE, 0};
      if (span_of(spans, nspans, count, t0 + t, lo, hi) >= 0) {
        r.smooth = box_mean(b_row.data(), b0, lo, hi, t0 + t, w);
        r.vib = (int32_t)((int64_t)c_row[(size_t)(t + 2 * w)] - (int64_t)r.smooth);
      }
      rec[t0 + t] = r;
    }
  }
  if (!stat || nspans == 0) return 0;
  // the partial kernel: the pieces of every statistics tile, each into its slot
  const int64_t tiles = (count + stat_tile - 1) / stat_tile;
  const int nl = p.lag_max - p.lag_min + 1;
  std::vector<Partial> part((size_t)(tiles + nspans), Partial{-1, -1, -1, -1});  // (a slot that is read was written)
  std::vector<int64_t> part_r((size_t)(tiles + nspans) * (size_t)nl, -1);
  std::vector<char> written((size_t)(tiles + nspans), 0);
  for (int64_t tl = 0; tl < tiles; ++tl) {
    const int64_t t0 = tl * stat_tile, t1 = t0 + stat_tile < count ? t0 + stat_tile : count;
    for (int64_t s = first_span_beyond(spans, nspans, t0); s < nspans && (int64_t)spans[s].first < t1; ++s) {
      int64_t lo, hi;
      span_frames(spans[s], count, lo, hi);
      const int64_t plo = lo > t0 ? lo : t0, phi = hi < t1 ? hi : t1;
      if (plo >= phi) continue;
      const int64_t slot = slot_of(tl, s);
      if (written[(size_t)slot]) return -2;  // two pieces in one slot
      written[(size_t)slot] = 1;
      Partial a = partial_none();
      for (int64_t f = phi - 1; f >= plo; --f) partial_take(a, rec[f]);  // (some order: here descending)
      part[(size_t)slot] = a;
      for (int L = p.lag_min; L <= top_lag(p, hi - lo); ++L) {
        int64_t acc = 0;
        for (int64_t f = plo; f < phi && f + L < hi; ++f) acc += (int64_t)rec[f].vib * (int64_t)rec[f + L].vib;
        part_r[(size_t)slot * (size_t)nl + (size_t)(L - p.lag_min)] = acc;
      }
    }
  }
  // the final kernel: a span's slots added up, the best lag by the total order, met from the highest lag down
  for (int64_t s = 0; s < nspans; ++s) {
    int64_t lo, hi;
    span_frames(spans[s], count, lo, hi);
    const int64_t F = hi - lo;
    Partial a = partial_none();
    int64_t r = 0;
    int32_t lag = 0;
    if (F > 0) {
      const int64_t tlo = lo / stat_tile, thi = (hi - 1) / stat_tile;
      for (int64_t tl = tlo; tl <= thi; ++tl) {
        if (!written[(size_t)slot_of(tl, s)]) return -3;  // a slot read before it was written
        partial_add(a, part[(size_t)slot_of(tl, s)]);
      }
      for (int L = top_lag(p, F); L >= p.lag_min; --L) {
        int64_t rl = 0;
        for (int64_t tl = tlo; tl <= thi; ++tl) rl += part_r[(size_t)slot_of(tl, s) * (size_t)nl + (size_t)(L - p.lag_min)];
        if (lag_better(rl, L, r, lag)) r = rl, lag = L;
      }
    }
    stat[s] = stat_of(a, F, lag, r);
  }
  return 0;
}

// what the host-pointer entry points refuse before any launch (they need a context; these do not)
int emu_contour_check_params(const mx_contour_params *p) { return params_ok(*p) ? 0 : -1; }
int emu_contour_check_spans(const mx_contour_span *spans, long nspans, long count, const int32_t *cents) {
  return contour_spans_error(spans, nspans, count, cents) ? -1 : 0;
}

}  // extern "C"

#ifdef CONTOUR_EMU_MAIN
int main() {
  // the smallest shapes: arrays of 1, 2 and 300 frames, spans at both ends, every extreme of the parameters, tiles of 1 frame
  long long acc = 0;
  for (long count : {1L, 2L, 300L}) {
    std::vector<int32_t> cents((size_t)count);
    for (long f = 0; f < count; ++f) cents[(size_t)f] = (int32_t)(72000 + (f * 37) % 900 - 450);
    std::vector<mx_contour_span> spans;
    if (count < 3) spans.push_back(mx_contour_span{0, (int32_t)count});
    else spans = {{0, 1}, {1, 140}, {141, 2}, {150, 150}};
    std::vector<mx_contour_rec> rec((size_t)count);
    std::vector<mx_contour_stat> stat(spans.size());
    for (const mx_contour_params p : {mx_contour_params{0, 1, 1}, mx_contour_params{64, 1, 256}, mx_contour_params{23, 15, 63}})
      for (int tile : {1, 7, 256}) {
        if (emu_contour_split(cents.data(), count, spans.data(), (long)spans.size(), &p, tile, tile * 3, rec.data(), stat.data())) return 1;
        for (const mx_contour_stat &s : stat) acc += s.r0 + s.lag + s.sum_smooth;
      }
  }
  mx_f0 r{100, 100.25f, 0.05f, 0.1f};
  int32_t c = 0;
  emu_contour_cents(&r, 1, 48000, 0.15f, 1e-3f, &c);
  std::printf("contour_emu ok: %lld, %d\n", acc, c);
  return 0;
}
#endif
