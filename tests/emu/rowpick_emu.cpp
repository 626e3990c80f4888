// rowpick_emu.cpp — TEST INFRASTRUCTURE: the two pitch picks of the N = 4096 STFT kernel on the CPU, lane by lane, through
// the helpers the kernel instantiates (melonix_amd/csrc/stft_core.h): the transform-side pick (every thread's E bins where
// the post-split leaves them: out_bin, band_mask; then the maximum over the workgroup) and the row-side pick of the ROWPICK
// instantiations (row_pick_key over the four consecutive bins of wave 0's lanes; then the maximum over the wave).
// The rows come from stft_emu.cpp's sliding-window emulation, which this unit includes.
// This is not a product path and is never loaded by melonix_amd.
#include "stft_emu.cpp"

namespace {

struct Rec {
  int bin;
  float mag;
};

Rec record_of(unsigned long long key) {
  Rec r;
  r.bin = 0x7fffffff - (int)(unsigned)(key & 0xffffffffull);
  r.mag = __builtin_bit_cast(float, (unsigned)(key >> 32));
  return r;
}

// a thread's registers mg[o] are the row's element out_bin(t, o): the kernel scatters exactly those floats into the row
template <class C>
Rec transform_side(const float *row, int kmin, int kmax) {
  unsigned long long wg = 0ull;
  for (int t = 0; t < C::T; ++t) {
    const uint32_t bmask = band_mask<C>(t, kmin, kmax);
    unsigned long long best = 0ull;
    for (int o = 0; o < C::E; ++o) {
      const int bin = out_bin<C>(t, o);
      const unsigned v = ((bmask >> o) & 1u) ? 0xffffffffu : 0u;
      const unsigned long long k =
          ((unsigned long long)(__builtin_bit_cast(unsigned, row[bin]) & v) << 32) | ((0x7fffffffu - (unsigned)bin) & v);
      best = k > best ? k : best;
    }
    wg = best > wg ? best : wg;  // wave_max_u64, then the maximum over red[]
  }
  return record_of(wg);
}

Rec row_side(const float *row, int kmin, int kmax) {
  unsigned long long w0 = 0ull;
  for (int tt = 0; tt < 64; ++tt) {  // wave 0: q[0] of lane tt holds bins 4 tt .. 4 tt + 3
    const unsigned long long k = row_pick_key(4 * tt, row[4 * tt], row[4 * tt + 1], row[4 * tt + 2], row[4 * tt + 3], kmin, kmax);
    w0 = k > w0 ? k : w0;
  }
  return record_of(w0);
}

}  // namespace

// rows: count x 2048 magnitudes of the N = 4096 plan; old_recs / new_recs: count records (int32 bin, float mag) each.
// Returns 0, or -1 where the band is not one the host hands to the row-side pick.
extern "C" int emu_rowpick(const float *rows, long count, int kmin, int kmax, void *old_recs, void *new_recs) {
  using C = Plan<4096, 16>;
  if (!(0 <= kmin && kmin <= kmax && kmax < 4 * 64)) return -1;
  for (long f = 0; f < count; ++f) {
    static_cast<Rec *>(old_recs)[f] = transform_side<C>(rows + (size_t)f * C::M, kmin, kmax);
    static_cast<Rec *>(new_recs)[f] = row_side(rows + (size_t)f * C::M, kmin, kmax);
  }
  return 0;
}
