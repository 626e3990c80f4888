// denoise_core.h — the per-lane arithmetic of the noise-reduction kernels (denoise_kernels.hip) around onset_core.h's 1024-point
// transform on ONE wavefront: the real-FFT split into the spectrum and its powers, the raw gains, the 1-2-1 smoothing over time
// and frequency, the inverse of the split, the first pass of the inverse transform (the other passes are onset_core.h's: the
// inverse is the forward transform of the conjugate, conjugated), the synthesis window and the overlap-add; and the geometry of
// the output-tile walk.  Plain C++ between the kernel's barriers, no intrinsics: tests/emu/denoise_emu.cpp runs the same functions
// lane by lane on the CPU.  Built with -ffp-contract=off: every product and sum rounds as written.  Definition:
// include/melonix_amd.h "Noise reduction".
//
// With U_k = 2 X_k (what the forward split leaves), M = 512, W = W1024:
//   S = U_k + conj U_{M-k},  D = U_k - conj U_{M-k},  4 Z_k = S + i conj(W^k) D            (k = 0: U_M is bin 512, packed into Z_0)
//   z_n = conj(DFT512(conj(4 Z)))_n / 2048,  y[2n] + i y[2n+1] = z_n
// A lane holds bins lane + 64 r going in and points lane + 64 r = sample pairs 128 r + 2 lane coming out: the layout pass 1 wants
// of its input and the layout the forward transform loads its samples in.
#pragma once
#include "onset_core.h"

namespace mx {
namespace dn {

using namespace onset;

constexpr int kHop = 256, kLead = 3, kBins = kM + 1;  // frame f starts at sample (f - kLead) kHop
constexpr int kMaxPrintFrames = 8192;
constexpr int kMaxRun = 32;                   // output blocks of kHop samples per wavefront
constexpr float kTwoThirds = 0x1.555556p-1f;  // (float)(2 / 3): the four frames' squared windows sum to 3/2
constexpr float kInv2048 = 1.0f / 2048.0f;

// the file's frames and output blocks
MX_ONSET_HD int64_t frames_of(int64_t n) { return (n + kHop - 1) / kHop + kLead; }
MX_ONSET_HD int64_t blocks_of(int64_t n) { return (n + kHop - 1) / kHop; }

// The walk of one wavefront over outputs [first, first + count) of a take: tile `index` owns blocks [b0, b1) of `run` blocks from
// the block of `first` on, synthesises frames b0 .. b1 + 2 (block b is the sum of frames b .. b + 3, and b1 + 2 <= F - 1) and
// analyses frames fa = max(b0 - 1, 0) .. min(b1 + 3, F - 1): the time smoothing wants a frame either side.
struct Tile {
  int64_t b0, b1, fa, F;
};
MX_ONSET_HD int64_t tiles_of(int64_t first, int64_t count, int run) {
  if (count <= 0) return 0;
  const int64_t ba = first / kHop, be = (first + count + kHop - 1) / kHop;
  return (be - ba + run - 1) / run;
}
MX_ONSET_HD Tile tile_of(int64_t first, int64_t count, int64_t n, int64_t index, int run) {
  const int64_t ba = first / kHop, be = (first + count + kHop - 1) / kHop;
  Tile t;
  t.b0 = ba + index * run;
  t.b1 = t.b0 + run < be ? t.b0 + run : be;
  t.fa = t.b0 > 0 ? t.b0 - 1 : 0;
  t.F = frames_of(n);
  return t;
}

// a sample of the padded image as the definition takes it: zeros outside [0, n) whatever the pads hold
MX_ONSET_HD float masked(float v, int64_t s, int64_t n) { return s >= 0 && s < n ? v : 0.f; }

// What a lane keeps of a frame's spectrum: U_k = 2 X_k, k = lane + 64 r, and bin 512 (real; lane 0's is the bin's, the other
// lanes' is never read)
struct Spec {
  float2 u[8];
  float u512;
};
// the split behind onset_core.h's store3, with the powers a = (|X_k| / 512)^2 (sibilant_core.h's scale: 2^-20 of |U|^2)
MX_ONSET_HD void split(int lane, const LaneConsts &c, const float2 (&z)[8], const float2 *img, Spec &s, float (&a)[8], float &a512) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const float2 p = z[r], q = img[(kM - k) & (kM - 1)];
    const float2 e = c_mk(p.x + q.x, p.y - q.y), d = c_mk(p.x - q.x, p.y + q.y);
    const float2 t = c_mul(c.ts[r], d);
    const float re = e.x + t.y, im = e.y - t.x;  // 2 X_k
    s.u[r] = c_mk(re, im);
    a[r] = (re * re + im * im) * (1.0f / 1048576.0f);
    if (r == 0) {  // k = 0 of lane 0: Z_0 = (X_0 + X_512) / 2 + i (X_0 - X_512) / 2
      s.u512 = e.x - t.y;
      a512 = (s.u512 * s.u512) * (1.0f / 1048576.0f);
    }
  }
}

// theta = sens P, g = a > theta ? 1 - theta / a : 0, then at least `floor`: comparisons, so a NaN power gives `floor`
MX_ONSET_HD float raw_gain(float a, float theta, float floor) {
  const float g = a > theta ? 1.f - theta / a : 0.f;
  return g < floor ? floor : g;
}
// the 1-2-1 kernel, over time and over frequency: ((lower + (centre + centre)) + upper) / 4
MX_ONSET_HD float s121(float lo, float c, float hi) { return ((lo + (c + c)) + hi) * 0.25f; }

// The frequency smoothing's exchange.  Row r of lane l is bin l + 64 r; its upper neighbour is row r of lane l + 1, and for lane
// 63 row r + 1 of lane 0 (bin 512 behind row 7); its lower neighbour row r of lane l - 1, and for lane 0 row r - 1 of lane 63.
// So for row r every lane publishes two values: `pub_up`, read by lane (l - 1) & 63, and `pub_dn`, read by lane (l + 1) & 63.
MX_ONSET_HD float pub_up(int lane, const float (&t)[8], float t512, int r) { return lane == 0 ? (r < 7 ? t[r + 1] : t512) : t[r]; }
MX_ONSET_HD float pub_dn(int lane, const float (&t)[8], int r) { return lane == kLanes - 1 ? t[r > 0 ? r - 1 : 0] : t[r]; }
// up[r] = pub_up of lane (l + 1) & 63, dn[r] = pub_dn of lane (l - 1) & 63, t511 = lane 63's t[7]; k is clamped to [0, 512]
MX_ONSET_HD void smooth_bins(int lane, const float (&t)[8], float t512, const float (&up)[8], const float (&dn)[8], float t511,
                             float (&g)[8], float &g512) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) g[r] = s121(lane == 0 && r == 0 ? t[0] : dn[r], t[r], up[r]);
  g512 = s121(t511, t512, t512);
}

// V = G U: the lane's bins into the image in bin order and into v, bin 512 behind them at img[512] (inside the image's padding)
MX_ONSET_HD void scaled(int lane, const Spec &s, const float (&g)[8], float g512, float2 *img, float2 (&v)[8]) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    v[r] = c_mk(g[r] * s.u[r].x, g[r] * s.u[r].y);
    img[lane + 64 * r] = v[r];
  }
  if (lane == 0) img[kM] = c_mk(g512 * s.u512, 0.f);
}
// the inverse of the split (behind a barrier): a[r] = conj(4 Z_k), k = lane + 64 r
MX_ONSET_HD void unsplit(int lane, const LaneConsts &c, const float2 (&v)[8], const float2 *img, float2 (&a)[8]) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const float2 p = v[r], q = img[kM - k];
    const float2 e = c_mk(p.x + q.x, p.y - q.y), d = c_mk(p.x - q.x, p.y + q.y);
    const float2 w = c.ts[r];
    const float2 t = c_mk(w.x * d.x + w.y * d.y, w.x * d.y - w.y * d.x);  // conj(W^k) D
    a[r] = c_mk(e.x - t.y, -(e.y + t.x));
  }
}
// onset_core.h's pass 1 without the window (behind a barrier: unsplit has read the image)
MX_ONSET_HD void ipass1(int lane, const LaneConsts &c, float2 (&a)[8], float2 *img) {
  dft8(a);
  img[lane] = a[0];
  MX_ONSET_UNROLL
  for (int k = 1; k < 8; ++k) img[lane + kRow * k] = c_mul(a[k], c.t1[k]);
}
// behind pass 3: the frame's samples 128 r + 2 lane, + 1: the conjugate, / 2048, times the window, times 2/3
MX_ONSET_HD void windowed(const LaneConsts &c, const float2 (&z)[8], float2 (&y)[8]) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r)
    y[r] = c_mk(((z[r].x * kInv2048) * c.w[r].x) * kTwoThirds, ((-z[r].y * kInv2048) * c.w[r].y) * kTwoThirds);
}

// The overlap-add a lane carries through its walk: while frame f is added, slot j holds block f - 3 + j, its pairs at 2 lane
// (h = 0) and 128 + 2 lane (h = 1).  A block is the sum of its four frames in ascending f from +0.f.
struct Ola {
  float2 s[4][2];
};
MX_ONSET_HD void ola_clear(Ola &o) {
  MX_ONSET_UNROLL
  for (int j = 0; j < 4; ++j) o.s[j][0] = o.s[j][1] = c_mk(0.f, 0.f);
}
MX_ONSET_HD void ola_add(Ola &o, const float2 (&y)[8]) {
  MX_ONSET_UNROLL
  for (int j = 0; j < 4; ++j) {
    o.s[j][0] = c_add(o.s[j][0], y[2 * j]);
    o.s[j][1] = c_add(o.s[j][1], y[2 * j + 1]);
  }
}
// slot 0 is complete and has been stored: the next frame's blocks
MX_ONSET_HD void ola_shift(Ola &o) {
  MX_ONSET_UNROLL
  for (int j = 0; j < 3; ++j) o.s[j][0] = o.s[j + 1][0], o.s[j][1] = o.s[j + 1][1];
  o.s[3][0] = o.s[3][1] = c_mk(0.f, 0.f);
}

}  // namespace dn
}  // namespace mx
