// onset_core.h — the per-lane arithmetic of the onset-strength kernel (onset_kernels.hip): a 1024-point real transform as a
// complex 512 = 8 x 8 x 8 on ONE wavefront (16 samples, 8 complex points per lane) plus the real-FFT split, the compressed
// magnitudes and the lane's share of the flux.  Plain C++ between the kernel's barriers, no intrinsics: tests/emu/onset_emu.cpp
// runs the same functions lane by lane on the CPU.  Built with -ffp-contract=off: every product and sum rounds as written.
//
// z_n = (w x)[2n] + i (w x)[2n+1], n = 64 n2 + 8 n1 + n0;  Z_k = sum_n z_n W512^{nk}, k = k0 + 8 k1 + 64 k2  (W_N = e^{-2 pi i/N}):
//   pass 1   lane (n1, n0) = 8 n1 + n0 holds n2 = 0..7:  A[k0] = DFT8 over n2, times W64^{n1 k0}
//   pass 2   lane (k0, n0) = 8 k0 + n0 holds n1 = 0..7:  B[k1] = DFT8 over n1, times W512^{n0 (k0 + 8 k1)}
//   pass 3   lane (k1, k0) = 8 k1 + k0 holds n0 = 0..7:  Z[lane + 64 k2] = DFT8 over n0
//   split    2 X_k = (Z_k + conj Z_{512-k}) - i W1024^k (Z_k - conj Z_{512-k}),  k = lane + 64 r
// The two transpositions go through an LDS image of 8 rows of 72 points (64 + 8 of padding: lanes that differ in their upper
// three bits land 8 points = 16 banks apart); the split reads Z_{512-k} from the image in bin order.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_ONSET_HD __host__ __device__ __forceinline__
#define MX_ONSET_UNROLL _Pragma("unroll")
#else
#define MX_ONSET_HD inline
#define MX_ONSET_UNROLL
struct float2 {
  float x, y;
};
#endif

namespace mx {
namespace onset {

constexpr int kN = 1024, kM = 512, kLanes = 64, kRow = 72, kImage = 8 * kRow;  // image: float2[kImage]
constexpr int kMaxLag = 4;
constexpr float kHalfSqrt2 = 0.70710678118654752440f;

MX_ONSET_HD float2 c_mk(float x, float y) {
  float2 r;
  r.x = x;
  r.y = y;
  return r;
}
MX_ONSET_HD float2 c_add(float2 a, float2 b) { return c_mk(a.x + b.x, a.y + b.y); }
MX_ONSET_HD float2 c_sub(float2 a, float2 b) { return c_mk(a.x - b.x, a.y - b.y); }
MX_ONSET_HD float2 c_mul(float2 a, float2 b) { return c_mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
MX_ONSET_HD float2 c_mul_mi(float2 a) { return c_mk(a.y, -a.x); }  // -i a

// a[k] <- sum_j a[j] W8^{jk}: two DFT4 (even, odd) and the W8^k butterflies
MX_ONSET_HD void dft8(float2 (&a)[8]) {
  const float2 s0 = c_add(a[0], a[4]), d0 = c_sub(a[0], a[4]), s1 = c_add(a[2], a[6]), d1 = c_mul_mi(c_sub(a[2], a[6]));
  const float2 e0 = c_add(s0, s1), e2 = c_sub(s0, s1), e1 = c_add(d0, d1), e3 = c_sub(d0, d1);
  const float2 t0 = c_add(a[1], a[5]), u0 = c_sub(a[1], a[5]), t1 = c_add(a[3], a[7]), u1 = c_mul_mi(c_sub(a[3], a[7]));
  const float2 o0 = c_add(t0, t1), q2 = c_sub(t0, t1), q1 = c_add(u0, u1), q3 = c_sub(u0, u1);
  const float2 o1 = c_mk((q1.x + q1.y) * kHalfSqrt2, (q1.y - q1.x) * kHalfSqrt2);   // W8   q1
  const float2 o2 = c_mul_mi(q2);                                                   // W8^2 q2
  const float2 o3 = c_mk((q3.y - q3.x) * kHalfSqrt2, (-q3.x - q3.y) * kHalfSqrt2);  // W8^3 q3
  a[0] = c_add(e0, o0);
  a[4] = c_sub(e0, o0);
  a[1] = c_add(e1, o1);
  a[5] = c_sub(e1, o1);
  a[2] = c_add(e2, o2);
  a[6] = c_sub(e2, o2);
  a[3] = c_add(e3, o3);
  a[7] = c_sub(e3, o3);
}

// What a lane keeps for the whole walk, from the table tw[j] = W1024^j, j < 1024: its 16 window weights (samples
// 128 n2 + 2 lane, + 1), the twiddles behind passes 1 and 2 and those of the split
struct LaneConsts {
  float2 w[8];   // Hann weights of the lane's sample pairs
  float2 t1[8];  // W64^{n1 k0}, k0 = 0..7 (n1 = lane >> 3)
  float2 t2[8];  // W512^{n0 (k0 + 8 k1)}, k1 = 0..7 (k0 = lane >> 3, n0 = lane & 7)
  float2 ts[8];  // W1024^{lane + 64 r}, r = 0..7
};
MX_ONSET_HD void lane_consts(int lane, const float2 *tw, LaneConsts &c) {
  const int lo = lane & 7, hi = lane >> 3;
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int j = 128 * r + 2 * lane;
    c.w[r] = c_mk(0.5f - 0.5f * tw[j].x, 0.5f - 0.5f * tw[j + 1].x);
    c.t1[r] = tw[16 * hi * r];
    c.t2[r] = tw[2 * lo * (hi + 8 * r)];
    c.ts[r] = tw[lane + 64 * r];
  }
}

// pass 1: x = the lane's raw sample pairs (x[r] = audio[128 r + 2 lane], [.. + 1]); leaves A' in the image
MX_ONSET_HD void pass1(int lane, const LaneConsts &c, const float2 (&x)[8], float2 *img) {
  float2 a[8];
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) a[r] = c_mk(x[r].x * c.w[r].x, x[r].y * c.w[r].y);
  dft8(a);
  img[lane] = a[0];
  MX_ONSET_UNROLL
  for (int k = 1; k < 8; ++k) img[lane + kRow * k] = c_mul(a[k], c.t1[k]);
}
// pass 2: reads A' (behind a barrier), returns B' in b; the caller stores it with store2 behind another barrier
MX_ONSET_HD void pass2(int lane, const LaneConsts &c, const float2 *img, float2 (&b)[8]) {
  const int n0 = lane & 7, k0 = lane >> 3;
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) b[r] = img[n0 + 8 * r + kRow * k0];
  dft8(b);
  MX_ONSET_UNROLL
  for (int k = 0; k < 8; ++k) b[k] = c_mul(b[k], c.t2[k]);
}
MX_ONSET_HD void store2(int lane, const float2 (&b)[8], float2 *img) {
  const int n0 = lane & 7, k0 = lane >> 3;
  MX_ONSET_UNROLL
  for (int k = 0; k < 8; ++k) img[k0 + 8 * k + kRow * n0] = b[k];
}
// pass 3: reads B' (behind a barrier), returns Z[lane + 64 r] in z
MX_ONSET_HD void pass3(int lane, const float2 *img, float2 (&z)[8]) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) z[r] = img[lane + kRow * r];
  dft8(z);
}
MX_ONSET_HD void store3(int lane, const float2 (&z)[8], float2 *img) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) img[lane + 64 * r] = z[r];
}
// split + compression: c[r] = log1pf(compress * |X_k| / 512), k = lane + 64 r (bin 0 is computed and never used)
MX_ONSET_HD void compressed(int lane, const LaneConsts &c, const float2 (&z)[8], const float2 *img, float compress, float (&out)[8]) {
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const float2 a = z[r], b = img[(kM - k) & (kM - 1)];
    const float2 e = c_mk(a.x + b.x, a.y - b.y), d = c_mk(a.x - b.x, a.y + b.y);
    const float2 t = c_mul(c.ts[r], d);
    const float re = e.x + t.y, im = e.y - t.x;  // 2 X_k
    const float m = sqrtf(re * re + im * im) * (1.0f / 1024.0f);
    out[r] = log1pf(compress * m);
  }
}
// the lane's share of the flux: bins lane + 64 r in ascending r, those inside [kmin, kmax].  max(0, d) keeps a NaN, as
// np.maximum does: !(d <= 0) is d > 0 for every d that is not NaN (the same additions in the same order), and true for a NaN,
// which then stays in the sum — a frame that could not be measured does not read as "no flux".
MX_ONSET_HD float lane_flux(int lane, const float (&cur)[8], const float (&prev)[8], int kmin, int kmax) {
  float s = 0.f;
  MX_ONSET_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const float d = cur[r] - prev[r];
    if (k >= kmin && k <= kmax && !(d <= 0.f)) s += d;
  }
  return s;
}
// The wavefront's sum, in the order the kernel takes: six exchange steps, lane l adding lane l ^ step's value, step = 32, 16,
// .., 1.  Every lane ends with the same bits (a + b == b + a).  Host form, over an array of the 64 lane values.
inline float wave_sum_host(float (&v)[kLanes]) {
  for (int step = 32; step >= 1; step >>= 1) {
    float n[kLanes];
    for (int l = 0; l < kLanes; ++l) n[l] = v[l] + v[l ^ step];
    for (int l = 0; l < kLanes; ++l) v[l] = n[l];
  }
  return v[0];
}

}  // namespace onset
}  // namespace mx
