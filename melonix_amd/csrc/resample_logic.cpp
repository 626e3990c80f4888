// resample_logic.cpp — the tap table of the sample-rate conversion (see resample_logic.h), expression by expression what
// include/melonix_amd.h "Sample-rate conversion" and tests/resample_ref.py write.
#include "resample_logic.h"

#include <cmath>
#include <vector>

#include "resample_core.h"

namespace mx {

double resample_bessel_i0(double x) {
  const double half = x / 2.0;
  double q = 1.0, sum = 1.0;  // q = (x / 2)^k / k!
  for (int k = 1; k < 1000; ++k) {
    q = q * half / (double)k;
    const double term = q * q;
    sum = sum + term;
    if (term < sum * 0x1p-60) break;
  }
  return sum;
}

void resample_table(const mx_resample_plan &p, float *out) {
  const double pi = 3.141592653589793;
  const int L = p.L, T = p.taps, H = p.half;
  const double s = p.L < p.M ? (double)p.L / (double)p.M : 1.0;
  const double beta = (double)rs::kKaiserBeta, i0_beta = resample_bessel_i0(beta);
  std::vector<double> row((size_t)T);
  for (int phi = 0; phi < L; ++phi) {
    float *h = out + (size_t)phi * T;
    if (s == 1.0 && phi == 0) {  // the output falls on an input sample: that sample
      for (int k = 0; k < T; ++k) h[k] = k == H - 1 ? 1.f : 0.f;
      continue;
    }
    double sum = 0.0;
    for (int k = 0; k < T; ++k) {
      const double u = (double)(k - (H - 1)) - (double)phi / (double)L;
      const double v = s * u, t = u / (double)H;
      const double sinc = v == 0.0 ? 1.0 : std::sin(pi * v) / (pi * v);
      double a = 1.0 - t * t;
      if (a < 0.0) a = 0.0;
      const double w = resample_bessel_i0(beta * std::sqrt(a)) / i0_beta;
      row[(size_t)k] = s * sinc * w;
      sum = sum + row[(size_t)k];
    }
    for (int k = 0; k < T; ++k) h[k] = (float)(row[(size_t)k] / sum);
  }
}

void resample_table_by_tap(const mx_resample_plan &p, float *out) {
  std::vector<float> rows((size_t)p.L * p.taps);
  resample_table(p, rows.data());
  for (int phi = 0; phi < p.L; ++phi)
    for (int k = 0; k < p.taps; ++k) out[(size_t)k * p.L + phi] = rows[(size_t)phi * p.taps + k];
}

}  // namespace mx
