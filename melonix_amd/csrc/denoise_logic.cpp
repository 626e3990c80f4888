// denoise_logic.cpp — see denoise_logic.h.
#include "denoise_logic.h"

#include <cmath>

#include "denoise_core.h"

namespace mx {

const char *denoise_params_error(const mx_denoise_params &p) {
  if (!(p.reduction_db >= 0.f && p.reduction_db <= 60.f)) return "reduction_db outside [0, 60]";
  if (!(p.sensitivity_db >= -12.f && p.sensitivity_db <= 24.f)) return "sensitivity_db outside [-12, 24]";
  return nullptr;
}

const char *noise_print_error(const float *print) {
  for (int k = 0; k < dn::kBins; ++k)
    if (!(print[k] >= 0.f) || !std::isfinite(print[k])) return "a noise print's values must be finite and >= 0";
  return nullptr;
}

DenoiseFactors denoise_factors(const mx_denoise_params &p) {
  DenoiseFactors f;
  f.floor = (float)std::pow(10.0, -(double)p.reduction_db / 20.0);
  f.sens = (float)std::pow(10.0, (double)p.sensitivity_db / 10.0);
  return f;
}

bool noise_region_frames(int64_t n, int64_t begin, int64_t end, int64_t *first_frame, int64_t *count) {
  if (begin < 0 || end < begin || end > n) return false;
  if (end - begin < dn::kN) return false;
  const int64_t f0 = dn::kLead + (begin + dn::kHop - 1) / dn::kHop, f1 = dn::kLead + (end - dn::kN) / dn::kHop;  // first, last
  if (f1 < f0 || f1 - f0 + 1 > dn::kMaxPrintFrames) return false;
  *first_frame = f0;
  *count = f1 - f0 + 1;
  return true;
}

void noise_print_of_rows(const float *rows, int64_t count, float *print) {
  for (int k = 0; k < dn::kBins; ++k) {
    double s = 0.0;
    for (int64_t f = 0; f < count; ++f) s += (double)rows[f * dn::kBins + k];
    print[k] = (float)(s / (double)count);
  }
}

}  // namespace mx
