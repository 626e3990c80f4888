// pcm16_emu.cpp — melonix_amd/csrc/pcm16.h compiled for the host: both conversions over arrays, and over runs of consecutive
// binary32 bit patterns (tests/test_pcm16_host.py walks all 2^32 of them).
#include <cstdint>
#include <cstring>

#include "../../melonix_amd/csrc/pcm16.h"

extern "C" {

void emu_pcm16_reference(const float *v, long n, int16_t *out) {
  for (long i = 0; i < n; ++i) out[i] = mx::pcm16_reference(v[i]);
}

void emu_pcm16_clamped(const float *v, long n, int16_t *out) {
  for (long i = 0; i < n; ++i) out[i] = mx::pcm16_clamped(v[i]);
}

// v[i] = the float whose bits are first + i; both conversions of it
void emu_pcm16_patterns(uint32_t first, long n, float *v, int16_t *reference, int16_t *clamped) {
  for (long i = 0; i < n; ++i) {
    const uint32_t bits = first + (uint32_t)i;
    float x;
    std::memcpy(&x, &bits, 4);
    v[i] = x;
    reference[i] = mx::pcm16_reference(x);
    clamped[i] = mx::pcm16_clamped(x);
  }
}

}  // extern "C"
