// tests/cpp/work_memory_host.cpp — the host side of the context's work memory and of the job-list calls, on the CPU under
// AddressSanitizer + UBSan + LeakSanitizer (tests/test_work_memory_host.py builds and runs it): capi_tempo.cpp, capi_key.cpp,
// capi_contour.cpp and capi_ctx.cpp linked over the fake of the HIP calls below and kernel launches that do nothing.
// The fake defers every copy to the next synchronise, as a stream does, so a call that returned with a copy of the caller's
// memory still queued is caught; "device" memory is zeroed host memory.  The k-th HIP call (launches included) fails for every k,
// at 1 job and at 300: each faulted call must return a negative status with a message, leave no copy queued and nothing
// allocated in the set whose buffer could not be had, and succeed when repeated.
#include <cstdio>
#include <functional>
#include <set>
#include <vector>

#include "../../melonix_amd/csrc/capi_internal.h"
#include "../../melonix_amd/csrc/chroma_core.h"
#include "../../melonix_amd/csrc/contour_core.h"
#include "../../melonix_amd/csrc/tempo_core.h"

namespace {
long g_calls = 0, g_fail_at = 0;
bool g_fired = false;
const void *g_refused = nullptr;  // where the refused hipMalloc would have put its pointer
std::set<void *> g_live;
std::vector<std::function<void()>> g_queue;
int g_stream_tag;

bool refuse() {
  if (++g_calls != g_fail_at) return false;
  g_fired = true;
  return true;
}
void drain() {
  for (auto &op : g_queue) op();
  g_queue.clear();
}
hipError_t launch() { return refuse() ? hipErrorLaunchFailure : hipSuccess; }
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) {
  if (refuse()) {
    g_refused = p;
    return hipErrorOutOfMemory;
  }
  *p = calloc(n ? n : 1, 1);
  g_live.insert(*p);
  return hipSuccess;
}
hipError_t hipFree(void *p) {  // (frees behind the stream, as the runtime does; never refused: the library ignores its status)
  drain();
  if (p && !g_live.erase(p)) {
    fprintf(stderr, "hipFree of %p, which is not allocated\n", p);
    abort();
  }
  free(p);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) {
  if (refuse()) return hipErrorUnknown;
  g_queue.push_back([=] { memcpy(dst, src, n); });
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t) {
  if (refuse()) return hipErrorUnknown;
  g_queue.push_back([=] { memset(dst, v, n); });
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
  if (refuse()) return hipErrorUnknown;
  drain();
  memcpy(dst, src, n);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {  // (a refused one has still waited: what was queued is done; an idle stream has no
  if (g_queue.empty()) return hipSuccess;       // error to report — the wait before a DeviceArray is freed, whose status nobody reads)
  drain();
  return refuse() ? hipErrorUnknown : hipSuccess;
}
hipError_t hipSetDevice(int) { return refuse() ? hipErrorInvalidDevice : hipSuccess; }
hipError_t hipGetDeviceCount(int *n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t *prop, int) {
  memset(prop, 0, sizeof *prop);
  strcpy(prop->gcnArchName, "gfx950");
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  *s = reinterpret_cast<hipStream_t>(&g_stream_tag);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
  *p = malloc(n);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *p) {
  free(p);
  return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (fake)" : "refused (fake)"; }

// what the units under test call of the rest of the library
int mx_onset_flux_dev(mx_ctx *, const mx_audio *, int, int, int64_t, int64_t, const mx_onset_flux_params *, float *) {
  return launch() == hipSuccess ? MX_OK : mx::fail(MX_ERR_DEVICE, "flux launch refused (fake)");
}
void mx_pitch_band(int, int, int *kmin, int *kmax) { *kmin = 8, *kmax = 160; }
}

namespace mx {
int stft_frames_per_block_cap(int, int, int) { return 16; }
void pv_release(mx_ctx *) {}
hipError_t launch_stft(int, int, const StftArgs &, hipStream_t) { return launch(); }
// (the one launch that does something: a smoothed curve of zeros would end the estimate before its comb jobs)
hipError_t launch_tempo_smooth(const float *in, int64_t count, int, const tempo::SmoothWeights &, float *out, hipStream_t) {
  if (launch() != hipSuccess) return hipErrorLaunchFailure;
  g_queue.push_back([=] { memcpy(out, in, (size_t)count * sizeof(float)); });
  return hipSuccess;
}
hipError_t launch_tempo_comb(const float *, int64_t, const mx_comb_job *, int64_t, mx_comb *, hipStream_t) { return launch(); }
hipError_t launch_chroma(const ChromaArgs &, hipStream_t) { return launch(); }
hipError_t launch_chroma_sum(const mx_chroma_rec *, int64_t, const mx_chroma_job *, int64_t, double *, hipStream_t) { return launch(); }
hipError_t launch_contour_cents(const mx_f0 *, int64_t, int, float, float, int32_t *, hipStream_t) { return launch(); }
size_t contour_part_bytes(int64_t count, int64_t nspans, const mx_contour_params &) { return (size_t)(count + nspans) * 8; }
hipError_t launch_contour_split(const int32_t *, int64_t, const mx_contour_span *, int64_t, const mx_contour_params &, mx_contour_rec *,
                                mx_contour_stat *, void *, hipStream_t) {
  return launch();
}
}  // namespace mx

namespace {
int g_failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++g_failed;                                          \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

// every k: the k-th HIP call of `call` refused, on a context that keeps no work memory (so every buffer has to be had anew)
void sweep(mx_ctx *ctx, const char *name, int64_t njobs, const std::function<int()> &call) {
  CHECK(call() == MX_OK, "%s (%lld jobs): the unfaulted call fails: %s", name, (long long)njobs, mx_last_error());
  long k = 1;
  for (;; ++k) {
    CHECK(mx_ctx_release_scratch(ctx) == MX_OK, "release: %s", mx_last_error());
    g_calls = 0, g_fail_at = k, g_fired = false, g_refused = nullptr;
    const int rc = call();
    g_fail_at = 0;
    if (!g_fired) {
      CHECK(rc == MX_OK, "%s: the unfaulted repeat fails: %s", name, mx_last_error());
      break;
    }
    CHECK(rc < 0 && mx_last_error()[0], "%s: HIP call %ld refused and the call returns %d", name, k, rc);
    CHECK(g_queue.empty(), "%s: HIP call %ld refused and the call returned with %zu copies queued", name, k, g_queue.size());
    if (g_refused)  // (a buffer of a set: the audio handle's and the tables' are not kept work memory)
      mx::for_each_work(ctx, [&](auto &set) {
        if (g_refused < (const void *)&set || g_refused >= (const void *)(&set + 1)) return;
        CHECK(rc == MX_ERR_NOMEM, "%s: a refused buffer of a set gives %d", name, rc);
        for (const mx::GrowBuf &b : set.buf) CHECK(!b.p && !b.cap, "%s: HIP call %ld: the set that failed keeps %zu bytes", name, k, b.cap);
      });
    g_queue.clear();
  }
  CHECK(call() == MX_OK, "%s: after the sweep the call fails: %s", name, mx_last_error());
  printf("  %-36s %4lld jobs: %3ld HIP calls refused one by one\n", name, (long long)njobs, k - 1);
}
}  // namespace

int main() {
  mx_ctx *ctx = nullptr;
  CHECK(mx_ctx_create(0, &ctx) == MX_OK, "context: %s", mx_last_error());
  if (!ctx) return 1;
  const int sr = 48000, hop = 256;
  {  // no jobs: MX_OK and not one HIP call, whatever the records
    const std::vector<mx_chroma_rec> rec(32);
    const std::vector<float> curve(64, 1.f);
    g_calls = 0;
    CHECK(mx_chroma_sum(ctx, rec.data(), 32, nullptr, 0, nullptr) == MX_OK && mx_tempo_comb(ctx, curve.data(), 64, nullptr, 0, nullptr) == MX_OK,
          "a call without jobs fails: %s", mx_last_error());
    CHECK(g_calls == 0, "calls without jobs made %ld HIP calls", g_calls);
  }
  for (const int64_t njobs : {(int64_t)1, (int64_t)300}) {
    // every input lives for one call only: a copy that outlives its call reads freed memory
    sweep(ctx, "mx_tempo_smooth", njobs, [&] {
      std::vector<float> flux(64 * (size_t)njobs, 1.f), out(flux.size());
      return mx_tempo_smooth(ctx, flux.data(), (int64_t)flux.size(), 4, out.data());
    });
    sweep(ctx, "mx_tempo_comb", njobs, [&] {
      std::vector<float> curve(64, 1.f);
      std::vector<mx_comb_job> jobs((size_t)njobs, mx_comb_job{0, 64, 3u << 16});
      std::vector<mx_comb> out((size_t)njobs);
      return mx_tempo_comb(ctx, curve.data(), 64, jobs.data(), njobs, out.data());
    });
    sweep(ctx, "mx_chroma_sum", njobs, [&] {
      std::vector<mx_chroma_rec> rec(32);
      std::vector<mx_chroma_job> jobs((size_t)njobs, mx_chroma_job{3, 20});
      std::vector<double> out((size_t)njobs * 40);
      return mx_chroma_sum(ctx, rec.data(), 32, jobs.data(), njobs, out.data());
    });
    sweep(ctx, "mx_chroma_sum (no records)", njobs, [&] {
      std::vector<mx_chroma_job> jobs((size_t)njobs, mx_chroma_job{0, 0});
      std::vector<double> out((size_t)njobs * 40);
      return mx_chroma_sum(ctx, nullptr, 0, jobs.data(), njobs, out.data());
    });
    const mx_contour_params cp{2, 1, 4};
    for (const bool want_rec : {true, false})
      sweep(ctx, want_rec ? "mx_contour_split" : "mx_contour_split (statistics)", njobs, [&] {
        std::vector<int32_t> cents(600, 96000);
        std::vector<mx_contour_span> spans((size_t)njobs);
        for (int64_t i = 0; i < njobs; ++i) spans[(size_t)i] = mx_contour_span{(int32_t)(2 * i), 2};
        std::vector<mx_contour_rec> rec(600);
        std::vector<mx_contour_stat> stat((size_t)njobs);
        return mx_contour_split(ctx, cents.data(), 600, spans.data(), njobs, &cp, want_rec ? rec.data() : nullptr, stat.data());
      });
    sweep(ctx, "mx_pitch_contour", njobs, [&] {
      std::vector<mx_f0> track(600, mx_f0{218, 218.18f, 0.05f, 0.1f});
      std::vector<mx_note> notes((size_t)njobs);
      for (int64_t i = 0; i < njobs; ++i) notes[(size_t)i] = mx_note{(int32_t)(2 * i * hop), (int32_t)((2 * i + 1) * hop), (int32_t)(2 * i), 2, 60., 0.f, 0.f};
      std::vector<mx_contour_rec> rec(600);
      std::vector<mx_contour_stat> stat((size_t)njobs);
      return mx_pitch_contour(ctx, track.data(), 600, sr, hop, 0, notes.data(), njobs, 0.15f, 1e-3f, nullptr, rec.data(), stat.data());
    });
    // key detection: the take alone (1 job), or 300 windows of up to two frames and the take
    sweep(ctx, "mx_key_detect", njobs, [&] {
      std::vector<float> wav((size_t)(300 * hop), 0.25f);
      mx_audio *a = nullptr;
      int rc = mx_audio_upload(ctx, wav.data(), (int64_t)wav.size(), &a);
      mx_key key{};
      mx_key_window *win = nullptr;
      int64_t nwin = 0;
      if (rc == MX_OK) rc = njobs == 1 ? mx_key_detect(ctx, a, sr, hop, nullptr, 0, 1, &key, nullptr, nullptr)
                                       : mx_key_detect(ctx, a, sr, hop, nullptr, 2, 1, &key, &win, &nwin);
      if (rc == MX_OK && njobs > 1) CHECK(nwin == 300, "mx_key_detect: %lld windows", (long long)nwin);
      mx_free(win);
      const long at = g_fail_at;
      g_fail_at = 0;  // (freeing the audio is not the subject)
      mx_audio_free(ctx, a);
      g_fail_at = at;
      return rc;
    });
  }
  // the estimates make their own job lists (the coarse pass: hundreds of jobs; the refinement: 25 per level)
  std::vector<float> pulse(4096, 0.1f);
  for (size_t f = 0; f < pulse.size(); f += 94) pulse[f] = 5.f;
  sweep(ctx, "mx_tempo_from_flux (windows)", 0, [&] {
    const std::vector<float> flux(pulse);
    mx_tempo t{};
    mx_tempo_window *win = nullptr;
    int64_t nwin = 0;
    const int rc = mx_tempo_from_flux(ctx, flux.data(), (int64_t)flux.size(), sr, hop, 0, nullptr, &t, &win, &nwin);
    mx_free(win);
    return rc;
  });
  sweep(ctx, "mx_tempo_detect", 0, [&] {
    std::vector<float> wav((size_t)(4096 * hop), 0.25f);
    mx_audio *a = nullptr;
    int rc = mx_audio_upload(ctx, wav.data(), (int64_t)wav.size(), &a);
    mx_tempo t{};
    if (rc == MX_OK) rc = mx_tempo_detect(ctx, a, sr, hop, nullptr, nullptr, &t, nullptr, nullptr);
    const long at = g_fail_at;
    g_fail_at = 0;
    mx_audio_free(ctx, a);
    g_fail_at = at;
    return rc;
  });
  // release gives every set back; what stays is the context's tables, and nothing once it is destroyed
  CHECK(mx_ctx_release_scratch(ctx) == MX_OK, "release: %s", mx_last_error());
  mx::for_each_work(ctx, [&](auto &set) {
    for (const mx::GrowBuf &b : set.buf) CHECK(!b.p, "a set keeps %zu bytes behind mx_ctx_release_scratch", b.cap);
  });
  mx_ctx_destroy(ctx);
  CHECK(g_live.empty(), "%zu device allocations outlive the context", g_live.size());
  printf("work_memory_host: %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
