// tests/cpp/fault_sweep.cpp — allocation-fault sweep over the C-ABI (SURVEY 8b "Errors": the reference's
// callers get empty results, never exceptions — an exception that crossed extern "C" would std::terminate the editor).
//
// This executable REPLACES the global operator new: the k-th allocation made while an entry point of the SHIPPED
// libmelonix_amd.so runs fails (std::bad_alloc, or nullptr for the nothrow forms), for k = 1, 2, ... until a call gets
// through without reaching its k-th allocation.  Every faulted call must come back — the process survives —, with a negative
// status and a message in mx_last_error(), and leave its outputs alone; afterwards the same call, unfaulted, must succeed and
// return what it returned before the sweep (the library's state survived: half-built tables, locked mutexes, a staged job).
// Under -fsanitize=address (the CPU suite builds it so) LeakSanitizer checks that nothing allocated on the way to the
// fault is lost.
//
//   fault_sweep host      the entry points that need no device (time maps, grains, schedules, the PV plan, the WAV writer)
//   fault_sweep host-malloc / device-malloc   (built with -DSWEEP_MALLOC, no sanitizer) the same sweeps with the faults in the
//                         library's own malloc() calls — the arrays it hands out for mx_free — instead of operator new
//   fault_sweep device    ... and those that do (context, audio, STFT in all modes, kept rows, grain table, resynthesis,
//                         export, phase vocoder incl. the three rank stages, pyramid, f0 and its decode, tempo, chroma and key,
//                         pitch contour, the mastering chain, the take processors — sample-rate conversion, noise reduction,
//                         compressor: range forms, print, gain curve and derived audio, the last also on a context of their
//                         own per call, first-use tables included): only allocations made FROM the
//                         library's own code are faulted there (the HIP runtime beneath it is not the subject)
#include <dlfcn.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "melonix_amd.h"

// ---- the faulting allocator --------------------------------------------------------------------------------------------------
namespace {
thread_local bool g_in_call = false;   // an entry point of the library is running on this thread
thread_local long g_fail_at = 0;       // fail the g_fail_at-th eligible allocation of the call (0: none)
thread_local long g_seen = 0;          // eligible allocations of the call so far
thread_local bool g_fired = false;
bool g_only_library_callers = false;   // device mode: only allocations whose caller is code of libmelonix_amd.so
bool g_fault_malloc = false;           // "malloc" modes: the faults go into the library's own malloc() calls instead of operator new

bool from_library(void *ret) {
  Dl_info info;
  return dladdr(ret, &info) && info.dli_fname && strstr(info.dli_fname, "libmelonix_amd");
}
bool should_fail(void *ret, bool is_malloc = false) {
  if (!g_in_call || g_fail_at <= 0 || g_fired || is_malloc != g_fault_malloc) return false;
  if (is_malloc) {  // the library's own output arrays (mx_free'd by the caller): only calls made from its code
    const bool was = g_in_call;
    g_in_call = false;
    const bool lib = from_library(ret);
    g_in_call = was;
    if (!lib) return false;
  }
  if (g_only_library_callers) {
    const bool was = g_in_call;
    g_in_call = false;  // (dladdr may allocate)
    const bool lib = from_library(ret);
    g_in_call = was;
    if (!lib) return false;
  }
  if (++g_seen == g_fail_at) {
    g_fired = true;
    return true;
  }
  return false;
}
void *take(std::size_t n, std::size_t align) {
  if (n == 0) n = 1;
  if (align <= alignof(max_align_t)) return std::malloc(n);
  void *p = nullptr;
  return posix_memalign(&p, align, n) == 0 ? p : nullptr;
}
}  // namespace

void *operator new(std::size_t n) {
  if (should_fail(__builtin_return_address(0))) throw std::bad_alloc();
  void *p = take(n, 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void *operator new[](std::size_t n) {
  if (should_fail(__builtin_return_address(0))) throw std::bad_alloc();
  void *p = take(n, 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void *operator new(std::size_t n, const std::nothrow_t &) noexcept { return should_fail(__builtin_return_address(0)) ? nullptr : take(n, 1); }
void *operator new[](std::size_t n, const std::nothrow_t &) noexcept { return should_fail(__builtin_return_address(0)) ? nullptr : take(n, 1); }
void *operator new(std::size_t n, std::align_val_t a) {
  if (should_fail(__builtin_return_address(0))) throw std::bad_alloc();
  void *p = take(n, (std::size_t)a);
  if (!p) throw std::bad_alloc();
  return p;
}
void *operator new[](std::size_t n, std::align_val_t a) {
  if (should_fail(__builtin_return_address(0))) throw std::bad_alloc();
  void *p = take(n, (std::size_t)a);
  if (!p) throw std::bad_alloc();
  return p;
}
void operator delete(void *p) noexcept { std::free(p); }
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete(void *p, std::size_t) noexcept { std::free(p); }
void operator delete[](void *p, std::size_t) noexcept { std::free(p); }
void operator delete(void *p, std::align_val_t) noexcept { std::free(p); }
void operator delete[](void *p, std::align_val_t) noexcept { std::free(p); }
void operator delete(void *p, std::size_t, std::align_val_t) noexcept { std::free(p); }
void operator delete[](void *p, std::size_t, std::align_val_t) noexcept { std::free(p); }
void operator delete(void *p, const std::nothrow_t &) noexcept { std::free(p); }
void operator delete[](void *p, const std::nothrow_t &) noexcept { std::free(p); }

#ifdef SWEEP_MALLOC
// (a build without sanitizers: malloc itself is replaced — glibc keeps the real one reachable as __libc_malloc)
extern "C" {
void *__libc_malloc(size_t);
void *malloc(size_t n) {
  if (should_fail(__builtin_return_address(0), true)) return nullptr;
  return __libc_malloc(n);
}
}
#endif

// ---- the sweep -----------------------------------------------------------------------------------------------------------------
namespace {
int g_failed_checks = 0;
long g_total_faults = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++g_failed_checks;                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);              \
      fprintf(stderr, "\n");                     \
    }                                            \
  } while (0)

// One entry point under test.  call(): runs it and returns its status (< 0: error) plus a checksum of what it produced —
// it must itself release whatever the library handed out; after a FAILED call it checks that the outputs were left alone.
struct Result {
  long status;
  uint64_t sum;
};
uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

void sweep(const char *name, const std::function<Result()> &call, long max_k = 4000) {
  const Result base = call();
  CHECK(base.status >= 0, "%s: the unfaulted call fails: %ld (%s)", name, base.status, mx_last_error());
  long k = 1, faults = 0;
  for (; k <= max_k; ++k) {
    g_fail_at = k;
    g_seen = 0;
    g_fired = false;
    g_in_call = true;
    const Result r = call();
    g_in_call = false;
    g_fail_at = 0;
    if (!g_fired) {  // the call makes fewer than k allocations: every one of them has been failed once
      CHECK(r.status >= 0 && r.sum == base.sum, "%s: unfaulted repeat differs (status %ld)", name, r.status);
      break;
    }
    ++faults;
    const char *msg = mx_last_error();
    CHECK(r.status < 0, "%s: allocation %ld failed and the call reports success (%ld)", name, k, r.status);
    CHECK(msg && msg[0], "%s: allocation %ld failed and mx_last_error() is empty", name, k);
  }
  CHECK(k <= max_k, "%s: more than %ld allocations in one call", name, max_k);
  const Result again = call();
  CHECK(again.status >= 0 && again.sum == base.sum, "%s: after the sweep the call returns %ld / another result (%s)", name, again.status,
        again.status < 0 ? mx_last_error() : "");
  g_total_faults += faults;
  printf("  %-28s %4ld allocation(s) failed one by one: status < 0 + message each time, result intact afterwards\n", name, faults);
}

std::vector<float> make_sweep(int64_t n, int sr = 48000) {
  std::vector<float> w((size_t)n);
  double ph = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    ph += 2.0 * M_PI * (110.0 + (1760.0 - 110.0) * (double)i / (double)n) / sr;
    w[(size_t)i] = (float)(0.5 * std::sin(ph));
  }
  return w;
}

void host_entries() {
  const int sr = 48000;
  const int64_t n = 2 * sr;
  const std::vector<float> w = make_sweep(n);
  const std::vector<mx_marker> mk = {{1000, 0., 0.0, 2.0}, {30000, 0., -0.2, -3.0}, {60000, 0., 0.3, 5.0}, {(int32_t)n - 1, 0., 0., 0.}};
  const mx_marker *m = mk.data();
  const int nm = (int)mk.size();
  printf("host entry points (no device):\n");
  // the time maps return values, not statuses: NaN (double / float) or MX_ERR_NOMEM (int) with the message set
  sweep("mx_sample2time", [&]() -> Result {
    const double v = mx_sample2time(m, nm, sr, 40000);
    return {std::isnan(v) ? -1 : 0, fnv(&v, sizeof v)};
  });
  sweep("mx_time2sample", [&]() -> Result {
    const int v = mx_time2sample(m, nm, sr, 0.9);
    return {v < 0 ? v : 0, (uint64_t)(int64_t)v};
  });
  sweep("mx_duration", [&]() -> Result {
    const double v = mx_duration(m, nm, sr, n);
    return {std::isnan(v) ? -1 : 0, fnv(&v, sizeof v)};
  });
  sweep("mx_time2pitchbend", [&]() -> Result {
    const float v = mx_time2pitchbend(m, nm, sr, n, 0.7);
    return {std::isnan(v) ? -1 : 0, fnv(&v, sizeof v)};
  });
  sweep("mx_column_range", [&]() -> Result {
    int key = -77, s = -77, e = -77;
    mx_column_range(m, nm, sr, 1.0, 1280, 10.0, &key, &s, &e);
    const bool untouched = key == -77 && s == -77 && e == -77;
    int v[3] = {key, s, e};
    return {untouched ? -1 : 0, fnv(v, sizeof v)};
  });
  int32_t *gs = nullptr, *gl = nullptr;
  int64_t ng = 0;
  sweep("mx_grains", [&]() -> Result {
    int32_t *s = nullptr, *l = nullptr;
    int64_t c = -5;
    const int rc = mx_grains(w.data(), n, &s, &l, &c);
    if (rc < 0) {
      CHECK(s == nullptr && l == nullptr, "mx_grains: outputs set on failure");
      return {rc, 0};
    }
    uint64_t h = fnv(s, (size_t)c * 4);
    h = fnv(l, (size_t)c * 4, h);
    mx_free(s);
    mx_free(l);
    return {rc, h};
  });
  CHECK(mx_grains(w.data(), n, &gs, &gl, &ng) == MX_OK && ng > 10, "grains for the schedules");
  std::vector<float> firsts((size_t)ng);
  for (int64_t g = 0; g < ng; ++g) firsts[(size_t)g] = w[(size_t)gs[g]];
  auto steps_result = [&](int rc, mx_step *st, int64_t ns, int64_t total) -> Result {
    if (rc < 0) {
      CHECK(st == nullptr, "schedule: steps set on failure");
      return {rc, 0};
    }
    uint64_t h = fnv(st, (size_t)ns * sizeof(mx_step));
    h = fnv(&total, 8, h);
    mx_free(st);
    return {rc, h};
  };
  sweep("mx_schedule_build", [&]() -> Result {
    mx_step *st = nullptr;
    int64_t ns = 0, total = 0;
    const int rc = mx_schedule_build(w.data(), n, sr, gs, gl, ng, m, nm, &st, &ns, &total);
    return steps_result(rc, st, ns, total);
  });
  sweep("mx_schedule_build_from", [&]() -> Result {
    mx_step *st = nullptr;
    int64_t ns = 0, total = 0;
    double ce = 0.;
    const int rc = mx_schedule_build_from(w.data(), n, sr, gs, gl, ng, m, nm, 0.25, 30000, &st, &ns, &total, &ce);
    return steps_result(rc, st, ns, total);
  });
  sweep("mx_schedule_build_table", [&]() -> Result {
    mx_step *st = nullptr;
    int64_t ns = 0, total = 0;
    double ce = 0.;
    const int rc = mx_schedule_build_table(n, sr, gs, gl, firsts.data(), ng, m, nm, 0.0, -1, &st, &ns, &total, &ce);
    return steps_result(rc, st, ns, total);
  });
  sweep("mx_pv_render_length", [&]() -> Result {
    const int64_t v = mx_pv_render_length(n, sr, m, nm);
    return {v < 0 ? v : 0, (uint64_t)v};
  });
  sweep("mx_pv_plan", [&]() -> Result {
    int64_t *ap = nullptr, *i0 = nullptr, fr = 0, ns = 0;
    double *tf = nullptr, *rf = nullptr;
    const int rc = mx_pv_plan(n, sr, m, nm, &ap, &tf, &rf, &i0, &fr, &ns);
    if (rc < 0) {
      CHECK(!ap && !i0 && !tf && !rf, "mx_pv_plan: outputs set on failure");
      return {rc, 0};
    }
    uint64_t h = fnv(ap, (size_t)fr * 8);
    h = fnv(tf, (size_t)fr * 8, h);
    h = fnv(rf, (size_t)fr * 8, h);
    h = fnv(i0, (size_t)(fr + 1) * 8, h);
    mx_free(ap);
    mx_free(tf);
    mx_free(rf);
    mx_free(i0);
    return {rc, h};
  });
  {
    std::vector<int16_t> pcm(5000);
    for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (int16_t)(i * 37 % 2000 - 1000);
    char path[] = "/tmp/mx_fault_sweep_XXXXXX";
    const int fd = mkstemp(path);
    if (fd >= 0) close(fd);
    sweep("mx_save_wav", [&]() -> Result {
      const int rc = mx_save_wav(path, pcm.data(), (int64_t)pcm.size(), sr, 1);
      return {rc, 0};
    });
    remove(path);
  }
  sweep("mx_minmax_range / pitch helpers", [&]() -> Result {
    int a = 0, b = 0;
    mx_pitch_band(4096, sr, &a, &b);
    const double nb = mx_note_bin(mx_bin_note(100, 4096, sr), 4096, sr);
    const int rl = mx_stft_run_length(4096, 256, 675000);
    const int64_t fc = mx_frame_count(n, 256);
    float mn = 0.f, mxv = 0.f;
    const float picks[4] = {-1.f, 1.f, -2.f, 2.f};
    const int64_t counts[1] = {2};
    mx_minmax_range(w.data(), 4, picks, counts, 1, 0, 4, &mn, &mxv);
    double v[6] = {(double)a, (double)b, nb, (double)rl, (double)fc, (double)mn + mxv};
    return {rl > 0 && fc > 0 ? 0 : -1, fnv(v, sizeof v)};
  });
  mx_free(gs);
  mx_free(gl);
  // the host logic of the mastering chain over a record list: 321 steps of S = 480 — 300 whole steps and two more gating hops, so
  // that the range has its 3 s windows —, the last one partial
  const int S = 480;
  std::vector<mx_loud_step> rec(321);
  for (size_t b = 0; b < rec.size(); ++b) rec[b] = mx_loud_step{(double)S * 1e-3 * (double)(1 + b * 7 % 13), 0.1f * (float)(1 + b % 5), S};
  rec.back().samples = 129;
  const int64_t nrec = (int64_t)rec.size(), covered = (nrec - 1) * S + 129;
  std::vector<double> curve((size_t)nrec);
  sweep("mx_loudness_curve", [&]() -> Result {
    const int rc = mx_loudness_curve(rec.data(), nrec, sr, 40, curve.data());
    return {rc, rc < 0 ? 0 : fnv(curve.data(), curve.size() * 8)};
  });
  sweep("mx_loudness_integrated", [&]() -> Result {
    mx_loudness m{};
    m.blocks = -7;
    const int rc = mx_loudness_integrated(rec.data(), nrec, sr, &m);
    if (rc < 0) CHECK(m.blocks == -7, "mx_loudness_integrated: output written on failure");
    const double v[5] = {m.integrated, m.momentary_max, m.shortterm_max, (double)m.peak, (double)(m.blocks * 1000 + m.passed_rel)};
    return {rc, rc < 0 ? 0 : fnv(v, sizeof v)};
  });
  sweep("mx_loudness_range", [&]() -> Result {
    mx_loudness_range_result r{};
    r.values = -7;
    const int rc = mx_loudness_range(rec.data(), nrec, sr, &r);
    if (rc < 0) CHECK(r.values == -7, "mx_loudness_range: output written on failure");
    const double v[4] = {r.lra, r.low_lufs, r.high_lufs, (double)(r.values * 1000 + r.gated)};
    return {rc, rc < 0 ? 0 : fnv(v, sizeof v)};
  });
  // three notes: whole steps inside, shorter than a step (the step that holds its middle), up to the last covered sample
  const std::vector<mx_note> notes = {{1000, 30000, 0, 0, 60., 0.f, 0.f}, {40000, 40100, 0, 0, 62., 0.f, 0.f},
                                      {90000, (int32_t)covered - 1, 0, 0, 64., 0.f, 0.f}};
  const int64_t nnotes = (int64_t)notes.size();
  sweep("mx_note_loudness", [&]() -> Result {
    double lufs[3] = {-7., -7., -7.};
    const int rc = mx_note_loudness(rec.data(), nrec, sr, notes.data(), nnotes, lufs);
    if (rc < 0) CHECK(lufs[0] == -7. && lufs[2] == -7., "mx_note_loudness: output written on failure");
    return {rc, rc < 0 ? 0 : fnv(lufs, sizeof lufs)};
  });
  sweep("mx_level_gain_points", [&]() -> Result {
    const double lufs[3] = {-30., std::nan(""), -18.};  // (a note without a loudness keeps amp 1)
    mx_gain_point pts[6] = {};
    double ref = -7.;
    const int rc = mx_level_gain_points(notes.data(), nnotes, lufs, nullptr, pts, &ref);
    if (rc < 0) CHECK(ref == -7. && pts[0].amp == 0.f, "mx_level_gain_points: output written on failure");
    return {rc, rc < 0 ? 0 : fnv(pts, sizeof pts, fnv(&ref, 8))};
  });
  sweep("mx_sibilant_gain_points", [&]() -> Result {
    const mx_sibilant sibs[2] = {{5000, 9000, 0, 0, 0.8f, 0.1f}, {20000, 20400, 0, 0, 0.7f, 0.1f}};
    mx_gain_point *pts = nullptr;
    int64_t npts = -5;
    const int rc = mx_sibilant_gain_points(sibs, 2, -6.0, 64, covered, &pts, &npts);
    if (rc < 0) {
      CHECK(pts == nullptr && npts == -5, "mx_sibilant_gain_points: outputs set on failure");
      return {rc, 0};
    }
    const uint64_t h = fnv(pts, (size_t)npts * sizeof(mx_gain_point));
    mx_free(pts);
    return {rc, h};
  });
  // the host logic of the analysis units that hands arrays out: two notes in a synthetic track, three peaks in a synthetic curve
  std::vector<mx_f0> track(200, mx_f0{0, 0.f, 1.f, 0.f});
  for (int f = 10; f < 180; ++f)
    if (f < 80 || f >= 100) track[(size_t)f] = mx_f0{f < 80 ? 218 : 145, f < 80 ? 218.18f : 145.45f, 0.05f, 0.1f};
  mx_note_params np;
  mx_note_params_default(&np);
  sweep("mx_detect_notes", [&]() -> Result {
    mx_note *out = nullptr;
    int64_t nn = -5;
    const int rc = mx_detect_notes(track.data(), (int64_t)track.size(), sr, 256, 0, &np, &out, &nn);
    if (rc < 0) {
      CHECK(out == nullptr && nn == -5, "mx_detect_notes: outputs set on failure");
      return {rc, 0};
    }
    const uint64_t h = fnv(out, (size_t)nn * sizeof(mx_note), (uint64_t)nn);
    mx_free(out);
    return {rc, h};
  });
  std::vector<float> flux(400, 0.5f);
  for (const int f : {50, 150, 300}) flux[(size_t)f] = 20.f;
  sweep("mx_onset_pick", [&]() -> Result {
    mx_onset *out = nullptr;
    int64_t no = -5;
    const int rc = mx_onset_pick(flux.data(), (int64_t)flux.size(), 256, 0, nullptr, &out, &no);
    if (rc < 0) {
      CHECK(out == nullptr && no == -5, "mx_onset_pick: outputs set on failure");
      return {rc, 0};
    }
    const uint64_t h = fnv(out, (size_t)no * sizeof(mx_onset), (uint64_t)no);
    mx_free(out);
    return {rc, h};
  });
  sweep("mx_timing_markers", [&]() -> Result {
    const int32_t anchors[3] = {50 * 256, 150 * 256, 300 * 256};
    mx_marker *out = nullptr;
    int64_t no = -5;
    const int rc = mx_timing_markers(anchors, 3, n, sr, nullptr, nullptr, 0, &out, &no);
    if (rc < 0) {
      CHECK(out == nullptr && no == -5, "mx_timing_markers: outputs set on failure");
      return {rc, 0};
    }
    uint64_t h = (uint64_t)no;
    for (int64_t i = 0; i < no; ++i) h = fnv(&out[i].pitchBend, 8, fnv(&out[i].dTime, 8, fnv(&out[i].note, 8, fnv(&out[i].sample, 4, h))));
    mx_free(out);
    return {rc, h};
  });
}

// The analysis units over the device take (tempo, chroma and key, pitch contour, f0 decode): their host forms pass through the
// context's staging buffers, work memory and job buffers.  The inputs of each are made once, unfaulted.
void analysis_entries(mx_ctx *ctx, mx_audio *a, int sr, int hop, int64_t F) {
  std::vector<float> flux((size_t)F), curve((size_t)F);
  CHECK(mx_onset_flux(ctx, a, sr, hop, 0, F, nullptr, flux.data()) == MX_OK, "flux: %s", mx_last_error());
  sweep("mx_tempo_smooth", [&]() -> Result {
    const int rc = mx_tempo_smooth(ctx, flux.data(), F, 4, curve.data());
    return {rc, rc < 0 ? 0 : fnv(curve.data(), curve.size() * 4)};
  });
  std::vector<mx_comb_job> combs;
  for (int k = 0; k < 12; ++k) combs.push_back(mx_comb_job{k, (int32_t)F - 2 * k, (uint32_t)(40 + 7 * k) << 16});
  sweep("mx_tempo_comb", [&]() -> Result {
    std::vector<mx_comb> rec(combs.size());
    const int rc = mx_tempo_comb(ctx, curve.data(), F, combs.data(), (int64_t)combs.size(), rec.data());
    return {rc, rc < 0 ? 0 : fnv(rec.data(), rec.size() * sizeof(mx_comb))};
  });
  auto tempo_result = [&](const char *name, int rc, const mx_tempo &t, mx_tempo_window *win, int64_t nwin) -> Result {
    if (rc < 0) {
      CHECK(t.levels == -7 && win == nullptr && nwin == -5, "%s: outputs set on failure", name);
      return {rc, 0};
    }
    const double v[6] = {t.bpm, t.offset, (double)t.score, (double)t.clarity, (double)t.locked_frames, (double)t.levels};
    const uint64_t h = fnv(win, (size_t)nwin * sizeof(mx_tempo_window), fnv(v, sizeof v));
    mx_free(win);
    return {rc, h};
  };
  sweep("mx_tempo_from_flux (windows)", [&]() -> Result {
    mx_tempo t{};
    t.levels = -7;
    mx_tempo_window *win = nullptr;
    int64_t nwin = -5;
    const int rc = mx_tempo_from_flux(ctx, flux.data(), F, sr, hop, 0, nullptr, &t, &win, &nwin);
    return tempo_result("mx_tempo_from_flux", rc, t, win, nwin);
  });
  sweep("mx_tempo_detect", [&]() -> Result {
    mx_tempo t{};
    t.levels = -7;
    mx_tempo_window *win = nullptr;
    int64_t nwin = -5;
    const int rc = mx_tempo_detect(ctx, a, sr, hop, nullptr, nullptr, &t, &win, &nwin);
    return tempo_result("mx_tempo_detect", rc, t, win, nwin);
  });
  std::vector<mx_chroma_rec> chroma((size_t)F);
  sweep("mx_chroma", [&]() -> Result {
    const int rc = mx_chroma(ctx, a, sr, hop, 0, F, nullptr, chroma.data());
    return {rc, rc < 0 ? 0 : fnv(chroma.data(), chroma.size() * sizeof(mx_chroma_rec))};
  });
  sweep("mx_chroma_sum", [&]() -> Result {
    const mx_chroma_job jobs[3] = {{0, F}, {10, 100}, {F, 0}};
    double sums[3 * 40];
    const int rc = mx_chroma_sum(ctx, chroma.data(), F, jobs, 3, sums);
    return {rc, rc < 0 ? 0 : fnv(sums, sizeof sums)};
  });
  sweep("mx_key_detect (windows)", [&]() -> Result {
    mx_key key{};
    key.tonic = -7;
    mx_key_window *win = nullptr;
    int64_t nwin = -5;
    const int rc = mx_key_detect(ctx, a, sr, hop, nullptr, 256, 128, &key, &win, &nwin);
    if (rc < 0) {
      CHECK(key.tonic == -7 && win == nullptr && nwin == -5, "mx_key_detect: outputs set on failure");
      return {rc, 0};
    }
    const uint64_t h = fnv(win, (size_t)nwin * sizeof(mx_key_window), fnv(&key, sizeof key));
    mx_free(win);
    return {rc, h};
  });
  std::vector<mx_f0> track((size_t)F), decoded((size_t)F);
  std::vector<mx_f0_cand> cands((size_t)F * MX_F0_CANDS);
  CHECK(mx_f0_candidates(ctx, a, sr, hop, 0, F, 55.f, 1760.f, 0.15f, track.data(), cands.data()) == MX_OK, "ladder: %s", mx_last_error());
  sweep("mx_f0_decode", [&]() -> Result {
    std::vector<uint8_t> state((size_t)F);
    const int rc = mx_f0_decode(ctx, track.data(), cands.data(), F, nullptr, decoded.data(), state.data());
    return {rc, rc < 0 ? 0 : fnv(state.data(), state.size(), fnv(decoded.data(), decoded.size() * sizeof(mx_f0)))};
  });
  sweep("mx_f0_track_decoded", [&]() -> Result {
    const int rc = mx_f0_track_decoded(ctx, a, sr, hop, 0, F, 55.f, 1760.f, 0.15f, nullptr, decoded.data());
    return {rc, rc < 0 ? 0 : fnv(decoded.data(), decoded.size() * sizeof(mx_f0))};
  });
  std::vector<int32_t> cents((size_t)F);
  sweep("mx_contour_cents", [&]() -> Result {
    const int rc = mx_contour_cents(ctx, decoded.data(), F, sr, 0.15f, 1e-3f, cents.data());
    return {rc, rc < 0 ? 0 : fnv(cents.data(), cents.size() * 4)};
  });
  // spans: the voiced runs of the take, cut into pieces of up to 100 frames (at least 4); the notes that give them
  std::vector<mx_contour_span> spans;
  std::vector<mx_note> notes;
  for (int64_t f = 0, run = 0; f <= F; ++f) {
    const bool voiced = f < F && cents[(size_t)f] != MX_CONTOUR_NONE;
    if (voiced && run < 100) {
      ++run;
      continue;
    }
    if (run >= 4) {
      spans.push_back(mx_contour_span{(int32_t)(f - run), (int32_t)run});
      notes.push_back(mx_note{(int32_t)((f - run) * hop), (int32_t)((f - 1) * hop), (int32_t)(f - run), (int32_t)run, 60., 0.f, 0.f});
    }
    run = voiced ? 1 : 0;
  }
  const int64_t ns = (int64_t)spans.size();
  CHECK(ns >= 2, "the take gives %lld spans", (long long)ns);
  mx_contour_params cp{};
  CHECK(mx_contour_params_default(sr, hop, &cp) == MX_OK, "contour parameters: %s", mx_last_error());
  std::vector<mx_contour_rec> rec((size_t)F);
  std::vector<mx_contour_stat> stat((size_t)ns);
  sweep("mx_contour_split", [&]() -> Result {
    const int rc = mx_contour_split(ctx, cents.data(), F, spans.data(), ns, &cp, rec.data(), stat.data());
    return {rc, rc < 0 ? 0 : fnv(stat.data(), stat.size() * sizeof(mx_contour_stat), fnv(rec.data(), rec.size() * sizeof(mx_contour_rec)))};
  });
  sweep("mx_contour_split (statistics)", [&]() -> Result {
    const int rc = mx_contour_split(ctx, cents.data(), F, spans.data(), ns, &cp, nullptr, stat.data());
    return {rc, rc < 0 ? 0 : fnv(stat.data(), stat.size() * sizeof(mx_contour_stat))};
  });
  sweep("mx_pitch_contour", [&]() -> Result {
    const int rc = mx_pitch_contour(ctx, decoded.data(), F, sr, hop, 0, notes.data(), ns, 0.15f, 1e-3f, nullptr, rec.data(), stat.data());
    return {rc, rc < 0 ? 0 : fnv(stat.data(), stat.size() * sizeof(mx_contour_stat), fnv(rec.data(), rec.size() * sizeof(mx_contour_rec)))};
  });
}

void device_entries() {
  printf("device entry points (allocations made from the library's own code):\n");
  const int sr = 48000;
  const int64_t n = 6 * sr;
  const std::vector<float> w = make_sweep(n);
  const std::vector<mx_marker> mk = {{1, 0., 0., 3.0}, {(int32_t)n - 1, 0., 0., 3.0}};
  mx_ctx *ctx = nullptr;
  sweep("mx_ctx_create / destroy", [&]() -> Result {
    mx_ctx *c = nullptr;
    const int rc = mx_ctx_create(0, &c);
    if (rc < 0) {
      CHECK(c == nullptr, "mx_ctx_create: handle set on failure");
      return {rc, 0};
    }
    mx_ctx_destroy(c);
    return {rc, 0};
  });
  if (mx_ctx_create(0, &ctx) != MX_OK) {
    CHECK(false, "no device: %s", mx_last_error());
    return;
  }
  mx_audio *a = nullptr;
  sweep("mx_audio_upload / free", [&]() -> Result {
    mx_audio *x = nullptr;
    const int rc = mx_audio_upload(ctx, w.data(), n, &x);
    if (rc < 0) {
      CHECK(x == nullptr, "mx_audio_upload: handle set on failure");
      return {rc, 0};
    }
    const int64_t len = mx_audio_length(x);
    mx_audio_free(ctx, x);
    return {rc, (uint64_t)len};
  });
  CHECK(mx_audio_upload(ctx, w.data(), n, &a) == MX_OK, "upload: %s", mx_last_error());
  const int N = 4096, hop = 256;
  const int64_t F = mx_frame_count(n, hop);
  std::vector<float> mags((size_t)F * (N / 2));
  std::vector<mx_pitch> pitch((size_t)F);
  // (a fresh context per sweep of the first STFT call would rebuild the tables each time; instead the sweep runs on a context
  // whose tables exist and, once, on a context that has none: release_scratch does not drop tables, a new context does)
  sweep("mx_stft_hop (first use: tables)", [&]() -> Result {
    mx_ctx *c = nullptr;
    mx_audio *x = nullptr;
    const bool was = g_in_call;
    g_in_call = false;  // (context and upload are not the subject here)
    const int r0 = mx_ctx_create(0, &c);
    const int r1 = r0 == MX_OK ? mx_audio_upload(c, w.data(), 8192, &x) : -1;
    g_in_call = was;
    if (r0 < 0 || r1 < 0) return {-100, 0};
    std::vector<mx_pitch> p(32);
    const int rc = mx_stft_hop(c, x, N, hop, 0, 32, -1, -1, nullptr, p.data());
    const uint64_t h = rc < 0 ? 0 : fnv(p.data(), p.size() * sizeof(mx_pitch));
    g_in_call = false;
    mx_audio_free(c, x);
    mx_ctx_destroy(c);
    g_in_call = was;
    return {rc, h};
  });
  sweep("mx_stft_hop", [&]() -> Result {
    const int rc = mx_stft_hop(ctx, a, N, hop, 0, F, -1, -1, mags.data(), pitch.data());
    return {rc, rc < 0 ? 0 : fnv(pitch.data(), pitch.size() * sizeof(mx_pitch), fnv(mags.data(), mags.size() * 4))};
  });
  std::vector<int32_t> ranges;
  for (int c = 0; c < 200; ++c) {
    ranges.push_back(c * 375 - 100);
    ranges.push_back(c * 375 + 275);
  }
  const int64_t R = (int64_t)ranges.size() / 2;
  std::vector<uint8_t> rgb((size_t)R * (N / 2) * 3);
  sweep("mx_stft_ranges", [&]() -> Result {
    const int rc = mx_stft_ranges(ctx, a, N, ranges.data(), R, -1, -1, mags.data(), pitch.data());
    return {rc, rc < 0 ? 0 : fnv(pitch.data(), (size_t)R * sizeof(mx_pitch), fnv(mags.data(), (size_t)R * (N / 2) * 4))};
  });
  sweep("mx_stft_ranges_rgb_mags", [&]() -> Result {
    const int rc = mx_stft_ranges_rgb_mags(ctx, a, N, ranges.data(), R, 900.f, mags.data(), rgb.data());
    return {rc, rc < 0 ? 0 : fnv(rgb.data(), rgb.size())};
  });
  sweep("mx_stft_ranges_keep / rows", [&]() -> Result {
    mx_rows *rows = nullptr;
    int rc = mx_stft_ranges_keep(ctx, a, N, ranges.data(), R, 900.f, nullptr, rgb.data(), &rows);
    if (rc < 0) {
      CHECK(rows == nullptr, "mx_stft_ranges_keep: handle set on failure");
      return {rc, 0};
    }
    uint64_t h = fnv(rgb.data(), rgb.size());
    rc = mx_rows_fetch(ctx, rows, 3, 50, mags.data());
    if (rc == MX_OK) rc = mx_rows_colormap(ctx, rows, 3, 50, 400.f, rgb.data());
    if (rc == MX_OK) h = fnv(rgb.data(), (size_t)50 * (N / 2) * 3, fnv(mags.data(), (size_t)50 * (N / 2) * 4, h));
    mx_rows_free(ctx, rows);
    return {rc, h};
  });
  int32_t *gs = nullptr, *gl = nullptr;
  float *gf = nullptr;
  int64_t ng = 0;
  sweep("mx_grain_table_dev", [&]() -> Result {
    int32_t *s = nullptr, *l = nullptr;
    float *f = nullptr;
    int64_t c = 0;
    const int rc = mx_grain_table_dev(ctx, a, &s, &l, &f, &c);
    if (rc < 0) {
      CHECK(!s && !l && !f, "mx_grain_table_dev: outputs set on failure");
      return {rc, 0};
    }
    uint64_t h = fnv(s, (size_t)c * 4, fnv(l, (size_t)c * 4, fnv(f, (size_t)c * 4)));
    mx_free(s);
    mx_free(l);
    mx_free(f);
    return {rc, h};
  });
  sweep("mx_grains_dev", [&]() -> Result {
    int32_t *s = nullptr, *l = nullptr;
    int64_t c = 0;
    const int rc = mx_grains_dev(ctx, a, &s, &l, &c);
    if (rc < 0) {
      CHECK(!s && !l, "mx_grains_dev: outputs set on failure");
      return {rc, 0};
    }
    const uint64_t h = fnv(s, (size_t)c * 4, fnv(l, (size_t)c * 4));
    mx_free(s);
    mx_free(l);
    return {rc, h};
  });
  CHECK(mx_grain_table_dev(ctx, a, &gs, &gl, &gf, &ng) == MX_OK, "grain table: %s", mx_last_error());
  mx_step *steps = nullptr;
  int64_t nsteps = 0, total = 0;
  CHECK(mx_schedule_build_table(n, sr, gs, gl, gf, ng, mk.data(), (int)mk.size(), 0.0, -1, &steps, &nsteps, &total, nullptr) == MX_OK, "schedule");
  std::vector<float> pf((size_t)std::max<int64_t>(total, n));
  std::vector<int16_t> pi((size_t)std::max<int64_t>(total, n));
  sweep("mx_resynth", [&]() -> Result {
    const int rc = mx_resynth(ctx, a, steps, nsteps, total, pf.data(), pi.data());
    return {rc, rc < 0 ? 0 : fnv(pi.data(), (size_t)total * 2, fnv(pf.data(), (size_t)total * 4))};
  });
  char path[] = "/tmp/mx_fault_sweep_wav_XXXXXX";
  {
    const int fd = mkstemp(path);
    if (fd >= 0) close(fd);
  }
  auto file_sum = [&]() -> uint64_t {
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    std::vector<unsigned char> b(1 << 20);
    uint64_t h = 1469598103934665603ull;
    size_t got;
    while ((got = fread(b.data(), 1, b.size(), f)) > 0) h = fnv(b.data(), got, h);
    fclose(f);
    return h;
  };
  sweep("mx_resynth_to_wav", [&]() -> Result {
    const int rc = mx_resynth_to_wav(ctx, a, steps, nsteps, total, path, sr, 1);
    return {rc, rc < 0 ? 0 : file_sum()};
  });
  sweep("mx_export_wav", [&]() -> Result {
    const int rc = mx_export_wav(ctx, w.data(), n, sr, mk.data(), (int)mk.size(), path, 1);
    return {rc, rc < 0 ? 0 : file_sum()};
  });
  remove(path);
  sweep("mx_pv_pitch_shift", [&]() -> Result {
    const int rc = mx_pv_pitch_shift(ctx, a, 3.0, pf.data(), pi.data());
    return {rc, rc < 0 ? 0 : fnv(pi.data(), (size_t)n * 2, fnv(pf.data(), (size_t)n * 4))};
  });
  sweep("mx_pv_pitch_shift (arena rebuilt)", [&]() -> Result {
    // every call builds the arena anew: the pipe's construction (streams, events, host tables) is swept too, and a failure
    // in the middle of it must not leave a half-built pipe for the next call to find
    int rc = mx_ctx_release_scratch(ctx);
    if (rc == MX_OK) rc = mx_pv_pitch_shift(ctx, a, 3.0, pf.data(), nullptr);
    return {rc, rc < 0 ? 0 : fnv(pf.data(), (size_t)n * 4)};
  });
  sweep("mx_pv_pitch_shift (chunks of 64)", [&]() -> Result {
    int rc = mx_pv_set_chunk_frames(ctx, 64);
    if (rc == MX_OK) rc = mx_pv_pitch_shift(ctx, a, 3.0, pf.data(), nullptr);
    const bool was = g_in_call;
    g_in_call = false;
    mx_pv_set_chunk_frames(ctx, 0);
    g_in_call = was;
    return {rc, rc < 0 ? 0 : fnv(pf.data(), (size_t)n * 4)};
  });
  sweep("mx_pv_render", [&]() -> Result {
    const int64_t len = mx_pv_render_length(n, sr, mk.data(), (int)mk.size());
    if (len < 0) return {len, 0};
    std::vector<float> out((size_t)len);
    const int rc = mx_pv_render(ctx, a, sr, mk.data(), (int)mk.size(), out.data(), nullptr);
    return {rc, rc < 0 ? 0 : fnv(out.data(), out.size() * 4)};
  });
  sweep("mx_pv_shard_* (rank 1 of 2)", [&]() -> Result {
    // rank 0's map and seams come from an unfaulted pass on a second context
    const bool was = g_in_call;
    g_in_call = false;
    mx_ctx *c0 = nullptr;
    mx_audio *a0 = nullptr;
    std::vector<uint32_t> s0(2048), carry(2048);
    std::vector<uint16_t> o0(2048);
    std::vector<float> h0(3840), t0(3840), h1(3840), t1(3840);
    int rc = mx_ctx_create(0, &c0);
    if (rc == MX_OK) rc = mx_audio_upload(c0, w.data(), n, &a0);
    if (rc == MX_OK) rc = mx_pv_shard_analyze(c0, a0, 3.0, 0, 2, s0.data(), o0.data());
    if (rc == MX_OK) rc = mx_pv_shard_synthesize(c0, nullptr, h0.data(), t0.data());
    g_in_call = was;
    uint64_t h = 0;
    if (rc == MX_OK) {
      std::vector<uint32_t> s1(2048);
      std::vector<uint16_t> o1(2048);
      rc = mx_pv_shard_analyze(ctx, a, 3.0, 1, 2, s1.data(), o1.data());
      for (int k = 0; k < 2048; ++k) carry[(size_t)k] = s0[(size_t)k];  // rank 0 restarts every bin: its map applied to zeros = its sums
      if (rc == MX_OK) rc = mx_pv_shard_synthesize(ctx, carry.data(), h1.data(), t1.data());
      int64_t lo = 0, hi = 0;
      if (rc == MX_OK) rc = mx_pv_shard_frames(n, 3.0, 1, 2, nullptr, nullptr, &lo, &hi);
      if (rc == MX_OK) rc = mx_pv_shard_finish(ctx, t0.data(), nullptr, pf.data(), pi.data());
      if (rc == MX_OK) h = fnv(pi.data(), (size_t)(hi - lo) * 2, fnv(pf.data(), (size_t)(hi - lo) * 4));
    } else {
      rc = -100;
    }
    g_in_call = false;
    if (a0) mx_audio_free(c0, a0);
    if (c0) mx_ctx_destroy(c0);
    g_in_call = was;
    return {rc, h};
  });
  sweep("mx_minmax_pyramid", [&]() -> Result {
    std::vector<float> picks((size_t)2 * n);
    int64_t counts[64];
    int nl = 0;
    const int rc = mx_minmax_pyramid(ctx, a, picks.data(), counts, &nl);
    uint64_t h = 0;
    if (rc == MX_OK) {
      int64_t tot = 0;
      for (int l = 0; l < nl; ++l) tot += counts[l];
      h = fnv(picks.data(), (size_t)tot * 8);
    }
    return {rc, h};
  });
  sweep("mx_f0_track", [&]() -> Result {
    std::vector<mx_f0> f0((size_t)F);
    const int rc = mx_f0_track(ctx, a, sr, hop, 0, F, 55.f, 1760.f, 0.15f, f0.data());
    return {rc, rc < 0 ? 0 : fnv(f0.data(), f0.size() * sizeof(mx_f0))};
  });
  analysis_entries(ctx, a, sr, hop, F);
  // a derived audio object of `m` samples on context `c`: its handle is set only on success; its samples and both pads are the
  // checksum
  auto derived_on = [](mx_ctx *c, int64_t m, int rc, mx_audio *b, const std::vector<int16_t> *pcm) -> Result {
    if (rc < 0) {
      CHECK(b == nullptr, "derived audio: handle set on failure");
      return {rc, 0};
    }
    std::vector<float> all((size_t)(m + 2 * MX_AUDIO_PAD));
    rc = mx_audio_length(b) == m ? mx_audio_download(c, b, -(int64_t)MX_AUDIO_PAD, (int64_t)all.size(), all.data()) : -100;
    mx_audio_free(c, b);
    return {rc, rc < 0 ? 0 : fnv(all.data(), all.size() * 4, pcm ? fnv(pcm->data(), pcm->size() * 2) : 0)};
  };
  // the take processors' arguments: 48 kHz to 44.1 kHz, a flat print with {12, 6}, the compressor's defaults (the sweep peaks at
  // 0.5, over their threshold)
  const int out_sr = 44100;
  const std::vector<float> print(MX_DENOISE_BINS, 1e-4f);
  const mx_denoise_params dp{12.f, 6.f};
  // the mastering chain at the smallest sizes that take every branch: 2049 samples at 48 kHz (one limiter tile plus one sample, 5
  // steps, one group) and one sample
  for (const int64_t len : {(int64_t)2049, (int64_t)1}) {
    mx_audio *s = nullptr;
    CHECK(mx_audio_upload(ctx, w.data() + 1000, len, &s) == MX_OK, "upload of %lld: %s", (long long)len, mx_last_error());
    const int64_t steps = mx_loudness_step_count(len, sr);
    char label[64];
    auto named = [&](const char *what) {
      snprintf(label, sizeof label, "%s (n = %lld)", what, (long long)len);
      return label;
    };
    sweep(named("mx_loudness_steps"), [&]() -> Result {
      std::vector<mx_loud_step> rec((size_t)steps);
      const int rc = mx_loudness_steps(ctx, s, sr, 0, (steps + 9) / 10, rec.data());
      uint64_t h = 0;
      for (const mx_loud_step &r : rec) h = fnv(&r.samples, 4, fnv(&r.peak, 4, fnv(&r.energy, 8, h)));
      return {rc, rc < 0 ? 0 : h};
    });
    sweep(named("mx_loudness_measure"), [&]() -> Result {
      mx_loudness m{};
      m.blocks = -7;
      const int rc = mx_loudness_measure(ctx, s, sr, &m);
      if (rc < 0) CHECK(m.blocks == -7, "mx_loudness_measure: output written on failure");
      const double v[5] = {m.integrated, m.momentary_max, m.shortterm_max, (double)m.peak, (double)m.blocks};
      return {rc, rc < 0 ? 0 : fnv(v, sizeof v)};
    });
    sweep(named("mx_true_peak_steps"), [&]() -> Result {
      std::vector<mx_tp_step> rec((size_t)steps);
      const int rc = mx_true_peak_steps(ctx, s, sr, 0, steps, rec.data());
      return {rc, rc < 0 ? 0 : fnv(rec.data(), rec.size() * sizeof(mx_tp_step))};
    });
    sweep(named("mx_true_peak_measure"), [&]() -> Result {
      float v[2] = {-7.f, -7.f};
      const int rc = mx_true_peak_measure(ctx, s, sr, &v[0], &v[1]);
      if (rc < 0) CHECK(v[0] == -7.f && v[1] == -7.f, "mx_true_peak_measure: outputs written on failure");
      return {rc, rc < 0 ? 0 : fnv(v, sizeof v)};
    });
    auto derived = [&](int rc, mx_audio *b, const std::vector<int16_t> *pcm) -> Result { return derived_on(ctx, len, rc, b, pcm); };
    sweep(named("mx_audio_gain (0 points)"), [&]() -> Result {
      mx_audio *b = nullptr;
      const int rc = mx_audio_gain(ctx, s, nullptr, 0, &b);
      return derived(rc, b, nullptr);
    });
    sweep(named("mx_audio_gain (2 points)"), [&]() -> Result {
      const mx_gain_point pts[2] = {{0, 0.5f}, {(int32_t)len, 2.f}};
      mx_audio *b = nullptr;
      const int rc = mx_audio_gain(ctx, s, pts, 2, &b);
      return derived(rc, b, nullptr);
    });
    const mx_limit_params lp{0.25f, 64};  // (the sweep peaks at 0.5: the limiter works)
    sweep(named("mx_audio_limit"), [&]() -> Result {
      mx_audio *b = nullptr;
      const int rc = mx_audio_limit(ctx, s, sr, &lp, &b, nullptr);
      return derived(rc, b, nullptr);
    });
    sweep(named("mx_audio_limit (int16)"), [&]() -> Result {
      std::vector<int16_t> pcm((size_t)len, (int16_t)0x5A5A);
      mx_audio *b = nullptr;
      const int rc = mx_audio_limit(ctx, s, sr, &lp, &b, pcm.data());
      return derived(rc, b, &pcm);
    });
    sweep(named("mx_audio_download"), [&]() -> Result {
      std::vector<float> all((size_t)(len + 2 * MX_AUDIO_PAD));
      const int rc = mx_audio_download(ctx, s, -(int64_t)MX_AUDIO_PAD, (int64_t)all.size(), all.data());
      return {rc, rc < 0 ? 0 : fnv(all.data(), all.size() * 4)};
    });
    // the take processors: a host form's outputs are pre-filled and must stand where it fails
    auto host_form = [&](const char *what, int rc, const void *f32, size_t nf, const void *i16, size_t ni) -> Result {
      const unsigned char *b = static_cast<const unsigned char *>(f32), *c = static_cast<const unsigned char *>(i16);
      if (rc < 0) {
        bool stands = true;
        for (size_t k = 0; k < nf; ++k) stands = stands && b[k] == 0x5A;
        for (size_t k = 0; k < ni; ++k) stands = stands && c[k] == 0x5A;
        CHECK(stands, "%s: outputs written on failure", what);
        return {rc, 0};
      }
      return {rc, fnv(i16, ni, fnv(f32, nf))};
    };
    const int64_t m = mx_resample_length(len, sr, out_sr), csteps = mx_compress_steps(len, sr);
    sweep(named("mx_resample"), [&]() -> Result {
      std::vector<float> out((size_t)m);
      memset(out.data(), 0x5A, out.size() * 4);
      return host_form("mx_resample", mx_resample(ctx, s, sr, out_sr, 0, m, out.data()), out.data(), out.size() * 4, nullptr, 0);
    });
    sweep(named("mx_audio_resample"), [&]() -> Result {
      mx_audio *b = nullptr;
      const int rc = mx_audio_resample(ctx, s, sr, out_sr, &b);
      return derived_on(ctx, m, rc, b, nullptr);
    });
    if (len == 2049)  // (one sample holds no frame of a print: the library refuses the region)
      sweep(named("mx_noise_print"), [&]() -> Result {
        std::vector<float> out(MX_DENOISE_BINS);
        memset(out.data(), 0x5A, out.size() * 4);
        return host_form("mx_noise_print", mx_noise_print(ctx, s, 0, 1024, out.data()), out.data(), out.size() * 4, nullptr, 0);
      });
    sweep(named("mx_denoise"), [&]() -> Result {
      std::vector<float> f((size_t)len);
      std::vector<int16_t> i((size_t)len);
      memset(f.data(), 0x5A, f.size() * 4);
      memset(i.data(), 0x5A, i.size() * 2);
      const int rc = mx_denoise(ctx, s, print.data(), &dp, 0, len, f.data(), i.data());
      return host_form("mx_denoise", rc, f.data(), f.size() * 4, i.data(), i.size() * 2);
    });
    sweep(named("mx_audio_denoise"), [&]() -> Result {
      mx_audio *b = nullptr;
      const int rc = mx_audio_denoise(ctx, s, print.data(), &dp, &b);
      return derived(rc, b, nullptr);
    });
    sweep(named("mx_compress"), [&]() -> Result {
      std::vector<float> f((size_t)len);
      std::vector<int16_t> i((size_t)len);
      memset(f.data(), 0x5A, f.size() * 4);
      memset(i.data(), 0x5A, i.size() * 2);
      const int rc = mx_compress(ctx, s, sr, nullptr, 0, len, f.data(), i.data());
      return host_form("mx_compress", rc, f.data(), f.size() * 4, i.data(), i.size() * 2);
    });
    sweep(named("mx_compress_gain"), [&]() -> Result {
      std::vector<int32_t> g((size_t)csteps);
      memset(g.data(), 0x5A, g.size() * 4);
      return host_form("mx_compress_gain", mx_compress_gain(ctx, s, sr, nullptr, 0, csteps, g.data()), g.data(), g.size() * 4, nullptr, 0);
    });
    sweep(named("mx_audio_compress"), [&]() -> Result {
      mx_audio *b = nullptr;
      const int rc = mx_audio_compress(ctx, s, sr, nullptr, &b);
      return derived(rc, b, nullptr);
    });
    mx_audio_free(ctx, s);
  }
  // ... and on a context of its own per call, so that the tables a context builds on first use (the 1024-point transform's
  // twiddles, the resampler's taps) are built, and faulted, under the call that owns the new object's buffer
  auto fresh = [&](int64_t m, const std::function<int(mx_ctx *, mx_audio *, mx_audio **)> &make) -> Result {
    mx_ctx *c = nullptr;
    mx_audio *s = nullptr, *b = nullptr;
    int rc = mx_ctx_create(0, &c);
    if (rc == MX_OK) rc = mx_audio_upload(c, w.data() + 1000, 2049, &s);
    if (rc == MX_OK) rc = make(c, s, &b);
    const Result r = rc == MX_OK ? derived_on(c, m, rc, b, nullptr) : Result{rc, 0};
    if (rc < 0) CHECK(b == nullptr, "derived audio on a fresh context: handle set on failure");
    const bool was = g_in_call;
    g_in_call = false;
    if (s) mx_audio_free(c, s);
    if (c) mx_ctx_destroy(c);
    g_in_call = was;
    return r;
  };
  sweep("mx_audio_denoise (fresh context)", [&]() -> Result {
    return fresh(2049, [&](mx_ctx *c, mx_audio *s, mx_audio **b) { return mx_audio_denoise(c, s, print.data(), &dp, b); });
  });
  sweep("mx_audio_resample (fresh context)", [&]() -> Result {
    return fresh(mx_resample_length(2049, sr, out_sr),
                 [&](mx_ctx *c, mx_audio *s, mx_audio **b) { return mx_audio_resample(c, s, sr, out_sr, b); });
  });
  sweep("mx_ctx_release_scratch", [&]() -> Result { return {mx_ctx_release_scratch(ctx), 0}; });
  mx_free(steps);
  mx_free(gs);
  mx_free(gl);
  mx_free(gf);
  mx_audio_free(ctx, a);
  mx_ctx_destroy(ctx);
}
}  // namespace

// what the sweep is there to catch, for the harness's own test: a C entry point that lets an exception out (noexcept stands in
// for the extern "C" boundary of a caller compiled as C: the exception has nowhere to go and the process is terminated)
extern "C" int unguarded_entry(void) noexcept {
  std::vector<int> v(1000);
  return (int)v.size() - 1000;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  if (mode == "selftest") {  // must NOT come back
    g_fail_at = 1;
    g_in_call = true;
    const int rc = unguarded_entry();
    g_in_call = false;
    printf("selftest: the unguarded entry point returned %d\n", rc);
    return 0;
  }
  printf("fault_sweep %s against %s\n", mode.c_str(), mx_version());
  if (mode == "host-malloc" || mode == "device-malloc") {
#ifndef SWEEP_MALLOC
    fprintf(stderr, "built without -DSWEEP_MALLOC\n");
    return 2;
#endif
    g_fault_malloc = true;
  }
  host_entries();
  if (mode == "device" || mode == "device-malloc") {
    g_only_library_callers = true;
    device_entries();
  }
  printf("fault_sweep %s: %ld faults injected, %d failed checks\n", mode.c_str(), g_total_faults, g_failed_checks);
  return g_failed_checks ? 1 : 0;
}
