// tempo_emu.cpp — the tempo estimator on the CPU: the kernels' arithmetic (melonix_amd/csrc/tempo_core.h) run thread by thread
// in the comb kernel's mapping (thread t takes phases t, t + threads, ..; the per-thread bests are then combined), and the
// library's own host logic (tempo_logic.cpp) over that comb.  tests/test_tempo_host.py compares every byte with
// tests/tempo_ref.py.  With -DTEMPO_EMU_MAIN it is a stand-alone program over the smallest shapes (for the sanitizers).
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared tempo_emu.cpp ../../melonix_amd/csrc/tempo_logic.cpp -o libtempo_emu.so
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../melonix_amd/csrc/tempo_core.h"
#include "../../melonix_amd/csrc/tempo_logic.h"

using namespace mx;
using namespace mx::tempo;

extern "C" {

int emu_tempo_smooth(const float *flux, long count, int W, float *out) {
  if (W < 0 || W > kMaxWidth) return -1;
  const SmoothWeights w = smooth_weights(W);
  for (long f = 0; f < count; ++f) out[f] = smooth_at(flux, count, f, W, w);
  return 0;
}

// one workgroup of `threads` threads per job; jobs are not checked (as on the device)
void emu_tempo_comb(const float *curve, long count, const mx_comb_job *jobs, long njobs, int threads, mx_comb *out) {
  std::vector<float> row(kMaxPhases);
  for (long j = 0; j < njobs; ++j) {
    const int nph = phases(jobs[j].period_q16);
    float best = 0.f;
    int best_phi = kMaxPhases;
    for (int t = threads - 1; t >= 0; --t) {  // (the threads' bests meet in some order: here the last thread's first)
      float tb = 0.f;
      int tp = kMaxPhases;
      for (int phi = t; phi < nph; phi += threads) {
        const float s = phase_score(curve, count, jobs[j], phi);
        row[(size_t)phi] = s;
        if (tp == kMaxPhases || better(s, phi, tb, tp)) tb = s, tp = phi;
      }
      if (tp != kMaxPhases && (best_phi == kMaxPhases || better(tb, tp, best, best_phi))) best = tb, best_phi = tp;
    }
    out[j] = record_at(row.data(), nph, best_phi);
  }
}

int emu_tempo_check_params(const mx_tempo_params *p) { return tempo_params_error(*p) ? -1 : 0; }
int emu_tempo_check_job(const mx_comb_job *job, long count) { return comb_job_error(*job, count) ? -1 : 0; }
int emu_tempo_check_ladder(const mx_tempo_params *p, int sr, int hop) {
  TempoLadder l;
  return tempo_ladder(*p, sr, hop, l) ? -1 : 0;
}

// the whole estimate; p null: the defaults.  windows: room for `cap` records, *nwindows the number there are.  -1: refused
int emu_tempo_estimate(const float *flux, long count, int sr, int hop, long first_frame, const mx_tempo_params *p, int threads,
                       mx_tempo *out, mx_tempo_window *windows, long cap, long *nwindows) {
  const mx_tempo_params q = p ? *p : kTempoDefaults;
  TempoLadder ladder;
  if (tempo_params_error(q) || tempo_ladder(q, sr, hop, ladder)) return -1;
  std::vector<float> e((size_t)count);
  emu_tempo_smooth(flux, count, q.smooth, e.data());
  std::vector<mx_tempo_window> win;
  const int rc = tempo_estimate(e.data(), count, first_frame, q, ladder,
                                [&](const std::vector<mx_comb_job> &jobs, std::vector<mx_comb> &rec) {
                                  for (const mx_comb_job &j : jobs)
                                    if (comb_job_error(j, count)) return -1;
                                  emu_tempo_comb(e.data(), count, jobs.data(), (long)jobs.size(), threads, rec.data());
                                  return 0;
                                },
                                *out, win);
  if (rc) return rc;
  *nwindows = (long)win.size();
  for (size_t i = 0; i < win.size() && (long)i < cap; ++i) windows[i] = win[i];
  return 0;
}

}  // extern "C"

#ifdef TEMPO_EMU_MAIN
int main() {
  // the smallest shapes: curves of 1, 2 and 65 frames, every width, jobs at both ends of the curve and of the period range,
  // and an estimate over a short pulse train
  unsigned acc = 0;
  for (long count : {1L, 2L, 65L}) {
    std::vector<float> o((size_t)count), e((size_t)count);
    for (long f = 0; f < count; ++f) o[(size_t)f] = (float)((f * 7 + 3) % 11);
    for (int W : {0, 1, 4, 32}) emu_tempo_smooth(o.data(), count, W, e.data());
    std::vector<mx_comb_job> jobs;
    for (uint32_t q : {kMinPeriod, kMinPeriod + 1u, 45u << 16, kMaxPeriod}) {
      jobs.push_back(mx_comb_job{0, (int32_t)count, q});
      jobs.push_back(mx_comb_job{0, 1, q});
      jobs.push_back(mx_comb_job{(int32_t)count - 1, 1, q});
    }
    std::vector<mx_comb> rec(jobs.size());
    emu_tempo_comb(e.data(), count, jobs.data(), (long)jobs.size(), 256, rec.data());
    for (const mx_comb &r : rec) acc += (unsigned)r.phase + (unsigned)(r.score * 16.f);
  }
  std::vector<float> flux(700, 0.f);
  for (size_t f = 20; f < flux.size(); f += 94) flux[f] = 10.f;
  mx_tempo t;
  std::vector<mx_tempo_window> win(64);
  long nwin = 0;
  mx_tempo_params p = kTempoDefaults;
  p.window_frames = 256;
  p.stride_frames = 64;
  if (emu_tempo_estimate(flux.data(), (long)flux.size(), 48000, 256, 0, &p, 256, &t, win.data(), (long)win.size(), &nwin)) return 1;
  std::printf("tempo_emu ok: %u, %.4f bpm, offset %.4f s, %ld windows, %d levels\n", acc, t.bpm, t.offset, nwin, t.levels);
  return 0;
}
#endif
