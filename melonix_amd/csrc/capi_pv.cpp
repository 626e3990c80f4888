// capi_pv.cpp — the build-defined phase-vocoder pitch shift (no reference counterpart): the chunk pipeline and the
// single-GPU entry points.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h, pv_pipe.h; the
// arena this runs in: capi_pv_arena.cpp; one rank of a multi-GPU run: capi_pv_shard.cpp).  There is no CPU compute path: every
// transform entry point needs a live gfx950 device and fails with MX_ERR_DEVICE otherwise.
//
// A call the arena holds in one chunk runs its kernels once each; what does not fit is walked chunk by chunk.  What one chunk
// hands the next is what one rank of a multi-GPU run hands its neighbour (pv_common.h, mx_pv_shard_*): the frame before the
// chunk is analysed again as its row 0, the dense offset row behind the chunk's last frame is the next chunk's carry_in, and the
// N - Hs samples across the boundary are the left chunk's raw tail plus the right chunk's raw head.  Chunks start on multiples
// of 32 frames (= the synthesis workgroups), so every float sum groups exactly as in one launch over the whole signal: outputs
// are bit-identical whatever the chunk length (tests/test_pv.py::test_gpu_chunked_equals_whole).
//
//   the context's stream   the two big kernels, one at a time:  A(0) A(1) S(0) A(2) S(1) A(3) S(2) ...
//   a side stream          everything small, beside an analysis: while A(k + 1) runs, the first-frame records, chunk maps
//                          and offsets of chunk k (pv_heads, pv_lock_walk, pv_lock_chunks), then pv_fixup + pv_resample of
//                          chunk k - 2
// Two slots of spectra + records alternate (chunk k + 1's analysis follows chunk k - 1's synthesis on the stream); the
// stretched signal and the workgroup halos of a chunk live in a ring of four.  Why nothing runs beside a synthesis, and
// why the two big kernels do not overlap each other: profiles/timeline_r05_pv_pipeline.log.
#include "pv_pipe.h"

using namespace mx;

namespace mx {

int64_t pv_frame_count(int64_t n, double r) { return (int64_t)std::ceil((double)n * r / kPvHs) + 1; }
// (the same binary64 expression as pv_resample evaluates)
int64_t pv_first_output_at(int64_t q, double r, int64_t n) {
  int64_t i = (int64_t)std::ceil(((double)q - kPvN / 2) / r);
  if (i < 0) i = 0;
  while (i > 0 && (int64_t)std::floor((double)(i - 1) * r + (double)(kPvN / 2)) >= q) --i;
  while (i < n && (int64_t)std::floor((double)i * r + (double)(kPvN / 2)) < q) ++i;
  return i < n ? i : n;
}

std::vector<PvChunk> pv_chunks_of(int64_t F_lo, int64_t F_hi, int64_t C) {
  std::vector<PvChunk> v;
  for (int64_t lo = F_lo; lo < F_hi;) {
    int64_t hi = std::min(F_hi, lo + C);
    if (F_hi - hi < 32) hi = F_hi;  // a remainder shorter than one synthesis workgroup rides with the last chunk
    v.push_back({lo, hi});
    lo = hi;
  }
  return v;
}

int pv_run(mx_ctx *ctx, PvPipe &p, PvRun &run) {
  NTables t;
  int rc = get_tables(ctx, kPvN, t);
  if (rc) return rc;
  const hipStream_t sm = ctx->stream, ss = p.ss, sf = p.sf;
  const std::vector<PvChunk> chunks = pv_chunks_of(run.F_lo, run.F_hi, p.shape.C);
  const int64_t K = (int64_t)chunks.size();
  if (K > 1 && (p.shape.slots < kPvSlots || p.shape.outs < kPvOutRing || p.shape.plans < kPvPlanRing))
    return fail(MX_ERR_INVALID, "phase vocoder: %lld chunks through an arena made for one", (long long)K);
  p.last_chunks = K;
  hipError_t e = hipSuccess;
  std::vector<PvArgs> args((size_t)K);
  for (int64_t k = 0; k < K; ++k) {
    const PvChunk c = chunks[(size_t)k];
    PvPipe::Slot &sl = p.slot[k % p.shape.slots];
    PvPipe::Out &o = p.out[k % p.shape.outs];
    const int64_t first = c.lo > 0 ? 1 : 0, Fl = c.hi - c.lo + first;
    PvArgs &g = args[(size_t)k];
    g = PvArgs{};
    g.audio = run.a->d_padded;
    g.n = run.a->n;
    g.ratio = run.r;
    g.frames = Fl;
    g.first = first;
    g.global_first = c.lo == 0;
    g.frame_base = c.lo;
    g.tw2 = t.tw2;
    g.tw3 = t.tw3;
    g.ubase = t.ubase;
    g.hann = p.hann;
    g.hann_scaled = p.hann_scaled;
    g.wsplit = p.wsplit;
    g.apos = p.plan[k % p.shape.plans].apos;
    g.hop = p.plan[k % p.shape.plans].hop;
    g.hratio = p.plan[k % p.shape.plans].hratio;
    g.xrows = sl.xrows;
    g.recs = sl.recs;
    g.rec_overflow = p.rec_overflow;
    g.pkmap = sl.pkmap;
    g.pkcount = sl.pkcount;
    g.fthr = sl.fthr;
    g.chunk_sums = sl.chunk_sums;
    g.chunk_org = sl.chunk_org;
    g.group_sums = sl.group_sums;
    g.group_org = sl.group_org;
    g.scan_chunk = (int)std::max<int64_t>(kPvMinScan, (Fl - first + kPvMaxScanChunks - 1) / kPvMaxScanChunks);
    g.halo = o.halo;
    g.s = o.s;
    g.s_len = (Fl - first) * kPvHs + kPvN;
    g.s_origin = c.lo * kPvHs;
    g.sample_rate = run.sample_rate;
    // frames per analysis workgroup: 16 in one launch over the whole signal (flat from 8 to 24 there); a chunk is four
    // rounds of workgroups at most, and what its launch loses is its ragged end — 8 (16: +0.8 ms per hour, 4: +0.2)
    g.frames_per_block = K > 1 ? 8 : 16;
    g.rec_wg_cap = (uint32_t)(g.frames_per_block * p.shape.rpf);
    g.rec_fpb_shift = g.frames_per_block == 8 ? 3 : 4;
    if (run.plan) {
      g.tf = o.tf;
      g.rf = o.rf;
      g.i0 = o.i0;
    }
    if (run.totals_only) {
      g.tot_sums = run.totmaps_sums + (size_t)k * kPvM;
      g.tot_org = run.totmaps_org + (size_t)k * kPvM;
    }
    g.carry_in = k > 0 ? p.carry[(k - 1) & 1] : run.carry_in;
    g.carry_out = p.carry[k & 1];
    // outputs of the chunk: those whose interpolation starts inside its hops (marker-driven: every frame owns its samples)
    if (!run.plan) {
      g.out_lo = k == 0 ? run.out_lo : pv_first_output_at(c.lo * kPvHs, run.r, run.a->n);
      g.out_hi = k == K - 1 ? run.out_hi : pv_first_output_at(c.hi * kPvHs, run.r, run.a->n);
    }
    g.pcm_f32 = run.pcm_f32;
    g.pcm_i16 = run.pcm_i16;
    g.pcm_base = run.pcm_base;
    if (k == 0 && run.defer_head) {
      // the rank's first N - Hs stretched samples need the previous rank's tail: their outputs wait for stage 3
      g.skip_head = 1;
      g.out_lo = std::min(g.out_hi, pv_first_output_at(c.lo * kPvHs + kPvSeam, run.r, run.a->n));
      run.head_hi = g.out_lo;
    }
    if (k == K - 1 && run.defer_tail) {
      // ... and the outputs that interpolate into the first sample behind the rank's hops need the next rank's head
      g.skip_tail = 1;
      g.out_hi = std::max(g.out_lo, std::min(g.out_hi, pv_first_output_at(c.hi * kPvHs - 1, run.r, run.a->n)));
      run.tail_lo = g.out_hi;
    }
    // the boundary between two chunks is finished in the left chunk's s: the right chunk copies it
    if (k > 0) g.prev_final = args[(size_t)k - 1].s + (args[(size_t)k - 1].frames - args[(size_t)k - 1].first) * kPvHs;
  }
  for (int64_t k = 0; k + 1 < K; ++k) args[(size_t)k].next_head = args[(size_t)k + 1].halo;  // the right chunk's head: its workgroup 0's halo

  // ---- the stages of one chunk ----
  // the constant-ratio plan rows of chunk k, on stream st (binary64 division and floor on the device: launch_pv_plan_const)
  auto plan_rows = [&](int64_t k, hipStream_t st) {
    const PvArgs &g = args[(size_t)k];
    const PvPipe::Plan &pl = p.plan[k % p.shape.plans];
    PV_TRY(launch_pv_plan_const(pl.apos, pl.hop, pl.hratio, g.frames, chunks[(size_t)k].lo - g.first, run.r, st));
  };
  // (the pipeline writes them three chunks ahead on the fix-up stream; only the rows of a run's first chunks, a marker plan's
  // and those of a rank's maps-only pass are made in front of their analysis)
  const bool plan_ahead = !run.plan && !run.totals_only;
  auto analysis = [&](int64_t k, hipStream_t sm) {  // (sm: the stream the transforms go on)
    const PvChunk c = chunks[(size_t)k];
    const PvArgs &g = args[(size_t)k];
    const PvPipe::Plan &pl = p.plan[k % p.shape.plans];
    if (run.plan) {
      const int64_t g0 = c.lo - g.first;  // global frame of local row 0
      PV_TRY(hipMemcpyAsync(pl.apos, run.plan->apos.data() + g0, (size_t)g.frames * 8, hipMemcpyHostToDevice, sm));
      PV_TRY(hipMemcpyAsync(pl.hop, run.plan_hop->data() + g0, (size_t)g.frames * 4, hipMemcpyHostToDevice, sm));
      PV_TRY(hipMemcpyAsync(pl.hratio, run.plan_hratio->data() + g0, (size_t)g.frames * 8, hipMemcpyHostToDevice, sm));
      // (the resampler's rows live with the chunk's stretched signal: the slot has a new tenant by the time it runs.  Its
      // last reader was the resampling of chunk k - 4 on the fix-up stream, queued at step k - 1 with an ev_fin behind it:
      // the event's latest record is that one when this is called)
      if (k >= p.shape.outs) PV_TRY(hipStreamWaitEvent(sm, p.ev_fin, 0));
      PV_TRY(hipMemcpyAsync(const_cast<double *>(g.tf), run.plan->tf.data() + c.lo, (size_t)(c.hi - c.lo) * 8, hipMemcpyHostToDevice, sm));
      PV_TRY(hipMemcpyAsync(const_cast<double *>(g.rf), run.plan->rf.data() + c.lo, (size_t)(c.hi - c.lo) * 8, hipMemcpyHostToDevice, sm));
      PV_TRY(hipMemcpyAsync(const_cast<int64_t *>(g.i0), run.plan->i0.data() + c.lo, (size_t)(c.hi - c.lo + 1) * 8, hipMemcpyHostToDevice, sm));
    } else if (!plan_ahead) {
      plan_rows(k, sm);
    }
    // (plan_ahead: the rows were written on the fix-up stream at chunk k - 3's step, in front of its ev_fin; the side stream
    // waited for that event before chunk k - 2's recurrence, whose ev_lock S(k - 2) waited for — and S(k - 2) is in front of
    // this launch on this stream: no wait of its own between the two big kernels)
    PV_TRY(launch_pv_analysis(g, sm));
    // (the side stream waits for S(k - 1), behind this launch on the stream, where there is one: one marker fewer between the
    // two big kernels)
    if (k == 0 || run.totals_only) PV_TRY(hipEventRecord(p.ev_an[k % p.shape.slots], sm));
  };
  auto synthesis = [&](int64_t k) {  // main stream
    const PvArgs &g = args[(size_t)k];
    PV_TRY(hipStreamWaitEvent(sm, p.ev_lock[k % p.shape.slots], 0));
    PV_TRY(launch_pv_synthesis(g, sm));
    if (k == 0 && run.defer_head) {
      PV_TRY(hipMemcpyAsync(p.head_raw, g.halo, kPvSeam * 4, hipMemcpyDeviceToDevice, sm));
      // (the sample behind the seam left the synthesis finished: hop 15 of the chunk's first workgroup)
      PV_TRY(hipMemcpyAsync(p.edge_head + kPvSeam, g.s + kPvSeam, 4, hipMemcpyDeviceToDevice, sm));
    }
    if (k == K - 1 && run.seams)  // the raw sums behind the rank's last hop (the fix-up normalises them in place)
      PV_TRY(hipMemcpyAsync(p.tail_raw, g.s + (g.frames - g.first) * kPvHs, kPvSeam * 4, hipMemcpyDeviceToDevice, sm));
    if (k == K - 1 && run.defer_tail)  // (the last sample of the rank's hops is finished too: the last workgroup's last hop)
      PV_TRY(hipMemcpyAsync(p.edge_tail, g.s + (g.frames - g.first) * kPvHs - 1, 4, hipMemcpyDeviceToDevice, sm));
    PV_TRY(hipEventRecord(p.ev_syn[k % p.shape.slots], sm));
  };

  if (!run.reuse_analysis) *p.rec_overflow = 0u;  // (host memory; nothing of an earlier call is in flight: every entry point joins its work)
  PV_TRY(hipEventRecord(p.ev_begin, sm));  // the input, and whatever used the arena before, are stream-ordered before this
  PV_TRY(hipStreamWaitEvent(ss, p.ev_begin, 0));
  PV_TRY(hipStreamWaitEvent(sf, p.ev_begin, 0));
  if (run.totals_only) {
    // stage 1 of a rank: transforms on the main stream, the maps (and the chunk's total map) beside the next chunk's
    for (int64_t k = 0; k < K && e == hipSuccess; ++k) {
      if (k >= p.shape.slots) PV_TRY(hipStreamWaitEvent(sm, p.ev_lock[k % p.shape.slots], 0));  // (the slot's maps are made)
      analysis(k, sm);
      PV_TRY(hipStreamWaitEvent(ss, p.ev_an[k % p.shape.slots], 0));
      PV_TRY(launch_pv_maps(args[(size_t)k], ss));
      PV_TRY(hipEventRecord(p.ev_lock[k % p.shape.slots], ss));
    }
  } else {
    // The main stream carries the two big kernels, one at a time:  A(0) A(1) S(0) A(2) S(1) A(3) S(2) ...  The side stream
    // carries everything small, beside an ANALYSIS: while A(k + 1) runs — S(k - 1) is through —, the records, maps and offsets
    // of chunk k, then the fix-up and resampling of chunk k - 2 (whose right neighbour's head S(k - 1) has just left).
    // Nothing runs beside a synthesis: its workgroups take a whole CU's LDS and registers, four to a CU, exactly one round
    // of them per chunk — a small kernel beside it displaces workgroups into a second round.
    if (plan_ahead && !run.reuse_analysis)
      for (int64_t k = 0; k < std::min<int64_t>(K, 3); ++k) plan_rows(k, sm);
    for (int64_t step = 0; step <= K && e == hipSuccess; ++step) {
      if (step < K && !run.reuse_analysis) analysis(step, sm);
      const int64_t j = step - 1;
      if (j < 0) continue;
      // side stream: chunk j's recurrence ...
      if (j >= 1) PV_TRY(hipStreamWaitEvent(ss, p.ev_syn[(j - 1) % p.shape.slots], 0));  // (behind it on the main stream: A(j) is done too)
      else if (!run.reuse_analysis) PV_TRY(hipStreamWaitEvent(ss, p.ev_an[j % p.shape.slots], 0));
      PvArgs gl = args[(size_t)j];
      gl.tot_sums = nullptr;
      gl.tot_org = nullptr;
      if (!run.reuse_analysis) PV_TRY(launch_pv_maps(gl, ss));
      PV_TRY(launch_pv_offsets(gl, ss));
      // the last hop of s is beyond every frame, and s[s_len] backs the interpolation's m + 1
      PV_TRY(hipMemsetAsync(gl.s + (gl.s_len - kPvHs), 0, (size_t)(kPvHs + 1) * 4, ss));
      PV_TRY(hipEventRecord(p.ev_lock[j % p.shape.slots], ss));
      // ... and, on a stream of its own (it must not hold the recurrence up, nor sit beside the synthesis the recurrence
      // releases): the plan rows of chunk j + 3 (their ring slot's last reader was chunk j - 1's maps, in front of S(j - 1)) and
      // chunk j - 2's fix-up and resampling, S(j - 1) being through
      if (j >= 1) PV_TRY(hipStreamWaitEvent(sf, p.ev_syn[(j - 1) % p.shape.slots], 0));
      if (plan_ahead && j + 3 < K) plan_rows(j + 3, sf);
      if (j >= 2) PV_TRY(launch_pv_finish(args[(size_t)j - 2], sf));
      PV_TRY(hipEventRecord(p.ev_fin, sf));
      // (S(j + 1) reuses a buffer the fix-up reads, A(j + 3) reads the plan rows: the next chunk's recurrence waits for both)
      PV_TRY(hipStreamWaitEvent(ss, p.ev_fin, 0));
      synthesis(j);
    }
    // the last two chunks' fix-up and resampling
    PV_TRY(hipStreamWaitEvent(sf, p.ev_syn[(K - 1) % p.shape.slots], 0));
    if (K >= 2) PV_TRY(launch_pv_finish(args[(size_t)K - 2], sf));
    PV_TRY(launch_pv_finish(args[(size_t)K - 1], sf));
    PV_TRY(hipEventRecord(p.ev_fin, sf));
    PV_TRY(hipStreamWaitEvent(sm, p.ev_fin, 0));  // everything joins the context's stream
  }
  if (e != hipSuccess) {
    hipStreamSynchronize(ss);
    hipStreamSynchronize(sf);
    hipStreamSynchronize(sm);
    return fail(MX_ERR_DEVICE, "phase vocoder: %s", hipGetErrorString(e));
  }
  return MX_OK;
}

int pv_run_in_arena(mx_ctx *ctx, int64_t frames, const std::function<int(PvPipe &)> &run) {
  for (int attempt = 0;; ++attempt) {
    PvPipe *p = nullptr;
    int rc = pv_pipe(ctx, frames, &p);
    if (rc) return rc;
    pv_shard_drop(*p);
    rc = run(*p);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (es != hipSuccess) return fail(MX_ERR_DEVICE, "phase vocoder: %s", hipGetErrorString(es));
    if (!pv_take_overflow(ctx, *p)) return MX_OK;
    // (more peaks than the compact record regions hold — an impulse train, noise —: once more, with full-size regions)
    if (attempt) return fail(MX_ERR_DEVICE, "phase vocoder: record regions overflowed at full size");
  }
}

}  // namespace mx

extern "C" {

int mx_pv_pitch_shift_dev(mx_ctx *ctx, const mx_audio *a, double semitones, float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_check(ctx, a)) return rc;
    if (!(semitones >= -48.0 && semitones <= 48.0)) return fail(MX_ERR_INVALID, "semitones out of range [-48, 48]");
    if (a->n == 0 || (!d_pcm_f32 && !d_pcm_i16)) return MX_OK;
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    PvRun run;
    run.a = a;
    run.r = std::pow(2.0, semitones / 12.0);
    run.F_lo = 0;
    run.F_hi = pv_frame_count(a->n, run.r);
    run.out_lo = 0;
    run.out_hi = a->n;
    run.pcm_f32 = d_pcm_f32;
    run.pcm_i16 = d_pcm_i16;
    return pv_run_in_arena(ctx, run.F_hi, [&](PvPipe &p) { return pv_run(ctx, p, run); });
  });
}

int mx_pv_pitch_shift(mx_ctx *ctx, const mx_audio *a, double semitones, float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_check(ctx, a)) return rc;
    if (a->n == 0 || (!pcm_f32_out && !pcm_i16_out)) return MX_OK;
    return pcm_to_host(ctx, a->n, pcm_f32_out, pcm_i16_out,
                       [&](float *d_f, int16_t *d_i) { return mx_pv_pitch_shift_dev(ctx, a, semitones, d_f, d_i); });
  });
}

// Marker-driven variant: the vocoder steered by the editor's markers as App::exportWav is (warped time, pitch bend).
int64_t mx_pv_render_length(int64_t n, int sampleRate, const mx_marker *markers, int nmarkers) {
  return mx_guard([&]() -> int64_t {
    if (n < 0 || nmarkers < 0 || (nmarkers > 0 && !markers)) return fail(MX_ERR_INVALID, "bad argument");
    PvPlan plan;
    std::string err;
    const int rc = build_pv_plan(markers, nmarkers, sampleRate, n, plan, err);
    if (rc) return fail(rc, "%s", err.c_str());
    return plan.n_out;
  });
}

int mx_pv_plan(int64_t n, int sampleRate, const mx_marker *markers, int nmarkers, int64_t **apos, double **tf,
               double **rf, int64_t **i0, int64_t *frames, int64_t *nsamples) {
  return mx_guard([&]() -> int {
    if (n < 0 || nmarkers < 0 || (nmarkers > 0 && !markers) || !apos || !tf || !rf || !i0 || !frames || !nsamples)
      return fail(MX_ERR_INVALID, "bad argument");
    PvPlan plan;
    std::string err;
    const int rc = build_pv_plan(markers, nmarkers, sampleRate, n, plan, err);
    if (rc) return fail(rc, "%s", err.c_str());
    const size_t F = plan.apos.size();
    HandOver h;
    h.add(apos, plan.apos.data(), F);
    h.add(i0, plan.i0.data(), F + 1);
    h.add(tf, plan.tf.data(), F);
    h.add(rf, plan.rf.data(), F);
    if (const int rc = h.give()) return rc;
    *frames = (int64_t)F;
    *nsamples = plan.n_out;
    return MX_OK;
  });
}

int mx_pv_render_dev(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_marker *markers, int nmarkers,
                     float *d_pcm_f32, int16_t *d_pcm_i16) {
  return mx_guard([&]() -> int {
    if (!ctx || !a || nmarkers < 0 || (nmarkers > 0 && !markers)) return fail(MX_ERR_INVALID, "bad argument");
    if (a->n == 0 || (!d_pcm_f32 && !d_pcm_i16)) return MX_OK;
    PvPlan plan;
    std::string err;
    int rc = build_pv_plan(markers, nmarkers, sampleRate, a->n, plan, err);
    if (rc) return fail(rc, "%s", err.c_str());
    if (plan.n_out == 0) return MX_OK;
    for (int64_t c : plan.apos)
      if (c < -(int64_t)MX_AUDIO_PAD / 2 || c > a->n + (int64_t)MX_AUDIO_PAD / 2)
        return fail(MX_ERR_INVALID, "a marker maps warped time outside the audio");
    // hops and stretch factors of the plan (the constant-ratio plan computes them on the device)
    const size_t F = plan.apos.size();
    std::vector<uint32_t> hop(F, 0u);
    std::vector<double> hratio(F, 0.0);
    for (size_t j = 1; j < F; ++j) {
      const int64_t h = plan.apos[j] - plan.apos[j - 1];
      if (h >= 1 && h <= 0x7fffffffLL) {
        hop[j] = (uint32_t)h;
        hratio[j] = (double)kPvHs / (double)h;
      }
    }
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    PvRun run;
    run.a = a;
    run.plan = &plan;
    run.plan_hop = &hop;
    run.plan_hratio = &hratio;
    run.sample_rate = sampleRate;
    run.F_lo = 0;
    run.F_hi = (int64_t)F;
    run.pcm_f32 = d_pcm_f32;
    run.pcm_i16 = d_pcm_i16;
    // (the plan's host arrays die with this frame: the run is joined before it returns)
    return pv_run_in_arena(ctx, (int64_t)F, [&](PvPipe &p) { return pv_run(ctx, p, run); });
  });
}

int mx_pv_render(mx_ctx *ctx, const mx_audio *a, int sampleRate, const mx_marker *markers, int nmarkers,
                 float *pcm_f32_out, int16_t *pcm_i16_out) {
  return mx_guard([&]() -> int {
    if (const int rc = handles_check(ctx, a)) return rc;
    const int64_t m = mx_pv_render_length(a->n, sampleRate, markers, nmarkers);
    if (m < 0) return (int)m;
    if (m == 0 || (!pcm_f32_out && !pcm_i16_out)) return MX_OK;
    return pcm_to_host(ctx, m, pcm_f32_out, pcm_i16_out, [&](float *d_f, int16_t *d_i) {
      return mx_pv_render_dev(ctx, a, sampleRate, markers, nmarkers, d_f, d_i);
    });
  });
}

}  // extern "C"
