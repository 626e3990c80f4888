// capi_pv_shard.cpp — one rank of a multi-GPU phase-vocoder run (the overlap-add seams): its frame range and its
// three stages, each with a host-pointer and a device-pointer entry point.  One unit of the C-ABI implementation behind
// include/melonix_amd.h (see capi_internal.h, pv_pipe.h).
//
// Every rank holds the whole input and takes a contiguous range of the frame axis (boundaries on multiples of 32 frames = the
// synthesis workgroups, so the float sums group exactly as in a single-GPU run).  Two small exchanges happen outside this library
// (RCCL / gloo all-gathers in the caller): after stage 1 the per-rank phase totals (2048 x {restart, phase}), after stage 2 the
// seams (2 x 3840 raw partial sums).  A rank's range gets its arena by the same policy as a single-GPU call (capi_pv_arena.cpp):
// a range the budget holds is one resident chunk whose rows stay in the arena from stage 1 to stage 2, so it is analysed once
// (stage 2 = offsets + synthesis); a longer range is walked in chunks and analysed twice (stage 1 for the maps alone, stage 2
// again with the carry).
#include "pv_pipe.h"

using namespace mx;

extern "C" {

int mx_pv_shard_frames(int64_t n, double semitones, int rank, int world, int64_t *frame_lo, int64_t *frame_hi,
                       int64_t *out_lo, int64_t *out_hi) {
  return mx_guard([&]() -> int {
    if (n <= 0 || world < 1 || rank < 0 || rank >= world || !(semitones >= -48.0 && semitones <= 48.0))
      return fail(MX_ERR_INVALID, "bad argument");
    const double r = std::pow(2.0, semitones / 12.0);
    const int64_t F = pv_frame_count(n, r);
    int64_t per = (F + world - 1) / world;
    per = (per + 31) / 32 * 32;
    // (every rank gets at least one synthesis workgroup of its own: the seams either side of a rank must not overlap)
    if (world > 1 && F - per * (world - 1) < 32)
      return fail(MX_ERR_INVALID, "signal too short for %d ranks (%lld frames)", world, (long long)F);
    const int64_t lo = (int64_t)rank * per, hi = rank == world - 1 ? F : lo + per;
    if (frame_lo) *frame_lo = lo;
    if (frame_hi) *frame_hi = hi;
    if (out_lo) *out_lo = rank == 0 ? 0 : pv_first_output_at(lo * kPvHs, r, n);
    if (out_hi) *out_hi = rank == world - 1 ? n : pv_first_output_at(hi * kPvHs, r, n);
    return MX_OK;
  });
}

}  // extern "C"

// The three stages; the host-pointer entry points and the _dev entry points share them (copies go by hipMemcpyDefault).
//   stage 1 -> map_out: 2048 uint32 sums, then 2048 uint16 source bins (12 KiB: one rank's entry of the first all-gather)
static int pv_shard_analyze_core(mx_ctx *ctx, const mx_audio *a, double semitones, int rank, int world, void *map_out) {
  if (!ctx || !a || !map_out) return fail(MX_ERR_INVALID, "bad argument");
  int64_t lo, hi, olo, ohi;
  int rc = mx_pv_shard_frames(a->n, semitones, rank, world, &lo, &hi, &olo, &ohi);
  if (rc) return rc;
  std::lock_guard<std::mutex> plk(ctx->pv_mu);
  PvRun run;
  run.a = a;
  run.r = std::pow(2.0, semitones / 12.0);
  run.F_lo = lo;
  run.F_hi = hi;
  run.totals_only = true;
  int64_t K = 1;
  rc = pv_run_in_arena(ctx, hi - lo + 1, [&](PvPipe &p) -> int {  // (+ the row before the range)
    // every chunk's total map (12 KiB each), folded into the rank's behind the last analysis; a resident range has one: it is
    // written where it stays (no allocation on the way of a rank that fits its budget)
    K = (int64_t)pv_chunks_of(lo, hi, p.shape.C).size();
    DeviceArray<uint32_t> sums;
    DeviceArray<uint16_t> org;
    hipError_t e = sums.alloc(p.ss, K > 1 ? (size_t)K * kPvM : 0);
    if (e == hipSuccess) e = org.alloc(p.ss, K > 1 ? (size_t)K * kPvM : 0);
    if (e != hipSuccess) return fail(MX_ERR_NOMEM, "phase-vocoder chunk maps: %s", hipGetErrorString(e));
    run.totmaps_sums = K > 1 ? sums.p : p.slot[0].tot_sums;
    run.totmaps_org = K > 1 ? org.p : p.slot[0].tot_org;
    if (const int st = pv_run(ctx, p, run)) return st;
    if (K > 1) PV_TRY(launch_pv_compose_maps(sums.p, org.p, K, p.slot[0].tot_sums, p.slot[0].tot_org, p.ss));
    PV_TRY(hipMemcpyAsync(map_out, p.slot[0].tot_sums, kPvM * 4, hipMemcpyDefault, p.ss));
    PV_TRY(hipMemcpyAsync(static_cast<char *>(map_out) + kPvM * 4, p.slot[0].tot_org, kPvM * 2, hipMemcpyDefault, p.ss));
    const hipError_t es = hipStreamSynchronize(p.ss);
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? MX_OK : fail(MX_ERR_DEVICE, "phase vocoder (analysis): %s", hipGetErrorString(e));
  });
  if (rc) return rc;
  PvPipe::Shard &j = ctx->pv->job;
  j.active = true;
  j.rank = rank;
  j.world = world;
  j.first = rank == 0;
  j.last = rank == world - 1;
  j.single = K == 1;  // the rows are resident: stage 2 goes straight to the offsets and the synthesis
  j.a = a;
  j.semitones = semitones;
  j.r = run.r;
  j.F_lo = lo;
  j.F_hi = hi;
  j.out_lo = olo;
  j.out_hi = ohi;
  return MX_OK;
}

//   stage 2: the carry into the rank — a host row (carry), or folded here from the gathered maps of the ranks below (d_maps_all:
//   [world] x 12 KiB as stage 1 wrote them) -> the rank's outputs but its edges, and its two seams (head then tail, 2 x 3840
//   floats: one rank's entry of the second all-gather)
static int pv_shard_synthesize_core(mx_ctx *ctx, const uint32_t *carry, const void *d_maps_all, float *d_pcm_f32, int16_t *d_pcm_i16,
                                    bool own_pcm, float *head_out, float *tail_out) {
  if (!ctx || !head_out || !tail_out) return fail(MX_ERR_INVALID, "bad argument");
  std::lock_guard<std::mutex> plk(ctx->pv_mu);
  PvPipe *p = ctx->pv;
  if (!p || !p->job.active || p->job.synthesized) return fail(MX_ERR_INVALID, "mx_pv_shard_analyze has not run on this context");
  PvPipe::Shard &j = p->job;
  if (!j.first && !carry && !d_maps_all) return fail(MX_ERR_INVALID, "carry_in is required on every rank but the first");
  if (!own_pcm && !d_pcm_f32 && !d_pcm_i16) return fail(MX_ERR_INVALID, "no output buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t sm = ctx->stream;
  const int64_t cnt = j.out_hi - j.out_lo;
  hipError_t e = hipSuccess;
  auto drop = [&](int rc) {  // (a failed stage ends the job, behind whatever it queued)
    hipStreamSynchronize(sm);
    pv_shard_drop(*p);
    return rc;
  };
  // the carry first: nothing is allocated yet if it cannot be had
  if (!j.first) {
    if (d_maps_all) {
      // the maps of ranks 0 .. rank - 1 composed in order and applied to a zero row: the composed map's sums (a bin whose
      // source is a bin of the zero row ends at its sum; so does one that restarted) — read where the all-gather left them,
      // one 8 KiB sums row and one 4 KiB source-bin row per rank
      constexpr int kEntry = kPvM * 6;
      const uint32_t *ms = static_cast<const uint32_t *>(d_maps_all);
      const uint16_t *mo = reinterpret_cast<const uint16_t *>(static_cast<const char *>(d_maps_all) + (size_t)kPvM * 4);
      PV_TRY(launch_pv_compose_maps(ms, mo, j.rank, p->carry_in, p->carry_org, sm, kEntry / 4, kEntry / 2));
    } else {
      PV_TRY(hipMemcpyAsync(p->carry_in, carry, kPvM * 4, hipMemcpyHostToDevice, sm));
    }
    if (e != hipSuccess) return drop(fail(MX_ERR_DEVICE, "phase vocoder (carry): %s", hipGetErrorString(e)));
  }
  // the rank's outputs wait on the device for stage 3: in the caller's buffers, or (host-pointer entry points: the caller
  // chooses the formats in stage 3) in buffers of the library's own, both formats
  if (own_pcm) {
    e = p->job_f.alloc(sm, (size_t)cnt);
    if (e == hipSuccess) e = p->job_i.alloc(sm, (size_t)cnt);
    if (e != hipSuccess) return drop(fail(MX_ERR_NOMEM, "device PCM buffers: %s", hipGetErrorString(e)));
    j.d_f = p->job_f.p;
    j.d_i = p->job_i.p;
  } else {
    j.d_f = d_pcm_f32;
    j.d_i = d_pcm_i16;
  }
  PvRun run;
  run.a = j.a;
  run.r = j.r;
  run.F_lo = j.F_lo;
  run.F_hi = j.F_hi;
  run.carry_in = j.first ? nullptr : p->carry_in;
  run.reuse_analysis = j.single;
  run.defer_head = !j.first;
  run.defer_tail = !j.last;
  run.seams = true;
  run.pcm_f32 = j.d_f;
  run.pcm_i16 = j.d_i;
  run.pcm_base = j.out_lo;
  run.out_lo = run.head_hi = j.out_lo;
  run.out_hi = run.tail_lo = j.out_hi;
  int rc = pv_run(ctx, *p, run);
  // the seams, raw: this rank's sums into the N - Hs samples before its first complete hop (all zero on the first rank,
  // whose first hops are complete) and after its last hop
  if (rc == MX_OK) {
    if (j.first) PV_TRY(hipMemsetAsync(p->head_raw, 0, kPvSeam * 4, sm));
    PV_TRY(hipMemcpyAsync(head_out, p->head_raw, kPvSeam * 4, hipMemcpyDefault, sm));
    PV_TRY(hipMemcpyAsync(tail_out, p->tail_raw, kPvSeam * 4, hipMemcpyDefault, sm));
  }
  const hipError_t es = hipStreamSynchronize(sm);
  if (rc == MX_OK && e == hipSuccess) e = es;
  if (rc || e != hipSuccess) return drop(rc ? rc : fail(MX_ERR_DEVICE, "phase vocoder (synthesis): %s", hipGetErrorString(e)));
  if (*p->rec_overflow != 0u)  // (a chunked range analyses again here, cut as in stage 1, which passed: cannot happen)
    return drop(fail(MX_ERR_DEVICE, "phase vocoder (synthesis): record regions overflowed behind a stage 1 that fitted"));
  j.synthesized = true;
  j.head_hi = run.head_hi;
  j.tail_lo = run.tail_lo;
  return MX_OK;
}

//   stage 3: the neighbours' seams (host rows, or device rows: entries of the gathered seams) -> the rank's edge outputs
static int pv_shard_finish_core(mx_ctx *ctx, const float *prev_tail, const float *next_head, const void *d_seams_all,
                                float *pcm_f32_out, int16_t *pcm_i16_out) {
  if (!ctx) return fail(MX_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> plk(ctx->pv_mu);
  PvPipe *p = ctx->pv;
  if (!p || !p->job.active || !p->job.synthesized) return fail(MX_ERR_INVALID, "mx_pv_shard_synthesize has not run on this context");
  PvPipe::Shard &j = p->job;
  if (d_seams_all) {  // [world] x {head, tail} x 3840 floats, as stage 2 wrote them
    const float *all = static_cast<const float *>(d_seams_all);
    prev_tail = j.first ? nullptr : all + ((size_t)(j.rank - 1) * 2 + 1) * kPvSeam;
    next_head = j.last ? nullptr : all + (size_t)(j.rank + 1) * 2 * kPvSeam;
  }
  if ((!j.first && !prev_tail) || (!j.last && !next_head)) return fail(MX_ERR_INVALID, "a neighbour's seam is missing");
  HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t sm = ctx->stream;
  hipError_t e = hipSuccess;
  PvArgs g{};
  g.ratio = j.r;
  g.pcm_f32 = j.d_f;
  g.pcm_i16 = j.d_i;
  g.pcm_base = j.out_lo;
  if (!j.first) {
    // the rank's first N - Hs stretched samples: its head + the previous rank's tail, then their outputs
    PV_TRY(hipMemcpyAsync(p->prev_tail, prev_tail, kPvSeam * 4, hipMemcpyDefault, sm));
    PV_TRY(launch_pv_edge_sum(p->edge_head, p->prev_tail, p->head_raw, kPvSeam, sm));  // left + right, as pv_fixup
    g.s = p->edge_head;
    g.s_origin = j.F_lo * kPvHs;
    g.out_lo = j.out_lo;
    g.out_hi = j.head_hi;
    PV_TRY(launch_pv_resample(g, sm));
  }
  if (!j.last) {
    // the outputs that interpolate between the rank's last stretched sample and the first one behind it
    PV_TRY(hipMemcpyAsync(p->next_head, next_head, kPvSeam * 4, hipMemcpyDefault, sm));
    PV_TRY(launch_pv_edge_sum(p->edge_tail + 1, p->tail_raw, p->next_head, 4, sm));
    g.s = p->edge_tail;
    g.s_origin = j.F_hi * kPvHs - 1;
    g.out_lo = j.tail_lo;
    g.out_hi = j.out_hi;
    PV_TRY(launch_pv_resample(g, sm));
  }
  // (the library's own PCM of the host-pointer form; nothing where the outputs are the caller's)
  PV_TRY(p->job_f.download(pcm_f32_out));
  PV_TRY(p->job_i.download(pcm_i16_out));
  const hipError_t es = hipStreamSynchronize(sm);
  if (e == hipSuccess) e = es;
  pv_shard_drop(*p);
  if (e != hipSuccess) return fail(MX_ERR_DEVICE, "phase vocoder (finish): %s", hipGetErrorString(e));
  return MX_OK;
}

extern "C" {

int mx_pv_shard_analyze(mx_ctx *ctx, const mx_audio *a, double semitones, int rank, int world, uint32_t *tot_sums_out,
                        uint16_t *tot_org_out) {
  return mx_guard([&] {
    if (!tot_sums_out || !tot_org_out) return fail(MX_ERR_INVALID, "bad argument");
    // (the two host arrays need not be adjacent: through one 12 KiB landing buffer)
    std::vector<uint32_t> map((size_t)kPvM * 6 / 4);
    const int rc = pv_shard_analyze_core(ctx, a, semitones, rank, world, map.data());
    if (rc) return rc;
    memcpy(tot_sums_out, map.data(), (size_t)kPvM * 4);
    memcpy(tot_org_out, map.data() + kPvM, (size_t)kPvM * 2);
    return MX_OK;
  });
}
int mx_pv_shard_synthesize(mx_ctx *ctx, const uint32_t *carry_in, float *head_out, float *tail_out) {
  return mx_guard([&] { return pv_shard_synthesize_core(ctx, carry_in, nullptr, nullptr, nullptr, true, head_out, tail_out); });
}
int mx_pv_shard_finish(mx_ctx *ctx, const float *prev_tail, const float *next_head, float *pcm_f32_out,
                       int16_t *pcm_i16_out) {
  return mx_guard([&] { return pv_shard_finish_core(ctx, prev_tail, next_head, nullptr, pcm_f32_out, pcm_i16_out); });
}

// The same three stages with everything a rank exchanges left on the device, laid out as the two all-gathers move it: stage 1
// writes the rank's 12 KiB entry of the maps, stage 2 reads the gathered maps ([world] entries; it folds those of the ranks below
// into its carry on the device) and writes the rank's 30 KiB entry of the seams, stage 3 reads the gathered seams.  The rank's
// PCM goes straight into the caller's device buffers (out_hi - out_lo samples, either may be NULL) from stage 2 on.
int mx_pv_shard_analyze_dev(mx_ctx *ctx, const mx_audio *a, double semitones, int rank, int world, void *d_map_out) {
  return mx_guard([&] { return pv_shard_analyze_core(ctx, a, semitones, rank, world, d_map_out); });
}
int mx_pv_shard_synthesize_dev(mx_ctx *ctx, const void *d_maps_all, float *d_pcm_f32, int16_t *d_pcm_i16, void *d_seams_out) {
  return mx_guard([&] {
    if (!d_seams_out || !d_maps_all) return fail(MX_ERR_INVALID, "bad argument");
    float *seams = static_cast<float *>(d_seams_out);
    return pv_shard_synthesize_core(ctx, nullptr, d_maps_all, d_pcm_f32, d_pcm_i16, false, seams, seams + kPvSeam);
  });
}
int mx_pv_shard_finish_dev(mx_ctx *ctx, const void *d_seams_all) {
  return mx_guard([&] {
    if (!d_seams_all) return fail(MX_ERR_INVALID, "bad argument");
    return pv_shard_finish_core(ctx, nullptr, nullptr, d_seams_all, nullptr, nullptr);
  });
}

}  // extern "C"
