// capi_pv_arena.cpp — the phase vocoder's work arena: its budget, shape, layout, build and release, and the entry points that
// set and report them.  One unit of the C-ABI implementation behind include/melonix_amd.h (see capi_internal.h, pv_pipe.h).
//
// The vocoder works inside a work arena with a memory BUDGET (round 6: mx_pv_set_arena_budget / MELONIX_PV_ARENA_MB; the
// default is a quarter of what the device has free at the context's first phase-vocoder call).  A call whose frames fit the
// budget is ONE chunk: its spectra stay resident between analysis and synthesis (one slot, 22 KiB per frame with the compact
// record regions: 17.9 GB for an hour at +3 st) and a rank of a multi-GPU run analyses its frames once.  What does not fit is
// walked CHUNK BY CHUNK (capi_pv.cpp), two slots alternating, with the longest chunk the budget holds (round 5: a fixed 32768
// frames whatever was free; rounds 1-4 laid the whole signal out at 41 KiB per frame and an 8-hour signal did not fit the GPU).
#include "pv_pipe.h"
#include "stft_tables.h"

using namespace mx;

namespace mx {

namespace {

constexpr PvShape pv_chunked(int64_t C, int rpf) { return PvShape{C, kPvSlots, kPvOutRing, kPvPlanRing, rpf}; }
constexpr PvShape pv_resident(int64_t C, int rpf) { return PvShape{C, 1, 1, 1, rpf}; }

size_t pv_layout(PvPipe &p, const PvShape &sh, char *base) {
  const int64_t C = sh.C;
  const int64_t rows = C + 32 + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return base ? base + o : nullptr;
  };
  p.hann = reinterpret_cast<float *>(take(kPvN * 4));
  p.hann_scaled = reinterpret_cast<float *>(take(kPvN * 4));
  p.wsplit = reinterpret_cast<float2 *>(take(kPvM * 8));
  // (a short chunk cuts its frame axis into fewer scan chunks than the cap: pv_run's scan_chunk is at least kPvMinScan frames)
  const size_t nmaps = (size_t)std::min<int64_t>(kPvMaxScanChunks, (rows + kPvMinScan - 1) / kPvMinScan) + 1, ngroups = (nmaps + 31) / 32;
  for (int i = 0; i < sh.plans; ++i) {
    PvPipe::Plan &pl = p.plan[i];
    pl.apos = reinterpret_cast<int64_t *>(take((size_t)rows * 8));
    pl.hop = reinterpret_cast<uint32_t *>(take((size_t)rows * 4));
    pl.hratio = reinterpret_cast<double *>(take((size_t)rows * 8));
  }
  for (int si = 0; si < sh.slots; ++si) {
    PvPipe::Slot &sl = p.slot[si];
    sl.xrows = reinterpret_cast<float2 *>(take((size_t)rows * kPvM * 8));
    // the record pool: one region per analysis workgroup (8 or 16 frames: rows rounded up to 16 covers either cut), rpf entries
    // per frame; + one row of slack (a walk's lanes past a row's count read entries nobody wrote — behind the last region too)
    sl.recs = reinterpret_cast<uint2 *>(take(((size_t)(rows + 16) * (size_t)sh.rpf + kPvM) * 8));
    sl.pkmap = reinterpret_cast<uint32_t *>(take((size_t)rows * (kPvM / 32) * 4));
    sl.pkcount = reinterpret_cast<uint32_t *>(take((size_t)rows * 4));
    sl.fthr = reinterpret_cast<float *>(take((size_t)rows * 4));
    sl.chunk_sums = reinterpret_cast<uint32_t *>(take(nmaps * kPvM * 4));
    sl.chunk_org = reinterpret_cast<uint16_t *>(take(nmaps * kPvM * 2));
    sl.group_sums = reinterpret_cast<uint32_t *>(take(ngroups * kPvM * 4));
    sl.group_org = reinterpret_cast<uint16_t *>(take(ngroups * kPvM * 2));
    sl.tot_sums = reinterpret_cast<uint32_t *>(take(kPvM * 4));
    sl.tot_org = reinterpret_cast<uint16_t *>(take(kPvM * 2));
  }
  for (int i = 0; i < sh.outs; ++i) {
    PvPipe::Out &o = p.out[i];
    o.halo = reinterpret_cast<float *>(take((size_t)pv_halo_floats(C + 32) * 4));
    o.s = reinterpret_cast<float *>(take(((size_t)(C + 32) * kPvHs + kPvN + 8) * 4));
    o.tf = reinterpret_cast<double *>(take((size_t)rows * 8));
    o.rf = reinterpret_cast<double *>(take((size_t)rows * 8));
    o.i0 = reinterpret_cast<int64_t *>(take((size_t)(rows + 1) * 8));
  }
  for (auto &c : p.carry) c = reinterpret_cast<uint32_t *>(take(kPvM * 4));
  p.carry_in = reinterpret_cast<uint32_t *>(take(kPvM * 4));
  p.carry_org = reinterpret_cast<uint16_t *>(take(kPvM * 2));
  p.prev_tail = reinterpret_cast<float *>(take(kPvSeam * 4));
  p.next_head = reinterpret_cast<float *>(take(kPvSeam * 4));
  p.head_raw = reinterpret_cast<float *>(take(kPvSeam * 4));
  p.tail_raw = reinterpret_cast<float *>(take(kPvSeam * 4));
  p.edge_head = reinterpret_cast<float *>(take((kPvSeam + 8) * 4));
  p.edge_tail = reinterpret_cast<float *>(take((kPvSeam + 8) * 4));
  return off;
}
size_t pv_shape_bytes(const PvShape &sh) {
  PvPipe tmp;
  return pv_layout(tmp, sh, nullptr);
}

// The budget: mx_pv_set_arena_budget, else MELONIX_PV_ARENA_MB, else a quarter of what the device had free when the context
// first needed an arena (taken once and kept until mx_ctx_release_scratch: a budget that followed the free memory call by call
// would rebuild the arena call by call).
int pv_budget(mx_ctx *ctx, size_t *out) {
  if (ctx->pv_budget_bytes > 0) {
    *out = (size_t)ctx->pv_budget_bytes;
    return MX_OK;
  }
  if (const char *e = getenv("MELONIX_PV_ARENA_MB")) {
    const long long mb = atoll(e);
    if (mb > 0) {
      *out = (size_t)mb << 20;
      return MX_OK;
    }
  }
  if (ctx->pv_budget_auto <= 0) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (ctx->pv) free_b += ctx->pv->bytes;  // (what the context holds already counts as available to it)
    ctx->pv_budget_auto = (int64_t)std::max<size_t>(free_b / 4, (size_t)64 << 20);
  }
  *out = (size_t)ctx->pv_budget_auto;
  return MX_OK;
}

// The shape of the arena a call over `frames` frames wants.  An explicit chunk length (mx_pv_set_chunk_frames /
// MELONIX_PV_CHUNK_FRAMES: tests that want many chunk boundaries in a short signal) is taken as it is, two slots (*pinned);
// otherwise one resident chunk if the budget holds the call's frames, else the longest chunks (multiples of 32 frames) two slots
// of which fit the budget.
int pv_shape_for(mx_ctx *ctx, int64_t frames, PvShape *out, bool *pinned) {
  int64_t C = ctx->pv_chunk_frames;
  if (C <= 0)
    if (const char *e = getenv("MELONIX_PV_CHUNK_FRAMES")) C = atoll(e);
  // (MELONIX_PV_FULL_RECORDS=1: full-size regions from the start — the A/B of the compact layout, tests/test_pv.py)
  const char *full_env = getenv("MELONIX_PV_FULL_RECORDS");
  const int rpf = (ctx->pv_rec_full || (full_env && full_env[0] == '1')) ? kPvM : kPvRecPerFrame;
  *pinned = C > 0;
  if (C > 0) {
    *out = pv_chunked(std::min<int64_t>(kPvMaxChunk, (C + 31) / 32 * 32), rpf);
    return MX_OK;
  }
  size_t budget = 0;
  const int rc = pv_budget(ctx, &budget);
  if (rc) return rc;
  const int64_t Fr = std::max<int64_t>(32, (frames + 31) / 32 * 32);
  if (pv_shape_bytes(pv_resident(Fr, rpf)) <= budget) {
    *out = pv_resident(Fr, rpf);
    return MX_OK;
  }
  // bytes are affine in C up to the 256-byte roundings: solve, then step down onto the budget
  const size_t b0 = pv_shape_bytes(pv_chunked(32, rpf)), b1 = pv_shape_bytes(pv_chunked(32 + 32 * 1024, rpf));
  if (b0 > budget)
    return fail(MX_ERR_NOMEM, "phase-vocoder arena budget of %zu MiB is below the %zu MiB the smallest chunks need", budget >> 20, (b0 >> 20) + 1);
  const double per32 = (double)(b1 - b0) / 1024.0;
  C = 32 + 32 * (int64_t)((double)(budget - b0) / per32);
  C = std::min<int64_t>(kPvMaxChunk, std::max<int64_t>(32, C));
  while (C > 32 && pv_shape_bytes(pv_chunked(C, rpf)) > budget) C -= 32;
  *out = pv_chunked(C, rpf);
  return MX_OK;
}

}  // namespace

// An arena that holds the call in one chunk is kept whatever it was made for; so is a chunked one of the wanted chunk length.
int pv_pipe(mx_ctx *ctx, int64_t frames, PvPipe **out) {
  HIP_TRY(hipSetDevice(ctx->device));  // HIP's current device is per thread
  PvShape want;
  bool pinned = false;
  int rc = pv_shape_for(ctx, frames, &want, &pinned);
  if (rc) return rc;
  if (ctx->pv) {
    const PvShape &have = ctx->pv->shape;
    const bool keep = pinned ? have == want : ((have.C >= (frames + 31) / 32 * 32 && have.rpf == want.rpf) || have == want);
    if (keep) {
      *out = ctx->pv;
      return MX_OK;
    }
  }
  pv_release(ctx);
  // the constants' host tables first: a failed allocation must not leave a half-built pipe behind (the next call would find an
  // arena of the wanted shape and use it)
  std::vector<float> hann((size_t)kPvN), hann_sc((size_t)kPvN);
  for (int j = 0; j < kPvN; ++j) {
    hann[(size_t)j] = (float)(0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * j / kPvN));
    hann_sc[(size_t)j] = hann[(size_t)j] * fold_scale(kPvN);  // exact: a power of two
  }
  std::vector<float2> wsplit((size_t)kPvM);
  for (int c = 0; c < kPvM; ++c) {
    const double ang = 2.0 * 3.14159265358979323846 * c / kPvN;
    wsplit[(size_t)c] = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  std::unique_ptr<PvPipe> p(new (std::nothrow) PvPipe());
  if (!p) return fail(MX_ERR_NOMEM, "out of host memory");
  p->shape = want;
  p->bytes = pv_layout(*p, want, nullptr);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < p->bytes)
    return fail(MX_ERR_NOMEM, "phase-vocoder work arena: %zu MiB needed for chunks of %lld frames, %zu MiB free", p->bytes >> 20,
                (long long)want.C, free_b >> 20);
  void *mem = nullptr;
  const hipError_t em = hipMalloc(&mem, p->bytes);
  if (em != hipSuccess) return fail(MX_ERR_NOMEM, "phase-vocoder work arena (%zu MiB): %s", p->bytes >> 20, hipGetErrorString(em));
  p->base = static_cast<char *>(mem);
  pv_layout(*p, want, p->base);
  ctx->pv = p.release();
  PvPipe &q = *ctx->pv;
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&q.rec_overflow), 64, hipHostMallocDefault);
  if (e == hipSuccess) *q.rec_overflow = 0u;
  if (e == hipSuccess) {
    // (what gets the side stream's small kernels through beside a transform is their WAVE priority — s_setprio in the
    // kernels: 0.5 ms per hour; the queue's priority measured nothing either way and is left at the default)
    e = hipStreamCreateWithFlags(&q.ss, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&q.sf, hipStreamNonBlocking);
  }
  hipEvent_t *const evs[] = {&q.ev_begin,  &q.ev_fin,     &q.ev_an[0],  &q.ev_an[1],
                             &q.ev_lock[0], &q.ev_lock[1], &q.ev_syn[0], &q.ev_syn[1]};
  static_assert(kPvSlots == 2, "the event list above names both slots");
  for (hipEvent_t *ev : evs)
    if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMemcpy(q.hann, hann.data(), kPvN * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q.hann_scaled, hann_sc.data(), kPvN * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q.wsplit, wsplit.data(), (size_t)kPvM * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    pv_release(ctx);
    return fail(MX_ERR_DEVICE, "phase vocoder setup: %s", hipGetErrorString(e));
  }
  *out = ctx->pv;
  return MX_OK;
}

// Behind a run whose work is complete (the caller has synchronised): did an analysis overflow its compact record regions?
// Then the run's results are void: the context switches to full-size regions for good (until its scratch is released), the
// arena goes back, and the caller repeats its run on the one pv_pipe builds next.
bool pv_take_overflow(mx_ctx *ctx, PvPipe &p) {
  if (!p.rec_overflow || *p.rec_overflow == 0u) return false;
  *p.rec_overflow = 0u;
  ctx->pv_rec_full = true;
  pv_release(ctx);
  return true;
}

void pv_shard_drop(PvPipe &p) {
  p.job_f.reset();
  p.job_i.reset();
  p.job = PvPipe::Shard{};
}

void pv_release(mx_ctx *ctx) {
  PvPipe *p = ctx->pv;
  if (!p) return;
  hipSetDevice(ctx->device);
  if (p->ss) hipStreamSynchronize(p->ss);
  if (p->sf) hipStreamSynchronize(p->sf);
  hipStreamSynchronize(ctx->stream);
  pv_shard_drop(*p);
  for (hipEvent_t ev : {p->ev_begin, p->ev_fin})
    if (ev) hipEventDestroy(ev);
  for (int i = 0; i < kPvSlots; ++i)
    for (hipEvent_t ev : {p->ev_an[i], p->ev_lock[i], p->ev_syn[i]})
      if (ev) hipEventDestroy(ev);
  if (p->ss) hipStreamDestroy(p->ss);
  if (p->sf) hipStreamDestroy(p->sf);
  hipFree(p->base);
  if (p->rec_overflow) hipHostFree(p->rec_overflow);
  delete p;
  ctx->pv = nullptr;
}

}  // namespace mx

extern "C" {

int mx_pv_set_chunk_frames(mx_ctx *ctx, int64_t frames) {
  return mx_guard([&]() -> int {
    if (!ctx || frames < 0) return fail(MX_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    ctx->pv_chunk_frames = frames;  // (the arena is rebuilt by the next call that needs another size)
    return MX_OK;
  });
}

int64_t mx_pv_arena_bytes(mx_ctx *ctx) {
  return mx_guard([&]() -> int64_t {
    if (!ctx) return fail(MX_ERR_INVALID, "null context");
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    return ctx->pv ? (int64_t)ctx->pv->bytes : 0;
  });
}

int mx_pv_set_arena_budget(mx_ctx *ctx, int64_t bytes) {
  return mx_guard([&]() -> int {
    if (!ctx || bytes < 0) return fail(MX_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    ctx->pv_budget_bytes = bytes;
    // (an arena above the new budget goes back now; one inside it is kept for as long as it serves)
    if (bytes > 0 && ctx->pv && ctx->pv->bytes > (size_t)bytes) pv_release(ctx);
    return MX_OK;
  });
}

int64_t mx_pv_arena_budget(mx_ctx *ctx) {
  return mx_guard([&]() -> int64_t {
    if (!ctx) return fail(MX_ERR_INVALID, "null context");
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t b = 0;
    const int rc = pv_budget(ctx, &b);
    return rc ? (int64_t)rc : (int64_t)b;
  });
}

int64_t mx_pv_last_chunks(mx_ctx *ctx) {
  return mx_guard([&]() -> int64_t {
    if (!ctx) return fail(MX_ERR_INVALID, "null context");
    std::lock_guard<std::mutex> plk(ctx->pv_mu);
    return ctx->pv ? ctx->pv->last_chunks : 0;
  });
}

}  // extern "C"
