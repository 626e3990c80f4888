// pv_pipe.h — what the three units of the phase vocoder share (capi_pv_arena.cpp: the arena's policy; capi_pv.cpp: the chunk
// pipeline and the single-GPU entry points; capi_pv_shard.cpp: the stages of one rank of a multi-GPU run).  Not installed.
#pragma once
#include <functional>

#include "capi_internal.h"

namespace mx {

constexpr int kPvN = 4096, kPvM = kPvN / 2, kPvHs = 256, kPvSeam = kPvN - kPvHs;
constexpr int64_t kPvMaxChunk = 1 << 22;
constexpr int kPvSlots = 2;  // (three or four buy nothing: profiles/timeline_r05_pv_pipeline.log)
constexpr int kPvPlanRing = 4;  // chunk k + 3's plan rows are written while chunk k - 1's are long read
constexpr int kPvOutRing = 4;  // chunk k's synthesis writes while chunk k - 2's fix-up reads k - 2, k - 1 (head) and k - 3 (boundary)
// Peak records: every analysis workgroup packs its frames' records into a region of its own of kPvRecPerFrame x (its frames)
// entries — a quarter of the 2048 a frame can have (an impulse): sweeps and music have tens to a few hundred peaks per frame,
// white noise ~410.  A run whose signal does not fit raises the overflow flag and is repeated, once, with full regions
// (kPvM per frame: cannot overflow); the context then stays with those until its scratch is released.
constexpr int kPvRecPerFrame = 512;
constexpr int kPvMinScan = 64;              // frames per scan chunk of the phase recurrence, at least
constexpr int64_t kPvMaxScanChunks = 1536;  // one round of row-walking workgroups, six per CU

// What an arena is made for: chunks of C frames (a multiple of 32; a slot has room for C + 32 frames and the row before them);
// `slots` sets of spectra + records (one: the call is a single chunk and its rows stay resident; two: chunks alternate), and the
// rings of the pipeline (one entry each where there is one chunk).  Chunk k uses slot k % slots, out k % outs, plan k % plans.
struct PvShape {
  int64_t C = 0;
  int slots = kPvSlots, outs = kPvOutRing, plans = kPvPlanRing;
  int rpf = kPvRecPerFrame;  // record capacity per frame of an analysis workgroup's region (kPvM: full)
  bool operator==(const PvShape &o) const { return C == o.C && slots == o.slots && outs == o.outs && plans == o.plans && rpf == o.rpf; }
};

struct PvPipe {
  PvShape shape;
  char *base = nullptr;
  size_t bytes = 0;
  // constants: the two windows, the split twiddles of the inverse transform
  float *hann = nullptr, *hann_scaled = nullptr;
  float2 *wsplit = nullptr;
  struct Plan {  // a chunk's analysis plan (positions, hops, stretch factors): written three chunks ahead, a ring of its own
    int64_t *apos;
    uint32_t *hop;
    double *hratio;
  } plan[kPvPlanRing] = {};
  struct Slot {  // what the analysis of a chunk leaves and its synthesis reads
    float2 *xrows;
    uint2 *recs;
    uint32_t *pkmap, *pkcount;
    float *fthr;
    uint32_t *chunk_sums, *group_sums, *tot_sums;
    uint16_t *chunk_org, *group_org, *tot_org;
  } slot[kPvSlots] = {};
  struct Out {  // what the synthesis of a chunk leaves and the fix-up / resampler read (+ the resampler's plan rows)
    float *halo, *s;
    double *tf, *rf;
    int64_t *i0;
  } out[kPvOutRing] = {};
  // [1] raised by an analysis whose record regions are too small for the signal: page-locked host memory the kernels write
  // through (once, on the rare overflow) and the host reads behind the call's synchronisation without another API call
  uint32_t *rec_overflow = nullptr;
  uint32_t *carry[2];  // the dense offset row behind chunk k's last frame: carry[k & 1]
  // one rank of a multi-GPU run: what it gets from its neighbours and owes them; carry_org: the source-bin row the carry's fold
  // from the gathered maps leaves behind (read by nobody)
  uint32_t *carry_in = nullptr;
  uint16_t *carry_org = nullptr;
  float *prev_tail = nullptr, *next_head = nullptr, *head_raw = nullptr, *tail_raw = nullptr, *edge_head = nullptr, *edge_tail = nullptr;
  hipStream_t ss = nullptr, sf = nullptr;  // the side streams: the recurrence; fix-up + resampling
  hipEvent_t ev_begin = nullptr, ev_fin = nullptr, ev_an[kPvSlots] = {}, ev_lock[kPvSlots] = {}, ev_syn[kPvSlots] = {};
  int64_t last_chunks = 0;  // chunks of the last run (mx_pv_last_chunks)
  // the staged job between mx_pv_shard_analyze and _finish
  struct Shard {
    bool active = false, first = false, last = false, single = false;
    int rank = 0, world = 1;
    const mx_audio *a = nullptr;
    double semitones = 0., r = 1.;
    int64_t F_lo = 0, F_hi = 0, out_lo = 0, out_hi = 0;
    bool synthesized = false;
    int64_t head_hi = 0, tail_lo = 0;  // the outputs [out_lo, head_hi) and [tail_lo, out_hi) wait for the neighbours' seams
    // the rank's outputs between stage 2 and stage 3 (device): the caller's buffers (_dev entry points) or job_f / job_i
    float *d_f = nullptr;
    int16_t *d_i = nullptr;
  } job;
  // the library's own PCM of the host-pointer rank stages (both formats: the caller chooses in stage 3); freed by pv_shard_drop
  DeviceArray<float> job_f;
  DeviceArray<int16_t> job_i;
};

// One run of the pipeline: the frames [F_lo, F_hi) of a signal of F frames.
struct PvRun {
  const mx_audio *a = nullptr;
  double r = 1.;                 // constant ratio (ignored with a plan)
  const PvPlan *plan = nullptr;  // marker-driven variant (whole signal only)
  const std::vector<uint32_t> *plan_hop = nullptr;
  const std::vector<double> *plan_hratio = nullptr;
  int sample_rate = 0;
  int64_t F_lo = 0, F_hi = 0;
  const uint32_t *carry_in = nullptr;  // device; null where the run starts at frame 0
  bool totals_only = false;            // stage 1 of a rank: analysis and maps, nothing synthesised
  uint32_t *totmaps_sums = nullptr;    // [chunks][M] per-chunk total maps (totals_only)
  uint16_t *totmaps_org = nullptr;
  bool reuse_analysis = false;         // the run is one chunk and slot 0 still holds its analysis (stage 2 behind stage 1)
  bool defer_head = false, defer_tail = false;  // a rank's edges wait for its neighbours' seams
  bool seams = false;                           // keep the raw sums behind the last hop (tail_raw)
  int64_t head_hi = 0, tail_lo = 0;             // out: the outputs [out_lo, head_hi) and [tail_lo, out_hi) were deferred
  float *pcm_f32 = nullptr;
  int16_t *pcm_i16 = nullptr;
  int64_t pcm_base = 0, out_lo = 0, out_hi = 0;
};

struct PvChunk {
  int64_t lo, hi;
};

#define PV_TRY(expr)                 \
  do {                               \
    if (e == hipSuccess) e = (expr); \
  } while (0)

// capi_pv_arena.cpp
// The pipe of the context for a call over `frames` frames, built (or rebuilt in another shape) on demand.  Caller holds ctx->pv_mu.
int pv_pipe(mx_ctx *ctx, int64_t frames, PvPipe **out);
// Behind a run whose work is complete: did an analysis overflow its compact record regions?  (Then the arena has gone back.)
bool pv_take_overflow(mx_ctx *ctx, PvPipe &p);
// ends the staged rank job and frees the library's own PCM
void pv_shard_drop(PvPipe &p);

// capi_pv.cpp
int64_t pv_frame_count(int64_t n, double r);
// smallest output sample whose interpolation base floor(i*r + N/2) reaches stretched sample q
int64_t pv_first_output_at(int64_t q, double r, int64_t n);
std::vector<PvChunk> pv_chunks_of(int64_t F_lo, int64_t F_hi, int64_t C);
int pv_run(mx_ctx *ctx, PvPipe &p, PvRun &run);
// An entry point's whole run over an arena that holds `frames` frames: `run(p)` on the arena (pv_run, and for stage 1 of a rank
// its chunk maps), joined, and repeated once on full-size record regions where an analysis overflowed the compact ones.
int pv_run_in_arena(mx_ctx *ctx, int64_t frames, const std::function<int(PvPipe &)> &run);

}  // namespace mx
