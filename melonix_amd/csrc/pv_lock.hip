// pv_lock.hip — the phase vocoder's recurrence over the peak records: pv_lock_walk, pv_lock_chunks (the stages: pv_common.h).
#include "pv_common.h"

namespace mx {
namespace {

// ---- the recurrence over the peak records ---------------------------------------------------------------------------
// State after row r, at the bins that are peaks of row r: whether the peak continued (a bit map) and, if so, its offset
// C_r[p] — as a value (APPLY) or as a map entry (source bin at the chunk's start | none, sum of deltas).  Row r + 1 looks
// its peaks' predecessors up in that state: E_r[p] = C_r[q] if q (the owner of bin p in row r: in the record) is valid and
// continued, else 0.  The FIRST row of a chunk takes E from the dense row the chunk starts from instead (every bin has an
// entry there: the identity map, or the offsets pv_lock_chunks computed), and the chunk's composed map is made dense again
// after its last row (every bin's owner in that row).
// APPLY = false: the chunk's composed map -> chunk_org / chunk_sums.  APPLY = true: chunk_sums holds the offsets at the
// chunk's start; the peaks' offsets are written in record order (0 for a peak that restarts: its bins keep their phases).
constexpr int kLockT = 128;
template <bool APPLY>
__global__ __launch_bounds__(kLockT) void pv_lock_walk(const PvArgs a) {
  MX_LATENCY_BOUND_KERNEL();
  constexpr int W = kPvM / 32;
  __shared__ uint32_t SUM[2][kPvM];
  __shared__ uint16_t ORG[APPLY ? 1 : 2][APPLY ? 2 : kPvM];
  __shared__ uint32_t CM[3][W];      // bit p: peak p of that row continued (this row's, the previous row's, the one being cleared)
  __shared__ uint32_t pkw[W + 2];    // (chunk end) the last row's peak map, a zero word either side
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int64_t r0 = a.first + c * a.scan_chunk, r1 = r0 + a.scan_chunk < a.frames ? r0 + a.scan_chunk : a.frames;
  if constexpr (APPLY) {
    for (int k = t; k < kPvM; k += kLockT) SUM[1][k] = a.chunk_sums[c * kPvM + k];  // E at the chunk's start
  }
  if (t < W) CM[0][t] = CM[1][t] = 0u;
  int cur = 0;     // SUM / ORG: the row being written; cur ^ 1: the previous row's state
  int cw = 0;      // CM: this row's map; (cw + 2) % 3 the previous row's; (cw + 1) % 3 is cleared for the next row
  // Rows are a few dozen records each and a row's work is a handful of LDS operations: what a row costs is the latency of
  // its records' load.  They are requested kAhead rows ahead (counts and each thread's first record, a register ring).
  constexpr int kAhead = 4;
  uint32_t cn[kAhead];
  uint2 rn[kAhead];
  // (a row's count and the place of its records are one word, pkcount[row]: the words run one block further ahead than the
  // records they address — iq: those of the block in rn, in_: those of the block behind it — so a record load never waits
  // for its address)
  uint32_t iq[kAhead], in_[kAhead];
  // (unconditional loads — a row past the chunk reads the chunk's last row again, a thread past the row's count reads an
  // entry nobody wrote: neither is used — so that the compiler can count them: behind a branch every wait becomes vmcnt(0)
  // and the ring hides nothing)
  auto info_of = [&](int64_t rr) { return a.pkcount[rr < r1 ? rr : r1 - 1]; };
  auto request = [&](int64_t rr, uint32_t info, uint32_t &cnt_, uint2 &rec_) {
    const int64_t rq = rr < r1 ? rr : r1 - 1;
    cnt_ = rr < r1 ? (info & kPkCountMask) : 0u;
    rec_ = a.recs[pv_rec_start(a, rq, info) + t];
  };
#pragma unroll
  for (int j = 0; j < kAhead; ++j) {
    iq[j] = info_of(r0 + j);
    in_[j] = info_of(r0 + kAhead + j);
  }
#pragma unroll
  for (int j = 0; j < kAhead; ++j) request(r0 + j, iq[j], cn[j], rn[j]);
  __syncthreads();
  for (int64_t rb = r0; rb < r1; rb += kAhead) {
    uint32_t cc[kAhead], ic[kAhead];
    uint2 rc[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      cc[j] = cn[j];
      rc[j] = rn[j];
      ic[j] = iq[j];
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      iq[j] = in_[j];
      request(rb + kAhead + j, iq[j], cn[j], rn[j]);
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) in_[j] = info_of(rb + 2 * kAhead + j);
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const int64_t r = rb + j;
      if (r >= r1) break;  // (block-uniform)
      const int cnt = (int)cc[j];
      uint2 rec = rc[j];
      uint2 *rrow = a.recs + pv_rec_start(a, r, ic[j]);
      const int cp = cw == 0 ? 2 : cw - 1, cx = cw == 2 ? 0 : cw + 1;
      if (t < W) CM[cx][t] = 0u;  // (last read during the previous row, before the barrier that ended it)
      for (int i = t; i < cnt; i += kLockT) {
        if (i != t) rec = rrow[i];
        const int p = (int)(rec.x & 2047u);
        const bool cont = (rec.x & kRecCont) != 0u;
        uint32_t val = 0u;
        uint16_t org = kPvNoBin;
        if (cont) {
          if (r == r0) {  // from the dense row the chunk starts from
            val = (APPLY ? SUM[cur ^ 1][p] : 0u) + rec.y;
            org = (uint16_t)p;
          } else {
            const int q = (int)((rec.x >> 11) & 2047u);
            const bool link = (rec.x & kRecQValid) != 0u && ((CM[cp][q >> 5] >> (q & 31)) & 1u) != 0u;
            val = (link ? SUM[cur ^ 1][q] : 0u) + rec.y;
            if constexpr (!APPLY) org = link ? ORG[cur ^ 1][q] : kPvNoBin;
          }
          SUM[cur][p] = val;
          if constexpr (!APPLY) ORG[cur][p] = org;
          atomicOr(&CM[cw][p >> 5], 1u << (p & 31));
        }
        if constexpr (APPLY) rrow[i].y = val;  // (0 where the peak restarts; the delta it replaces has no reader left)
      }
      __syncthreads();  // row r's state is complete; nobody reads row r-1's any more
      cur ^= 1;
      cw = cx;
    }
  }
  if constexpr (!APPLY) {
    // the chunk's map, dense: bin k ends the chunk with its owner's entry (or restarted: no owner, or an owner that did not
    // continue).  cur ^ 1 (SUM / ORG) and the map before cw hold the last row's state.
    const int cl = cw == 0 ? 2 : cw - 1;
    const int64_t rl = r1 - 1;
    if (t < W) pkw[t + 1] = r1 > r0 ? a.pkmap[(size_t)rl * W + t] : 0u;
    if (t < 2) pkw[t ? W + 1 : 0] = 0u;
    __syncthreads();
    for (int k = t; k < kPvM; k += kLockT) {
      const int o = pv_owner(&pkw[1], k);
      const bool ok = o != (int)kPvNoBin && ((CM[cl][o >> 5] >> (o & 31)) & 1u) != 0u;
      a.chunk_sums[c * kPvM + k] = ok ? SUM[cur ^ 1][o] : 0u;
      a.chunk_org[c * kPvM + k] = ok ? ORG[cur ^ 1][o] : kPvNoBin;
    }
  }
}

// Composition of chunk maps, in order (two bins per thread, one barrier per map).  One workgroup composes the maps
// sums[n0 .. n0 + cnt) / org[...] of its group, n0 = blockIdx.x * per_group:
// MAP = false: the offsets every map of the group starts from, beginning with init (+ blockIdx.x * M when init_per_group;
//              null: zeros) — they REPLACE the map's delta row.
// MAP = true:  the group's composed map -> out_sums / out_org [blockIdx.x][M]; the maps stay.
// The frame axis is cut into ~1536 chunks (one round of row-walking workgroups: what a walk costs is rows x latency), so
// their composition is two-level: groups of kPvGroup chunk maps in parallel (MAP = true), one pass over the group maps
// (MAP = false: group-start offsets, from carry_in — the offset row at the end of the previous rank's last frame,
// irrelevant for the rank that holds frame 0, which restarts every bin; MAP = true: this rank's total map, what the
// other ranks need to know of it), then the groups again in parallel from their start offsets (MAP = false).
constexpr int kChunkT = 1024, kChunkV = kPvM / kChunkT;
constexpr int kPvGroup = 32;
template <bool MAP>
__global__ __launch_bounds__(kChunkT) void pv_lock_chunks(uint32_t *sums, uint16_t *org, int64_t n, int per_group,
                                                          const uint32_t *init, int init_per_group, uint32_t *out_sums,
                                                          uint16_t *out_org, uint32_t *final_out, int s_stride = kPvM,
                                                          int o_stride = kPvM) {
  // (s_stride / o_stride: elements from one map's row to the next — kPvM where the maps are two dense arrays; the gathered
  // rank maps of a multi-GPU run interleave a 8 KiB sums row and a 4 KiB source-bin row per rank)
  MX_LATENCY_BOUND_KERNEL();
  __shared__ uint32_t D[2][kPvM];
  __shared__ uint16_t O[MAP ? 2 : 1][MAP ? kPvM : 2];
  const int t = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * per_group;
  const int64_t cnt = n0 + per_group < n ? per_group : n - n0;
  sums += n0 * s_stride;
  org += n0 * o_stride;
  if (init && init_per_group) init += (int64_t)blockIdx.x * kPvM;
  uint32_t sd[kChunkV];
  uint16_t so[kChunkV];
#pragma unroll
  for (int j = 0; j < kChunkV; ++j) {
    const int k = t + kChunkT * j;
    sd[j] = MAP ? 0u : (init ? init[k] : 0u);
    so[j] = (uint16_t)k;
    D[0][k] = sd[j];
    if constexpr (MAP) O[0][k] = so[j];
  }
  int cur = 0;
  uint32_t nd[kChunkV];
  uint16_t no[kChunkV];
#pragma unroll
  for (int j = 0; j < kChunkV; ++j) {
    nd[j] = cnt > 0 ? sums[t + kChunkT * j] : 0u;
    no[j] = cnt > 0 ? org[t + kChunkT * j] : kPvNoBin;
  }
  for (int64_t c = 0; c < cnt; ++c) {
    __syncthreads();
    uint32_t cd[kChunkV];
    uint16_t co[kChunkV];
#pragma unroll
    for (int j = 0; j < kChunkV; ++j) { cd[j] = nd[j]; co[j] = no[j]; }
    if (c + 1 < cnt) {
#pragma unroll
      for (int j = 0; j < kChunkV; ++j) {
        nd[j] = sums[(c + 1) * s_stride + t + kChunkT * j];
        no[j] = org[(c + 1) * o_stride + t + kChunkT * j];
      }
    }
#pragma unroll
    for (int j = 0; j < kChunkV; ++j) {
      const int k = t + kChunkT * j;
      if constexpr (!MAP) sums[c * s_stride + k] = sd[j];  // the offsets this map starts from
      if (co[j] == kPvNoBin) {
        sd[j] = cd[j];
        so[j] = kPvNoBin;
      } else {
        sd[j] = D[cur][co[j]] + cd[j];
        if constexpr (MAP) so[j] = O[cur][co[j]];
      }
      D[cur ^ 1][k] = sd[j];
      if constexpr (MAP) O[cur ^ 1][k] = so[j];
    }
    cur ^= 1;
  }
  if constexpr (MAP) {
#pragma unroll
    for (int j = 0; j < kChunkV; ++j) {
      out_sums[(int64_t)blockIdx.x * kPvM + t + kChunkT * j] = sd[j];
      out_org[(int64_t)blockIdx.x * kPvM + t + kChunkT * j] = so[j];
    }
  } else if (final_out) {  // (single-workgroup pass) the offsets behind the last map: what the next range starts from
#pragma unroll
    for (int j = 0; j < kChunkV; ++j) final_out[t + kChunkT * j] = sd[j];
  }
}

// the group maps of the chunk maps (chunk_sums / chunk_org stay as they are)
void launch_group_maps(const PvArgs &a, int64_t nchunks, hipStream_t s) {
  const unsigned G = (unsigned)((nchunks + kPvGroup - 1) / kPvGroup);
  hipLaunchKernelGGL(pv_lock_chunks<true>, dim3(G), dim3(kChunkT), 0, s, a.chunk_sums, a.chunk_org, nchunks, kPvGroup,
                     (const uint32_t *)nullptr, 0, a.group_sums, a.group_org, (uint32_t *)nullptr);
}
}  // namespace

hipError_t launch_pv_maps(const PvArgs &a, hipStream_t s) {
  if (a.frames - a.first <= 0) return hipSuccess;
  const int64_t nchunks = pv_chunks(a);
  if (const hipError_t e = launch_pv_heads(a, s); e != hipSuccess) return e;
  hipLaunchKernelGGL(pv_lock_walk<false>, dim3((unsigned)nchunks), dim3(kLockT), 0, s, a);
  launch_group_maps(a, nchunks, s);
  if (a.tot_sums) {  // this range's total map: the composition of its group maps
    const int64_t G = (nchunks + kPvGroup - 1) / kPvGroup;
    hipLaunchKernelGGL(pv_lock_chunks<true>, dim3(1), dim3(kChunkT), 0, s, a.group_sums, a.group_org, G, (int)G,
                       (const uint32_t *)nullptr, 0, a.tot_sums, a.tot_org, (uint32_t *)nullptr);
  }
  return hipGetLastError();
}
hipError_t launch_pv_offsets(const PvArgs &a, hipStream_t s) {
  if (a.frames - a.first <= 0) return hipSuccess;
  const int64_t nchunks = pv_chunks(a);
  const int64_t G = (nchunks + kPvGroup - 1) / kPvGroup;
  // the offsets every group starts from (they replace the group maps' delta rows) ...
  hipLaunchKernelGGL(pv_lock_chunks<false>, dim3(1), dim3(kChunkT), 0, s, a.group_sums, a.group_org, G, (int)G, a.carry_in, 0,
                     (uint32_t *)nullptr, (uint16_t *)nullptr, a.carry_out);
  // ... and, from those, the offsets every chunk starts from
  hipLaunchKernelGGL(pv_lock_chunks<false>, dim3((unsigned)G), dim3(kChunkT), 0, s, a.chunk_sums, a.chunk_org, nchunks, kPvGroup,
                     (const uint32_t *)a.group_sums, 1, (uint32_t *)nullptr, (uint16_t *)nullptr, (uint32_t *)nullptr);
  hipLaunchKernelGGL(pv_lock_walk<true>, dim3((unsigned)nchunks), dim3(kLockT), 0, s, a);
  return hipGetLastError();
}
// The composition, in order, of n maps (sums / org [n][N/2]) -> out_sums / out_org [N/2]: a rank that walks its frames chunk
// by chunk keeps every chunk's total map (12 KiB) and folds them into the rank's here.
hipError_t launch_pv_compose_maps(const uint32_t *sums, const uint16_t *org, int64_t n, uint32_t *out_sums, uint16_t *out_org, hipStream_t s,
                                  int sums_stride, int org_stride) {
  if (n <= 0 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  // (MAP = true reads the maps only)
  hipLaunchKernelGGL(pv_lock_chunks<true>, dim3(1), dim3(kChunkT), 0, s, const_cast<uint32_t *>(sums), const_cast<uint16_t *>(org), n, (int)n,
                     (const uint32_t *)nullptr, 0, out_sums, out_org, (uint32_t *)nullptr, sums_stride > 0 ? sums_stride : kPvM,
                     org_stride > 0 ? org_stride : kPvM);
  return hipGetLastError();
}

}  // namespace mx
