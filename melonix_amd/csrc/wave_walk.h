// wave_walk.h — what the kernels share that walk a run of consecutive frames on Plan<4096,16> beside stft_kernel:
// pv_analysis, pv_synthesis (pv_*.hip), f0_yin (f0_kernels.hip) and chroma_frames (chroma_kernels.hip).  Pieces, not a
// schedule: what a kernel does between its barriers stays its own — but for the three passes of a transform behind a register
// image (walk_passes), which f0_yin and chroma_frames take barrier for barrier, and the start of their walk (fill_ltw2,
// block_run).  Their launch side is kernels.h's walk_grid.  Private to those units.
#pragma once
#include "stft_core.h"
#include "stft_kernel_impl.h"  // wave_reduce_u32

namespace mx {

using f32x4 = float __attribute__((ext_vector_type(4)));
using u32x4 = uint32_t __attribute__((ext_vector_type(4)));
using i16x4 = short __attribute__((ext_vector_type(4)));

// XCD-aware block -> run map (stft_kernel, stft_kernel_impl.h, carries its own copy): the dispatcher places block b on
// XCD b % 8 and each XCD has a private L2, so every XCD takes one contiguous eighth of the runs — the samples that
// neighbouring runs share (95 % at a hop of 256) are then an L2 hit instead of a second fetch over the fabric.
// Bijective for any grid size; a different placement only costs speed.
__device__ __forceinline__ unsigned xcd_block(unsigned b, unsigned nb) {
  const unsigned xcd = b & 7u, q = nb >> 3, r = nb & 7u;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// inclusive sum over the 64 lanes of a wavefront through the DPP crossbar (row_shr 1, 2, 4, 8; row_bcast:15, row_bcast:31),
// int or float
template <typename T>
__device__ __forceinline__ T wave_scan_add(T x) {
  static_assert(sizeof(T) == 4, "one DPP move per step");
#define MX_SCAN_STEP(CTRL, ROWS) \
  x += __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROWS, 0xf, false));
  MX_SCAN_STEP(0x111, 0xf)
  MX_SCAN_STEP(0x112, 0xf)
  MX_SCAN_STEP(0x114, 0xf)
  MX_SCAN_STEP(0x118, 0xf)
  MX_SCAN_STEP(0x142, 0xa)
  MX_SCAN_STEP(0x143, 0xc)
#undef MX_SCAN_STEP
  return x;
}

// Of the seven pass-3 twiddles gamma^r of a column three stay in registers for the whole walk (r = 1, 2, 4) ...
template <class P>
__device__ __forceinline__ void load_w3_bases(const cpx *tw3, int col, cpx (&b)[3]) {
  b[0] = tw3[0 * P::NS3 + col];
  b[1] = tw3[1 * P::NS3 + col];
  b[2] = tw3[3 * P::NS3 + col];
}
// ... and the other four are one packed product each per frame: w[r - 1] = gamma^r, r = 1..7, from b = gamma^{1, 2, 4}
// (power 1 passes through an empty asm, or the products are hoisted out of the walk and held like the table values).
__device__ __forceinline__ void root_powers7(const cpx (&b)[3], cpx *w) {
  cpx g1 = b[0];
  asm volatile("" : "+v"(g1.x), "+v"(g1.y));
  w[0] = g1;
  w[1] = b[1];
  w[3] = b[2];
  w[2] = pk_cmul2(b[1], g1);
  w[4] = pk_cmul2(b[2], g1);
  w[5] = pk_cmul2(b[2], b[1]);
  w[6] = pk_cmul2(b[2], w[2]);
}

// The pass-2 twiddles into the workgroup's LDS copy, once per walk (a barrier before pass 2 reads them is the caller's)
template <class P>
__device__ __forceinline__ void fill_ltw2(int t, const cpx *tw2, cpx *ltw2) {
  for (int i = t; i < P::TW2; i += P::T) ltw2[i] = tw2[i];
}

// The frames [f0, f1) of a launch of `count` that this block walks, `run` to a block through xcd_block; empty where f0 >= f1
__device__ __forceinline__ void block_run(int run, int64_t count, int64_t &f0, int64_t &f1) {
  const unsigned lb = xcd_block(blockIdx.x, gridDim.x);
  f0 = (int64_t)lb * run;
  f1 = f0 + run < count ? f0 + run : count;
}

// The three passes of stft_core.h on the register image Y (thread t's point c = t + T*e in Y[e]): on return v holds
// the transform in pass 3's layout (v[r] = Z[t + NS3 r], v[q_index(r)] = Z[k0q + NS3 r]).  Four barriers, the first before
// the image is written: every wave is done with its previous contents.  Leaves the image busy: the caller synchronises
// before it writes it.  f0_yin runs it three times a frame (two forward transforms and, on the conjugate, the inverse),
// chroma_frames once.
template <class P>
__device__ __forceinline__ void walk_passes(int t, bool wave0, const cpx (&Y)[P::E], cpx (&v)[P::E], cpx *img, const cpx *ltw2,
                                            const cpx (&w3b)[3]) {
  pass1<P>(Y, v);
  __syncthreads();  // every wave is done with the image's previous contents
  store_t1<P>(t, v, img);
  __syncthreads();
  cpx w2[P::R2 - 1];
  load_t1_tw2<P>(t, v, img, ltw2, w2);
  __syncthreads();
  pass2_reg<P>(v, w2);
  store_t2<P>(t, v, img);
  __syncthreads();
  load_t2<P>(t, v, img);
  cpx w3r[P::R3 - 1];
  root_powers7(w3b, w3r);
  if (wave0) pass3_reg<P, true>(t, v, w3r);
  else pass3_reg<P, false>(t, v, w3r);
}

// The real-FFT split behind pass 3 (stft_core.h PostFly, post_cplx) from post_bases' values (kept for the walk; their
// products are a frame's own, as above): only thread 0's wavefront carries the second base and the t == 0 case.
template <class P>
__device__ __forceinline__ void post_split(int t, bool wave0, cpx ulo, cpx uhi, const cpx (&v)[P::E], cpx (&X)[P::E]) {
  asm volatile("" : "+v"(ulo.x), "+v"(ulo.y), "+v"(uhi.x), "+v"(uhi.y));
  cpx u[P::R3];
  if (wave0) {
    PostFly<P, 0>::run(ulo, uhi, u);
    post_cplx<P, true>(t, v, u, X);
  } else {
    PostFly<P, 0>::run(ulo, ulo, u);
    post_cplx<P, false>(t, v, u, X);
  }
}

}  // namespace mx
