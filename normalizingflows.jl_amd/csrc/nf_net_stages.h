// nf_net_stages.h -- the stages the conditioner-network (coupling) kernels share: nf_pack.h, nf_coupling.hip, nf_rqs.hip,
// nf_deep.hip, nf_wide.hip.  One copy of each.
//
// As in nf_target_stages.h a stage is a __device__ __forceinline__ function that declares no LDS of its own (a kernel keeps
// its __shared__ arrays and passes pointers), and a stage that only one kernel has stays in that kernel's file.  Pointer
// parameters carry no __restrict__ (the kernels' own parameters do, and that is what the compiler sees after inlining), except
// net_fold_acc's, which the functions it replaces had.  Two
// kernels of this family that do the same thing do not always add in the same ORDER (sequential ((s0 + s1) + s2) + s3 in the
// RealNVP kernels of nf_pack.h, pairwise (s0 + s1) + (s2 + s3) in the spline and deep ones): the order is a template flag,
// because the bits are part of what a kernel computes ("The conditioner-network kernels' shared stages").
#pragma once
#include "nf_common.h"
#include "nf_mfma.h"

// ---- reverse kernels: a wave's weight-gradient accumulators ----------------------------------------------------------
template <int IB, int OB>
__device__ __forceinline__ void net_zero_acc(f32x16 (&a)[IB][OB], float (&b)[OB]) {
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int o = 0; o < OB; ++o)
#pragma unroll
      for (int r = 0; r < 16; ++r) a[i][o][r] = 0.f;
#pragma unroll
  for (int o = 0; o < OB; ++o) b[o] = 0.f;
}

// Fold one wave's accumulators of a layer into the LDS image (the weight image's layout, row stride S); `first`: store, else add.
// A block's sixteen partial sums are read in one go, then written back.  As one read-modify-write after the other
// (`*p = *p + a`) every LDS round trip was exposed: tools/trace_deep_bwd.py showed the fold at 15.0 k of a phase's 56.6 k
// clocks for one hidden layer of 64 and 52.8 k of 183 k for three -- more than a quarter of the reverse kernel.
// (fold_acc of nf_coupling.hip is that element-wise form, with a derived stride: another instruction sequence, kept there.)
template <int IB, int OB, int S>
__device__ __forceinline__ void net_fold_acc(float *__restrict__ w, float *__restrict__ b, const f32x16 (&a)[IB][OB], const float (&bs)[OB],
                                             bool first, int l31, int hi) {
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int o = 0; o < OB; ++o) {
      float *p = w + (i * 32 + 4 * hi) * S + o * 32 + l31;  // row nf_row(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi
      float old[16];
      if (!first) {
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = p[((r & 3) + 8 * (r >> 2)) * S];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) p[((r & 3) + 8 * (r >> 2)) * S] = first ? a[i][o][r] : old[r] + a[i][o][r];
    }
#pragma unroll
  for (int o = 0; o < OB; ++o) {
    const float v = bs[o] + __shfl_xor(bs[o], 32);
    if (hi == 0) {
      float *p = b + o * 32 + l31;
      *p = first ? v : *p + v;
    }
  }
}

// ---- slab reductions and fused epilogues --------------------------------------------------------------------------------
// The block-0 prologue: the deterministic sum of the forward launch's `nlpart` double partials -> *dst (the step's loss).
// Every thread of a block of WAVES waves calls it (it holds a barrier); sm: WAVES doubles.
template <int WAVES, bool PAIRWISE>
__device__ __forceinline__ void net_finish_partials(const double *lpart, int nlpart, double *sm, float *dst) {
  double c = 0.0;
  for (int i = threadIdx.x; i < nlpart; i += 64 * WAVES) c += lpart[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    if constexpr (PAIRWISE) {
      static_assert(!PAIRWISE || WAVES == 4, "the pairwise order is written for four waves");
      *dst = (float)((sm[0] + sm[1]) + (sm[2] + sm[3]));
    } else {
      double t = 0.0;
      for (int w = 0; w < WAVES; ++w) t += sm[w];
      *dst = (float)t;
    }
  }
}

// the waves' shares of one lane, added in the kernel's own order
template <int WAVES, bool PAIRWISE>
__device__ __forceinline__ float net_part_sum(const float (*part)[64], int lane) {
  if constexpr (PAIRWISE) {
    static_assert(!PAIRWISE || WAVES == 4, "the pairwise order is written for four waves");
    return (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  } else {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += part[w][lane];
    return t;
  }
}

// ---- whole-chain forward kernels (affine_chain_body, rqs_chain_body): a tile's input into the E / O registers ------------
// E[b][r] holds feature 2 (32 b + nf_row(r, hi)) of sample l31 of the tile, O[b][r] the feature after it.
//
// the tiled batch through the tile's descriptor (features >= d read as 0), padding samples zeroed
template <int CB, int MB>
__device__ __forceinline__ void chain_load_tile(f32x16 (&E)[CB], f32x16 (&O)[MB], const TileIO &io, bool valid) {
#pragma unroll
  for (int b = 0; b < CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = tile_load(io, tile_soff(b, r, 0));
      const float o = tile_load(io, tile_soff(b, r, 1));
      E[b][r] = valid ? e : 0.f;
      O[b][r] = valid ? o : 0.f;
    }
}
