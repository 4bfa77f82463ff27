// nf_target_stages.h -- the stages the matrix-pipe target kernels share (nf_linpred.hip, nf_mixture.hip, nf_softmax.hip,
// nf_bnn.hip, nf_ordinal.hip, nf_riskset.hip), one copy of each, and the host helpers of their launchers.
//
// Every one of the six files holds a tiled Float32 kernel (one workgroup of four waves per 32-sample tile, both GEMMs on
// v_mfma_f32_32x32x2_f32) and a flat float / double kernel (k_target's layout: 16 lanes per sample, 16 samples per block).
// A stage here is a __device__ __forceinline__ function that declares no LDS of its own: the kernels keep their __shared__
// arrays and pass pointers, so a kernel's static LDS layout is what its own file says.  A stage that only one kernel has
// stays in that kernel's file.  Pointer parameters keep __restrict__ and the flat tail forms its lane / wave indices from
// threadIdx.x itself: both are what keeps a kernel's instructions what they were with the stage written out in place
// ("The target kernels' shared stages").
#pragma once
#include <type_traits>
#include <utility>

#include "nf_common.h"
#include "nf_mfma.h"

// =====================================================================================================================
// device stages
// =====================================================================================================================
// ---- tiled kernels: the wave's image of a 32-row block of X, and GEMM 1 from it -----------------------------------
// rows [i0, i0 + 32) x features [f0, f0 + pc) of X [.. x p] -> the wave's image (row stride S); zero up to the end of pc's last
// 32-feature block.  A half-wave copies 32 consecutive features of one row (128 bytes); every load is issued before the first store.
__device__ __forceinline__ void tgt_stage(float *__restrict__ img, int S, const float *__restrict__ X, int i0, int p, int f0, int pc, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  for (int cb = 0; cb * 32 < pc; ++cb) {
    const int col = cb * 32 + l31;
    float v[16];
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) v[rp] = col < pc ? X[(long)(i0 + 2 * rp + hi) * p + f0 + col] : 0.f;
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) img[(2 * rp + hi) * S + col] = v[rp];
  }
}

// the row-bounded form: rows [i0, i0 + 32) x features [0, p) of X [rows x p]; zero beyond the matrix too
__device__ __forceinline__ void tgt_stage_rows(float *__restrict__ img, int S, const float *__restrict__ X, int i0, int rows, int p, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  for (int cb = 0; cb * 32 < p; ++cb) {
    const int col = cb * 32 + l31;
    float v[16];
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) {
      const int i = i0 + 2 * rp + hi;
      v[rp] = (i < rows && col < p) ? X[(long)i * p + col] : 0.f;
    }
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) img[(2 * rp + hi) * S + col] = v[rp];
  }
}

// U += X_chunk Y_chunk: A from the image, B from the tile at the chunk's first feature (sYc); pc features, in groups of four
// k-steps = eight features (image columns >= pc are zero)
__device__ __forceinline__ f32x16 tgt_gemm1(f32x16 U, const float *__restrict__ img, int S, const float *__restrict__ sYc, int pc, int l31, int hi) {
  const int ng = (pc + 7) >> 3;
  const float *pa = img + l31 * S + hi;
  const float *pb = sYc + hi * 32 + l31;
  for (int g = 0; g < ng; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) U = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[8 * g + 2 * e], pb[(8 * g + 2 * e) * 32], U, 0, 0, 0);
  }
  return U;
}

// the zero-initialised form at feature offset f of the tile (unit / class k of p features: f = k p)
__device__ __forceinline__ f32x16 tgt_gemm1_at(const float *__restrict__ img, int S, const float *__restrict__ sY, int f, int p, int l31, int hi) {
  f32x16 U;
#pragma unroll
  for (int r = 0; r < 16; ++r) U[r] = 0.f;
  const int ng = (p + 7) >> 3;
  const float *pa = img + l31 * S + hi;
  const float *pb = sY + (f + hi) * 32 + l31;
  for (int g = 0; g < ng; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) U = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[8 * g + 2 * e], pb[(8 * g + 2 * e) * 32], U, 0, 0, 0);
  }
  return U;
}

// ---- every kernel: the ELBO tail ----------------------------------------------------------------------------------------
// sample j's term: e = log p(y_j) -> e - logq[j] + ladj[j] (each where given), stored to elbos_out where given; returns the
// sample's contribution to the block's partial
template <class T>
__device__ __forceinline__ double tgt_elbo_term(T e, long j, const T *__restrict__ logq, const T *__restrict__ ladj, T *__restrict__ elbos_out,
                                                double pscale) {
  if (logq) e -= logq[j];
  if (ladj) e += ladj[j];
  if (elbos_out) elbos_out[j] = e;
  return pscale * (double)e;
}

// the block's partial (256 threads): the 64-lane shuffle sum, the four waves' sums through sm[4] in a fixed order.  Every
// thread of the block calls this (it holds a barrier); partial is uniform over the launch.
__device__ __forceinline__ void tgt_block_partial(double contrib, double *__restrict__ sm, double *__restrict__ partial) {
  if (partial) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = contrib;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  }
}

// =====================================================================================================================
// host launch helpers
// =====================================================================================================================
// What nf_launch_target_tiled / nf_launch_target hand to a target's launcher (after nf_target_check).
struct TgtTiledArgs {
  nf_ctx *ctx;
  const nf_target *t;
  int d;
  long N;
  const float *yt, *logq, *ladj;
  float *gt;
  double gscale;
  float *elbos_out;
  double *partial;
  double pscale;
};
struct TgtFlatArgs {
  nf_ctx *ctx;
  int dtype;
  const nf_target *t;
  int d;
  long N;
  const void *y, *logq, *ladj;
  void *logp_out, *grad_out;
  double gscale;
  void *elbos_out;
  double *partial;
  double pscale;
};

// f(std::integral_constant<int, DB>) for the tile's block count DB in {1, 2, 4, 8} that holds d (d <= 256: the caller has
// refused the rest); MAXDB cuts the ladder (and what gets instantiated) for a kernel that stops earlier
template <int MAXDB = 8, class F>
int tgt_dispatch_db(int d, F &&f) {
  if (d <= 32 || MAXDB == 1) return f(std::integral_constant<int, 1>());
  if constexpr (MAXDB >= 2) {
    if (d <= 64 || MAXDB == 2) return f(std::integral_constant<int, 2>());
  }
  if constexpr (MAXDB >= 4) {
    if (d <= 128 || MAXDB == 4) return f(std::integral_constant<int, 4>());
  }
  if constexpr (MAXDB >= 8) return f(std::integral_constant<int, 8>());
  return NF_ERR_UNSUPPORTED;
}

// f(T()) for the element type of NF_DTYPE_*
template <class F>
int tgt_dispatch_dtype(int dtype, F &&f) {
  return dtype == NF_DTYPE_F32 ? f(float()) : f(double());
}

// nf_lds_once<KERN> (nf_common.h) sets the LDS attribute once per device; a launcher opens its ProfScope between that and the
// launch, so that the scope covers the launch alone.
// 256-thread blocks with `lds` bytes of dynamic LDS on the context's stream, one per 32-sample tile / per 16 samples.  `head`:
// the kernel's own leading parameters, up to the target's data; the parameters every kernel ends with are filled in here.
template <auto KERN, class... H>
int tgt_launch_tiled(const TgtTiledArgs &a, size_t lds, H... head) {
  hipLaunchKernelGGL(KERN, dim3((unsigned)((a.N + 31) / 32)), dim3(256), lds, a.ctx->stream, head..., a.logq, a.ladj, a.gt, (float)a.gscale,
                     a.elbos_out, a.partial, a.pscale);
  return (int)hipGetLastError();
}
template <auto KERN, class T, class... H>
int tgt_launch_flat(const TgtFlatArgs &a, size_t lds, H... head) {
  hipLaunchKernelGGL(KERN, dim3((unsigned)((a.N + 15) / 16)), dim3(256), lds, a.ctx->stream, head..., (const T *)a.logq, (const T *)a.ladj,
                     (T *)a.logp_out, (T *)a.grad_out, (T)a.gscale, (T *)a.elbos_out, a.partial, a.pscale);
  return (int)hipGetLastError();
}

// the launchers of the six files, the same contract as k_target_tiled / k_target: same outputs and partial counts
int nf_launch_target_linpred_tiled(const TgtTiledArgs &a);
int nf_launch_target_linpred(const TgtFlatArgs &a);
int nf_launch_target_mixture_tiled(const TgtTiledArgs &a);
int nf_launch_target_mixture(const TgtFlatArgs &a);
int nf_launch_target_softmax_tiled(const TgtTiledArgs &a);
int nf_launch_target_softmax(const TgtFlatArgs &a);
int nf_launch_target_bnn_tiled(const TgtTiledArgs &a);
int nf_launch_target_bnn(const TgtFlatArgs &a);
int nf_launch_target_ordinal_tiled(const TgtTiledArgs &a);
int nf_launch_target_ordinal(const TgtFlatArgs &a);
int nf_launch_target_riskset_tiled(const TgtTiledArgs &a);
int nf_launch_target_riskset(const TgtFlatArgs &a);
