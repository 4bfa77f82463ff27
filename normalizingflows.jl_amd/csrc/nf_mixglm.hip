// nf_mixglm.hip -- the mixed-family GLM target (NF_TARGET_MIXGLM; gfx950): the generalised linear-predictor form with a row
// function PER 32-ROW BLOCK,
//     log p(y) = par[1] + sum_b sum_{i in b} wt_i phi_{f_b}(u_i; q_b) + lin . y - pw |y|^2 / 2,   u = A y + off,
//     grad     = A' (wt o phi') + lin - pw y,     pw = 1 / s1^2 (0 for the flat prior s1 = +inf; the host folded its normaliser into par[1]).
// Block b = rows [32 b, 32 b + 32) has a family code f_b and a family parameter q_b:
//     0 log sigmoid | 1 log Phi | 2 -exp | 3 Student (q = nu) | 4 -u^2 / 2   (the row functions of nf_linpred.h, unchanged)
//     5 the check function -u (q - [u < 0]), q = tau in (0, 1)                (PhiCheck, nf_linpred.h)
// so that a likelihood, a non-Gaussian prior on coefficients (rows e_j / scale), a Gaussian penalty (rows of a factor of S) and a
// second outcome sit in ONE matrix product.  Data: A [R x d] row-major, the host's rows SORTED BY FAMILY and every (family, parameter)
// run padded to whole 32-row blocks by rows of weight 0 (R a multiple of 32), and ONE buffer
//     p0 = lin[d] | off[R] | wt[R] | fam[R / 32] | bpar[R / 32] | par[2]      (MixRows below; par = (0, const)).
// Two kernels, the counterparts of nf_linpred.hip's:
//   k_target_mixglm_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_mixglm        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// The family is dispatched ONCE PER BLOCK: in the tiled kernel a wave owns a whole block, so the code is wave-uniform -- it is read
// beside the block's offsets and weights, bounded by select, made a scalar (first lane), and the wave branches to one of seven arms:
// six are each the fully unrolled 16-register loop of ONE row function, the seventh drops the block.  A block executes its own family's instructions only: a normal-prior
// block never pays for erfcx, and nothing is selected among six results.  The flat kernel passes A in 16-row half blocks, so the code
// is uniform over the workgroup there.  A code outside 0 .. 5 (NaN included) takes that seventh arm: phi = phi' = 0, and GEMM 2 is
// skipped -- the block contributes exactly nothing.  Nothing is addressed through the code.
// A row of weight 0 contributes exactly 0 by SELECT (glm_weigh).  Nothing is clamped.  No atomics: two launches give the same bits.
// Shared stages: the row functions and glm_weigh (nf_linpred.h); tgt_stage and tgt_gemm1 (the wave's image of a row block, GEMM 1 from
// it), tgt_elbo_term and tgt_block_partial and the launch helpers (nf_target_stages.h).  The tile load, the wave-ordered combine, the
// tiled epilogue and the flat kernel's y -> sY load stand here in place, as in every file of the family (nf_ordinal.hip's reason).
// This file's device code is compiled without packed fp32 arithmetic (the attribute below, device pass only, this translation unit
// only): the middles are scalar code per accumulator register next to MFMAs.  DESIGN.md section 4 has the launch with and without it.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define MX_BLOCK 256
#define MX_WAVES 4
#define MX_MAXD 256
#define MX_CW 128  // features of A a wave's image holds at a time

// The row data, addressed inside the one buffer p0 = lin[d] | off[R] | wt[R] | fam[R / 32] | bpar[R / 32] | par[2].
template <class T>
struct MixRows {
  const T *lin, *off, *wt, *fam, *bpar, *par;
  __device__ __forceinline__ MixRows(const T *p0, int d, int R)
      : lin(p0), off(p0 + d), wt(p0 + d + R), fam(p0 + d + 2 * (long)R), bpar(p0 + d + 2 * (long)R + (R >> 5)), par(p0 + d + 2 * (long)R + 2 * (R >> 5)) {}
  // The host cannot validate device memory: a block's code is an integer of 0 .. 5 or -1, by select (NaN fails both comparisons).
  static __device__ __forceinline__ int code(T v) { return (v >= (T)0 && v < (T)6) ? (int)v : -1; }
};

// the arm of a dropped block
struct PhiNone {
  template <class T>
  static __device__ __forceinline__ void eval(T, T, T &phi, T &dphi) {
    phi = dphi = (T)0;
  }
};

// f(PHI()) for the row function of a block's code (uniform over the caller's wave / workgroup): one compare-and-branch chain per
// block, every arm compiled with its row function a type
template <class F>
__device__ __forceinline__ void mix_with_family(int code, F &&f) {
  if (code == 0)
    f(PhiLogSigmoid());
  else if (code == 1)
    f(PhiLogNormCdf());
  else if (code == 2)
    f(PhiNegExp());
  else if (code == 3)
    f(PhiStudent());
  else if (code == 4)
    f(PhiHalfSquare());
  else if (code == 5)
    f(PhiCheck());
  else
    f(PhiNone());
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The tile sits in LDS,
// [feature][sample], features >= d and padding samples zero.  Each wave takes the row blocks rb = wave, wave + 4, ... of A (32 rows,
// ONE family: with the rows sorted by family, a family's blocks are consecutive and so dealt round over the four waves) and stages
// its block into an image of its own, 32 rows x up to 128 features (row stride odd: GEMM 1 -- lanes along rows -- and GEMM 2 -- lanes
// along features -- are both free of bank conflicts).  d > 128 (DB = 8 only) takes two chunks: GEMM 1 accumulates over them, GEMM 2
// runs over them in reverse, so the last chunk of GEMM 1 is the first of GEMM 2 and only the other one is staged again:
//   GEMM 1   U[i][j] = off_i + sum_f A[i][f] Y[f][j]     (off is the initial accumulator)
//   phi      in the accumulator registers under the block's family: register r of a lane of half `hi` is row nf_row(r, hi) of sample
//            l & 31; wt by select; wt phi' left in the accumulator, which IS
//   GEMM 2   G[f][j] += sum_i A[i][f] (wt phi')[i][j]    's B operand (the register chaining of nf_mfma.h)
// The block's code and parameter, its 16 offsets and 16 weights per lane are requested before the staging loads, so they are in by
// the time the image is.  The four waves' G and log-p sums are combined through LDS in wave order: the same bits every launch.
template <int DB>
struct MgGeo {
  static constexpr int YT = 32 * DB * 32;  // the tile; reused for the reduction of G over the four waves
  __host__ __device__ static constexpr int stride(int d) { return 32 * (((d < MX_CW ? d : MX_CW) + 31) >> 5) + 1; }
  __host__ __device__ static constexpr int floats(int d) { return YT + MX_WAVES * 32 * stride(d); }
};

// one arm: the 16 rows of a lane under ONE row function; phi' under its weight replaces u in the accumulator
template <class PHI>
__device__ __forceinline__ void mix_arm(f32x16 &U, const float (&wt)[16], float q, float &lp) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float ph, dp;
    PHI::eval(U[r], q, ph, dp);
    glm_weigh(wt[r], ph, dp);
    lp += ph;
    U[r] = dp;
  }
}

template <int DB>
__global__ __launch_bounds__(MX_BLOCK) void k_target_mixglm_tiled(int d, int R, long N, const float *__restrict__ yt, const float *__restrict__ p0,
                                                                  const float *__restrict__ A, float pw, const float *__restrict__ logq,
                                                                  const float *__restrict__ ladj, float *__restrict__ gt, float gscale,
                                                                  float *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  using G = MgGeo<DB>;
  const MixRows<float> rd(p0, d, R);
  const int S = G::stride(d);
  const int nch = DB == 8 ? (d + MX_CW - 1) / MX_CW : 1;  // (d <= 128 below DB = 8)
  extern __shared__ float mx_lds[];
  float *sY = mx_lds;
  float *sA = mx_lds + G::YT;
  __shared__ float sL[MX_WAVES][64];  // [wave][lane] log-p partial sums
  __shared__ float red[MX_BLOCK / 32][32], redl[MX_BLOCK / 32][32];
  __shared__ double sm[MX_WAVES];
  const long tile = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // a scalar: so are rb, the block's code and its parameter
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YT / MX_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * MX_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * MX_BLOCK] = yv[k];
  }
  __syncthreads();

  float *img = sA + wave * 32 * S;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f;
  const int nrb = R >> 5;
  for (int rb = wave; rb < nrb; rb += MX_WAVES) {
    const int i0 = rb * 32;
    const float fv = rd.fam[rb], q = rd.bpar[rb];  // (requested with the offsets and the weights, before the staging loads)
    float wt[16];
    f32x16 U;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + nf_row(r, hi);
      U[r] = rd.off[i];
      wt[r] = rd.wt[i];
    }
    for (int ch = 0; ch < nch; ++ch) {
      const int f0 = ch * MX_CW, pc = d - f0 < MX_CW ? d - f0 : MX_CW;
      tgt_stage(img, S, A, i0, d, f0, pc, lane);
      wave_lds_fence();
      U = tgt_gemm1(U, img, S, sY + f0 * 32, pc, l31, hi);
      if (ch + 1 < nch) wave_lds_fence();  // the next chunk overwrites the image
    }

    // the middle: ONE branch per block to the block's own row function
    const int code = __builtin_amdgcn_readfirstlane(MixRows<float>::code(fv));
    mix_with_family(code, [&](auto phi) { mix_arm<decltype(phi)>(U, wt, q, lp); });

    if (code >= 0) {  // (wave-uniform) a dropped block adds nothing: its rows of A are not multiplied at all
      for (int ch = nch - 1; ch >= 0; --ch) {
        const int f0 = ch * MX_CW, pc = d - f0 < MX_CW ? d - f0 : MX_CW;
        if (ch != nch - 1) {
          wave_lds_fence();
          tgt_stage(img, S, A, i0, d, f0, pc, lane);
          wave_lds_fence();
        }
#pragma unroll
        for (int b = 0; b < DB; ++b) {
          if (b * 32 >= f0 && b * 32 < f0 + pc) {  // (wave-uniform) block b holds features of this chunk
            const float *pa = img + (4 * hi) * S + (b * 32 - f0) + l31;
#pragma unroll
            for (int t = 0; t < 16; ++t) Gacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[((t & 3) + 8 * (t >> 2)) * S], U[t], Gacc[b], 0, 0, 0);
          }
        }
      }
    }
    wave_lds_fence();  // the next staging overwrites the image
  }

  // the four waves' G and log-p sums, combined in wave order
  sL[wave][lane] = lp;
  for (int w = 0; w < MX_WAVES; ++w) {
    __syncthreads();  // (first pass: every wave is done reading the tile)
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < DB; ++b)
        if (b * 32 < d) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float *p = sY + (b * 32 + nf_row(r, hi)) * 32 + l31;
            *p = w == 0 ? Gacc[b][r] : *p + Gacc[b][r];
          }
        }
    }
  }
  __syncthreads();

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s
  const int s = threadIdx.x & 31, qf = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f, ly = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER], lv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = qf + k * (MX_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
      lv[k] = i < d ? rd.lin[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = qf + k * (MX_BLOCK / 32);
      yy += yv[k] * yv[k];
      ly += lv[k] * yv[k];
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] + lv[k] - pw * yv[k]) : 0.f;
    }
  }
  red[qf][s] = yy;
  redl[qf][s] = ly;
  __syncthreads();
  double contrib = 0.0;
  if (qf == 0 && valid) {
    float t = 0.f, tl = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < MX_BLOCK / 32; ++k) t += red[k][s];
#pragma unroll
    for (int k = 0; k < MX_BLOCK / 32; ++k) tl += redl[k][s];
#pragma unroll
    for (int w = 0; w < MX_WAVES; ++w) l += sL[w][s] + sL[w][32 + s];
    const float e = rd.par[1] + l + tl - 0.5f * pw * t;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  A passes through LDS in blocks of
// 16 rows (half a family block: the code is uniform over the workgroup): lane q of a sample takes row q (u, phi, phi'), phi' goes
// through LDS, and lane q then owns the features q, q + 16, ... of the gradient.
#define MXF_LANES 16
#define MXF_SPB (MX_BLOCK / MXF_LANES)
#define MXF_RB 16

template <class T>
__global__ __launch_bounds__(MX_BLOCK) void k_target_mixglm(int d, int R, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                            const T *__restrict__ A, T pw, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                            T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale, T *__restrict__ elbos_out,
                                                            double *__restrict__ partial, double pscale) {
  const MixRows<T> rd(p0, d, R);
  extern __shared__ double mxf_lds[];
  const int S = d + 1, SD = MXF_RB + 1;
  T *sY = (T *)mxf_lds;        // [sample][d + 1]
  T *sA = sY + MXF_SPB * S;    // [row][d + 1]
  T *sD = sA + MXF_RB * S;     // [sample][17] wt phi'
  __shared__ double sm[MX_BLOCK / 64];
  const int q = threadIdx.x & (MXF_LANES - 1), sl = threadIdx.x / MXF_LANES;
  const long j = (long)blockIdx.x * MXF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < MXF_SPB * d; idx += MX_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * MXF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  T g[MX_MAXD / MXF_LANES];
#pragma unroll
  for (int k = 0; k < MX_MAXD / MXF_LANES; ++k) g[k] = (T)0;
  T lp = 0;
  for (int i0 = 0; i0 < R; i0 += MXF_RB) {
    const int code = MixRows<T>::code(rd.fam[i0 >> 5]);           // the block's family (uniform)
    const T par = rd.bpar[i0 >> 5], ov = rd.off[i0 + q], wv = rd.wt[i0 + q];  // (requested with the block of A)
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < MXF_RB * d; idx += MX_BLOCK) {
      const int row = idx / d, f = idx - row * d;
      sA[row * S + f] = A[(long)(i0 + row) * d + f];
    }
    __syncthreads();
    T u = ov;
    for (int f = 0; f < d; ++f) u += sA[q * S + f] * sY[sl * S + f];
    T ph, dp;
    mix_with_family(code, [&](auto phi) { decltype(phi)::eval(u, par, ph, dp); });
    glm_weigh(wv, ph, dp);
    lp += ph;
    sD[sl * SD + q] = dp;
    __syncthreads();
    if (code >= 0) {  // (uniform) a dropped block's rows of A are not multiplied at all
#pragma unroll
      for (int k = 0; k < MX_MAXD / MXF_LANES; ++k) {
        const int f = k * MXF_LANES + q;
        if (f < d) {
          T a = g[k];
#pragma unroll
          for (int r = 0; r < MXF_RB; ++r) a += sA[r * S + f] * sD[sl * SD + r];
          g[k] = a;
        }
      }
    }
  }
  T yy = 0, ly = 0;
#pragma unroll
  for (int k = 0; k < MX_MAXD / MXF_LANES; ++k) {
    const int f = k * MXF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f], lv = rd.lin[f];
      yy += yv * yv;
      ly += lv * yv;
      if (grad_out) grad_out[j * d + f] = gscale * (g[k] + lv - pw * yv);
    }
  }
  lp = group16_sum(lp);
  yy = group16_sum(yy);
  ly = group16_sum(ly);
  double contrib = 0.0;
  if (valid && q == 0) {
    const T e = rd.par[1] + lp + ly - (T)0.5 * pw * yy;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = R, a multiple of 32; s1 = the prior sigma)
// ---------------------------------------------------------------------------------------------------------------------
static double mixglm_pw(const nf_target *t) { return std::isinf(t->s1) ? 0.0 : 1.0 / (t->s1 * t->s1); }

template <int DB>
static int launch_mixglm_tiled(const TgtTiledArgs &a) {
  using G = MgGeo<DB>;
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_mixglm_tiled<DB>>(ctx, G::floats(32 * DB) * sizeof(float)));
  ProfScope ps(ctx, "target_mixglm");
  return tgt_launch_tiled<k_target_mixglm_tiled<DB>>(a, (size_t)G::floats(a.d) * sizeof(float), a.d, (int)a.t->s0, a.N, a.yt, (const float *)a.t->p0,
                                                     (const float *)a.t->p1, (float)mixglm_pw(a.t));
}

int nf_launch_target_mixglm_tiled(const TgtTiledArgs &a) {
  if (a.d > MX_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_db(a.d, [&](auto db) { return launch_mixglm_tiled<db()>(a); });
}

// elements of LDS the flat kernel takes at d
static size_t mixglm_flat_lds(int d) { return (size_t)((MXF_SPB + MXF_RB) * (d + 1) + MXF_SPB * (MXF_RB + 1)); }

template <class T>
static int launch_mixglm_flat(const TgtFlatArgs &a) {
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_mixglm<T>>(ctx, mixglm_flat_lds(MX_MAXD) * sizeof(T)));  // the most any served target takes
  ProfScope ps(ctx, "target_mixglm");
  return tgt_launch_flat<k_target_mixglm<T>, T>(a, mixglm_flat_lds(a.d) * sizeof(T), a.d, (int)a.t->s0, a.N, (const T *)a.y, (const T *)a.t->p0,
                                                (const T *)a.t->p1, (T)mixglm_pw(a.t));
}

int nf_launch_target_mixglm(const TgtFlatArgs &a) {
  if (a.d > MX_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_mixglm_flat<decltype(e)>(a); });
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
