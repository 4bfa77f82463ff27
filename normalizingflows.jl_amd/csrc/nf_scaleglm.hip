// nf_scaleglm.hip -- the scaled-block GLM target (NF_TARGET_SCALEGLM; gfx950): the mixed-family form (nf_mixglm.hip) with a LEARNED
// log-scale coordinate per 32-row block,
//     y = [beta (p) ; tau (S)],   d = p + S <= 256,   1 <= S <= 16,   u = A y + off (A's tau columns are zero),
//     log p(y) = par[1] + sum_b sum_{i in b} wt_i phi_{f_b}(z_i; q_b) + lin . y - sum_j fom_j y_j^2 / 2 + sum_s h_s(tau_s - hm_s),
//     z_i      = exp(-tau_{s_b}) u_i,
//     d / d u_i   = wt_i phi'(z_i) exp(-tau_{s_b}),
//     d / d tau_s = -sum_{b: s_b = s} sum_{i in b} wt_i phi'(z_i) z_i + lin_{p+s} - fom_{p+s} tau_s + h_s'.
// Block b = rows [32 b, 32 b + 32) has kind 35's family code f_b and parameter q_b (0 log sigmoid | 1 log Phi | 2 -exp | 3 Student |
// 4 -u^2 / 2 | 5 check) and a SCALE INDEX s_b in {-1, 0 .. S-1}; -1 is "no scale", kind 35's block exactly.  A P-spline / GAM smooth with
// a learned smoothing parameter, a random-walk or ICAR prior with a learned innovation scale, a Bayesian lasso with a learned global
// scale and a learned residual scale per outcome or per stratum are all this shape.  h_s is one of the hierarchical kinds' three
// hyper-priors over a log-scale (hk_s = 0 log-normal, 1 half-normal, 2 half-Cauchy; HierRows::hyper's arithmetic).  The host folded
// everything linear in y (the -n_s tau_s of the scaled families' normalisers, the half families' Jacobians) into lin and every
// constant into par[1].  Data: A [R x d] row-major, R a multiple of 32, and ONE buffer
//     p0 = lin[d] | off[R] | wt[R] | fam[R / 32] | bpar[R / 32] | sidx[R / 32] | fom[d] | hm[S] | his[S] | hk[S] | par[2]   (SgRows below).
// Two kernels, the counterparts of nf_mixglm.hip's:
//   k_target_scaleglm_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_scaleglm        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// What the scale adds to kind 35's tiled kernel.  exp(-tau_s) is computed ONCE PER TILE into sE[s][sample] (the library's
// exponential: S values per sample, and the hardware one's error grows with |tau|).  A wave owns a whole block, so s_b is
// wave-uniform like the family code: it is read beside it, bounded by select, made a scalar; a lane reads its sample's
// em = sE[s_b][sample] (one LDS read per lane per block) and the block's arm forms z = u em BEFORE anything is squared or
// exponentiated, leaves phi' em in the accumulator for GEMM 2 and sums st = sum_r wt phi' z over the lane's 16 rows.  st goes to
// the bin sDt[wave][s_b][lane]: the slot is the lane's own and the bin index is a scalar -- nf_ordinal.hip's sDc mechanism: no
// gather, no indexed register array, no atomics.  The epilogue thread that owns coordinate p + s of a sample adds its eight bins
// in a fixed order (wave ascending; low half, then high half), so two launches give the same bits.
// A code outside 0 .. 5 drops its block from G, log p and every bin; an index outside 0 .. S-1 (NaN included) is "no scale".  A row
// of weight 0 contributes exactly 0 to all three by SELECT.  Nothing is clamped, nothing is addressed through a value read from p0
// that has not been bounded.
// mix_with_family, PhiNone and the code's bound are copies of nf_mixglm.hip's (a file-local copy: moving them to a header is not
// needed by anything else).  Shared stages: the row functions and glm_weigh (nf_linpred.h); tgt_stage, tgt_gemm1, tgt_elbo_term,
// tgt_block_partial and the launch helpers (nf_target_stages.h).
// This file's device code is compiled without packed fp32 arithmetic, as nf_mixglm.hip's is and for its reason: the middles are
// scalar code per accumulator register next to MFMAs.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define SG_BLOCK 256
#define SG_WAVES 4
#define SG_MAXD 256
#define SG_MAXS 16
#define SG_CW 128  // features of A a wave's image holds at a time

// The row data, addressed inside the one buffer p0 (above).  y's last S coordinates are the log-scales: p = d - S.
template <class T>
struct SgRows {
  const T *lin, *off, *wt, *fam, *bpar, *sidx, *fom, *hm, *his, *hk, *par;
  int p, S;
  __device__ __forceinline__ SgRows(const T *p0, int d, int R, int ns) : p(d - ns), S(ns) {
    const int B = R >> 5;
    lin = p0, off = p0 + d, wt = off + R, fam = wt + R, bpar = fam + B, sidx = bpar + B, fom = sidx + B;
    hm = fom + d, his = hm + ns, hk = his + ns, par = hk + ns;
  }
  // The host cannot validate device memory: a block's code is an integer of 0 .. 5 or -1, its scale index one of 0 .. S-1 or -1,
  // both by select (NaN fails both comparisons).
  static __device__ __forceinline__ int code(T v) { return (v >= (T)0 && v < (T)6) ? (int)v : -1; }
  __device__ __forceinline__ int scale(T v) const { return (v >= (T)0 && v < (T)S) ? (int)v : -1; }
  // h_s(t - hm_s) and its derivative: the hierarchical kinds' three hyper-priors on a log-scale (HierRows::hyper's forms)
  __device__ __forceinline__ void hyper(int s, T t, T &hv, T &hd) const {
    const T x = t - hm[s], kind = hk[s];
    if (kind == (T)0) {
      const T sc = his[s], z = x * sc;
      hv = (T)-0.5 * z * z;
      hd = -z * sc;
    } else if (kind == (T)1) {
      const T e = lp_exp((T)2 * x);
      hv = (T)-0.5 * e;
      hd = -e;
    } else {  // -softplus(2 x) = log sigmoid(-2 x) ; -2 sigmoid(2 x): the exp(-|.|) forms of the logit row function
      T dp;
      PhiLogSigmoid::eval((T)-2 * x, (T)0, hv, dp);
      hd = (T)-2 * dp;
    }
  }
};

// the arm of a dropped block
struct SgPhiNone {
  template <class T>
  static __device__ __forceinline__ void eval(T, T, T &phi, T &dphi) {
    phi = dphi = (T)0;
  }
};

// f(PHI()) for the row function of a block's code (uniform over the caller's wave / workgroup): one compare-and-branch chain per
// block, every arm compiled with its row function a type
template <class F>
__device__ __forceinline__ void sg_with_family(int code, F &&f) {
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
    f(SgPhiNone());
}

// one row at z = u em under its weight: phi, phi' and phi' z, each exactly 0 for weight 0 by select (z may be anything there)
template <class PHI, class T>
__device__ __forceinline__ void sg_row(T u, T em, T w, T q, T &ph, T &dp, T &dz) {
  const T z = u * em;
  PHI::eval(z, q, ph, dp);
  glm_weigh(w, ph, dp);
  dz = w == (T)0 ? (T)0 : dp * z;
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// Kind 35's structure (nf_mixglm.hip): one workgroup of four waves per 32-sample tile, the tile in LDS [feature][sample]; a wave
// takes the row blocks rb = wave, wave + 4, ..., stages its block into an image of its own (32 rows x up to 128 features, odd row
// stride), GEMM 1 from the offsets, the block's arm in the accumulator registers, GEMM 2 with the accumulator as its B operand;
// d > 128 (DB = 8 only) takes two feature chunks, GEMM 2 over them in reverse.  The four waves' G and log-p sums are combined
// through LDS in wave order.  Static LDS on top of kind 35's: sE 2 KB and sDt 16 KB -- with the 98 KB of DB = 8's tile and images
// 119 KB of the 160 KB a workgroup may hold.
template <int DB>
struct SgGeo {
  static constexpr int YT = 32 * DB * 32;  // the tile; reused for the reduction of G over the four waves
  __host__ __device__ static constexpr int stride(int d) { return 32 * (((d < SG_CW ? d : SG_CW) + 31) >> 5) + 1; }
  __host__ __device__ static constexpr int floats(int d) { return YT + SG_WAVES * 32 * stride(d); }
};

// one arm: the 16 rows of a lane under ONE row function at z = u em; phi' em under its weight replaces u in the accumulator
template <class PHI>
__device__ __forceinline__ void sg_arm(f32x16 &U, const float (&wt)[16], float q, float em, float &lp, float &st) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float ph, dp, dz;
    sg_row<PHI>(U[r], em, wt[r], q, ph, dp, dz);
    lp += ph;
    st += dz;
    U[r] = dp * em;
  }
}

template <int DB>
__global__ __launch_bounds__(SG_BLOCK) void k_target_scaleglm_tiled(int d, int R, int ns, long N, const float *__restrict__ yt, const float *__restrict__ p0,
                                                                    const float *__restrict__ A, const float *__restrict__ logq,
                                                                    const float *__restrict__ ladj, float *__restrict__ gt, float gscale,
                                                                    float *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  using G = SgGeo<DB>;
  const SgRows<float> rd(p0, d, R, ns);
  const int S = G::stride(d);
  const int nch = DB == 8 ? (d + SG_CW - 1) / SG_CW : 1;  // (d <= 128 below DB = 8)
  extern __shared__ float sg_lds[];
  float *sY = sg_lds;
  float *sA = sg_lds + G::YT;
  __shared__ float sE[SG_MAXS][32];             // [scale][sample] exp(-tau)
  __shared__ float sDt[SG_WAVES][SG_MAXS][64];  // [wave][scale][lane] the lane's -sum wt phi' z under the scale
  __shared__ float sL[SG_WAVES][64];            // [wave][lane] log-p partial sums
  __shared__ float red[SG_BLOCK / 32][32], redl[SG_BLOCK / 32][32];
  __shared__ double sm[SG_WAVES];
  const long tile = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // a scalar: so are rb, the block's code, scale and parameter
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YT / SG_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * SG_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * SG_BLOCK] = yv[k];
  }
  for (int s = 0; s < rd.S; ++s) sDt[wave][s][lane] = 0.f;  // the lane's own bins
  __syncthreads();
  for (int idx = threadIdx.x; idx < rd.S * 32; idx += SG_BLOCK) (&sE[0][0])[idx] = expf(-sY[rd.p * 32 + idx]);  // once per tile (padding samples: 1)
  __syncthreads();

  float *img = sA + wave * 32 * S;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f;
  const int nrb = R >> 5;
  for (int rb = wave; rb < nrb; rb += SG_WAVES) {
    const int i0 = rb * 32;
    const float fv = rd.fam[rb], q = rd.bpar[rb], sv = rd.sidx[rb];  // (requested with the offsets and the weights, before the staging loads)
    float wt[16];
    f32x16 U;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + nf_row(r, hi);
      U[r] = rd.off[i];
      wt[r] = rd.wt[i];
    }
    for (int ch = 0; ch < nch; ++ch) {
      const int f0 = ch * SG_CW, pc = d - f0 < SG_CW ? d - f0 : SG_CW;
      tgt_stage(img, S, A, i0, d, f0, pc, lane);
      wave_lds_fence();
      U = tgt_gemm1(U, img, S, sY + f0 * 32, pc, l31, hi);
      if (ch + 1 < nch) wave_lds_fence();  // the next chunk overwrites the image
    }

    // the middle: ONE branch per block to the block's own row function, at the block's own scale
    const int code = __builtin_amdgcn_readfirstlane(SgRows<float>::code(fv));
    const int sb = __builtin_amdgcn_readfirstlane(rd.scale(sv));
    const float em = sb >= 0 ? sE[sb][l31] : 1.f;
    float st = 0.f;
    sg_with_family(code, [&](auto phi) { sg_arm<decltype(phi)>(U, wt, q, em, lp, st); });
    if (sb >= 0) sDt[wave][sb][lane] -= st;  // (wave-uniform bin, the lane's own slot; a dropped block's st is 0)

    if (code >= 0) {  // (wave-uniform) a dropped block adds nothing: its rows of A are not multiplied at all
      for (int ch = nch - 1; ch >= 0; --ch) {
        const int f0 = ch * SG_CW, pc = d - f0 < SG_CW ? d - f0 : SG_CW;
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
  for (int w = 0; w < SG_WAVES; ++w) {
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

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s; the owner of coordinate
  // p + sc adds the scale's eight bins (wave ascending; low half, then high half) and its hyper-prior
  const int s = threadIdx.x & 31, qf = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f, ly = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER], lv[PER], ov[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = qf + k * (SG_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
      lv[k] = i < d ? rd.lin[i] : 0.f;
      ov[k] = i < d ? rd.fom[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = qf + k * (SG_BLOCK / 32);
      yy += ov[k] * (yv[k] * yv[k]);
      ly += lv[k] * yv[k];
      float g = sY[(i < d ? i : 0) * 32 + s] + lv[k] - ov[k] * yv[k];
      if (i >= rd.p && i < d) {
        const int sc = i - rd.p;
        float dt = 0.f, hv, hd;
#pragma unroll
        for (int w = 0; w < SG_WAVES; ++w) dt += sDt[w][sc][s], dt += sDt[w][sc][32 + s];
        rd.hyper(sc, yv[k], hv, hd);
        ly += hv;
        g += dt + hd;
      }
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * g : 0.f;
    }
  }
  red[qf][s] = yy;
  redl[qf][s] = ly;
  __syncthreads();
  double contrib = 0.0;
  if (qf == 0 && valid) {
    float t = 0.f, tl = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < SG_BLOCK / 32; ++k) t += red[k][s];
#pragma unroll
    for (int k = 0; k < SG_BLOCK / 32; ++k) tl += redl[k][s];
#pragma unroll
    for (int w = 0; w < SG_WAVES; ++w) l += sL[w][s] + sL[w][32 + s];
    const float e = rd.par[1] + l + tl - 0.5f * t;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// Kind 35's flat layout: 16 lanes per sample, 16 samples per block, one partial per block.  A passes through LDS in blocks of 16
// rows (half a family block: the code and the scale index are uniform over the workgroup): lane q of a sample takes row q (u, z, phi,
// phi'), phi' em goes through LDS, and lane q then owns the features q, q + 16, ... of the gradient.  exp(-tau) is computed once
// per sample and scale into sEm; the 16 rows' wt phi' z are summed by group16_sum and lane 0 of the sample keeps the running sum
// of the scale in sT[sample][s] (its own slots), which the owner of coordinate p + s reads in the tail.  Every sum is a T.
#define SGF_LANES 16
#define SGF_SPB (SG_BLOCK / SGF_LANES)
#define SGF_RB 16

template <class T>
__global__ __launch_bounds__(SG_BLOCK) void k_target_scaleglm(int d, int R, int ns, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                              const T *__restrict__ A, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                              T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale, T *__restrict__ elbos_out,
                                                              double *__restrict__ partial, double pscale) {
  const SgRows<T> rd(p0, d, R, ns);
  extern __shared__ double sgf_lds[];
  const int S = d + 1, SD = SGF_RB + 1;
  T *sY = (T *)sgf_lds;        // [sample][d + 1]
  T *sA = sY + SGF_SPB * S;    // [row][d + 1]
  T *sD = sA + SGF_RB * S;     // [sample][17] wt phi' em
  T *sEm = sD + SGF_SPB * SD;  // [sample][16] exp(-tau_s)
  T *sT = sEm + SGF_SPB * SG_MAXS;  // [sample][16] -sum wt phi' z under scale s
  __shared__ double sm[SG_BLOCK / 64];
  const int q = threadIdx.x & (SGF_LANES - 1), sl = threadIdx.x / SGF_LANES;
  const long j = (long)blockIdx.x * SGF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < SGF_SPB * d; idx += SG_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * SGF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  __syncthreads();
  sEm[sl * SG_MAXS + q] = q < rd.S ? lp_exp(-sY[sl * S + rd.p + q]) : (T)1;  // (SGF_LANES == SG_MAXS: lane q takes scale q)
  sT[sl * SG_MAXS + q] = (T)0;
  T g[SG_MAXD / SGF_LANES];
#pragma unroll
  for (int k = 0; k < SG_MAXD / SGF_LANES; ++k) g[k] = (T)0;
  T lp = 0;
  for (int i0 = 0; i0 < R; i0 += SGF_RB) {
    const int code = SgRows<T>::code(rd.fam[i0 >> 5]), sb = rd.scale(rd.sidx[i0 >> 5]);  // the block's family and scale (uniform)
    const T par = rd.bpar[i0 >> 5], ov = rd.off[i0 + q], wv = rd.wt[i0 + q];                // (requested with the block of A)
    __syncthreads();  // sEm (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < SGF_RB * d; idx += SG_BLOCK) {
      const int row = idx / d, f = idx - row * d;
      sA[row * S + f] = A[(long)(i0 + row) * d + f];
    }
    __syncthreads();
    T u = ov;
    for (int f = 0; f < d; ++f) u += sA[q * S + f] * sY[sl * S + f];
    const T em = sb >= 0 ? sEm[sl * SG_MAXS + sb] : (T)1;
    T ph, dp, dz;
    sg_with_family(code, [&](auto phi) { sg_row<decltype(phi)>(u, em, wv, par, ph, dp, dz); });
    lp += ph;
    sD[sl * SD + q] = dp * em;
    if (sb >= 0) {  // (uniform)
      dz = group16_sum(dz);
      if (q == 0) sT[sl * SG_MAXS + sb] -= dz;
    }
    __syncthreads();
    if (code >= 0) {  // (uniform) a dropped block's rows of A are not multiplied at all
#pragma unroll
      for (int k = 0; k < SG_MAXD / SGF_LANES; ++k) {
        const int f = k * SGF_LANES + q;
        if (f < d) {
          T a = g[k];
#pragma unroll
          for (int r = 0; r < SGF_RB; ++r) a += sA[r * S + f] * sD[sl * SD + r];
          g[k] = a;
        }
      }
    }
  }
  __syncthreads();  // sT is complete
  T yy = 0, ly = 0;
#pragma unroll
  for (int k = 0; k < SG_MAXD / SGF_LANES; ++k) {
    const int f = k * SGF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f], lv = rd.lin[f], fo = rd.fom[f];
      yy += fo * (yv * yv);
      ly += lv * yv;
      T gr = g[k] + lv - fo * yv;
      if (f >= rd.p) {  // tau_s: the rows' sum under the scale and the hyper-prior
        T hv, hd;
        rd.hyper(f - rd.p, yv, hv, hd);
        ly += hv;
        gr += sT[sl * SG_MAXS + (f - rd.p)] + hd;
      }
      if (grad_out) grad_out[j * d + f] = gscale * gr;
    }
  }
  lp = group16_sum(lp);
  yy = group16_sum(yy);
  ly = group16_sum(ly);
  double contrib = 0.0;
  if (valid && q == 0) {
    const T e = rd.par[1] + lp + ly - (T)0.5 * yy;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = R, a multiple of 32; s1 = S in 1 .. 16, S < d)
// ---------------------------------------------------------------------------------------------------------------------
template <int DB>
static int launch_scaleglm_tiled(const TgtTiledArgs &a) {
  using G = SgGeo<DB>;
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_scaleglm_tiled<DB>>(ctx, G::floats(32 * DB) * sizeof(float)));
  ProfScope ps(ctx, "target_scaleglm");
  return tgt_launch_tiled<k_target_scaleglm_tiled<DB>>(a, (size_t)G::floats(a.d) * sizeof(float), a.d, (int)a.t->s0, (int)a.t->s1, a.N, a.yt,
                                                       (const float *)a.t->p0, (const float *)a.t->p1);
}

int nf_launch_target_scaleglm_tiled(const TgtTiledArgs &a) {
  if (a.d > SG_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_db(a.d, [&](auto db) { return launch_scaleglm_tiled<db()>(a); });
}

// elements of LDS the flat kernel takes at d
static size_t scaleglm_flat_lds(int d) { return (size_t)((SGF_SPB + SGF_RB) * (d + 1) + SGF_SPB * (SGF_RB + 1) + 2 * SGF_SPB * SG_MAXS); }

template <class T>
static int launch_scaleglm_flat(const TgtFlatArgs &a) {
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_scaleglm<T>>(ctx, scaleglm_flat_lds(SG_MAXD) * sizeof(T)));  // the most any served target takes
  ProfScope ps(ctx, "target_scaleglm");
  return tgt_launch_flat<k_target_scaleglm<T>, T>(a, scaleglm_flat_lds(a.d) * sizeof(T), a.d, (int)a.t->s0, (int)a.t->s1, a.N, (const T *)a.y,
                                                  (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_scaleglm(const TgtFlatArgs &a) {
  if (a.d > SG_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_scaleglm_flat<decltype(e)>(a); });
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
