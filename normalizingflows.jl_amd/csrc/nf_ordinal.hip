// nf_ordinal.hip -- the ordinal (cumulative-logit) regression target (NF_TARGET_ORDINAL_LOGIT; gfx950):
//     y = [beta (p) ; gamma (C - 1)] in R^d, d = p + C - 1;   c_1 = gamma_1,  c_k = c_{k-1} + exp(gamma_k)  (ordered cutpoints),
//     eta_i = x_i . beta + off_i,   P(k_i) = sigmoid(c_{k_i + 1} - eta_i) - sigmoid(c_{k_i} - eta_i),   c_0 = -inf, c_C = +inf,
//     log p(y) = par[1] + sum_i wt_i log P(k_i) - par[0]/2 |beta|^2 - par[2]/2 sum_k (c_k - par[3])^2 + sum_{k>=2} gamma_k.
// The difference of the two sigmoids is never formed:  sigmoid(a) - sigmoid(b) = sigmoid(a) sigmoid(-b) (1 - exp(-(a - b))),  and for
// adjacent cutpoints a - b = exp(gamma_{k+1}) belongs to the sample, not to the row:
//     sum_i wt_i log P(k_i) = sum_i wt_i ([k_i < C-1] log sigmoid(c_{k_i + 1} - eta_i) + [k_i > 0] log sigmoid(eta_i - c_{k_i}))
//                             + sum_{k=1}^{C-2} n_k log1mexp(exp(gamma_{k+1})),      n_k = sum_i wt_i [k_i = k]  (host, float64)
// so a row is at most two PhiLogSigmoid terms.  Gradients:
//     g_i    = wt_i ([k_i > 0] sigmoid(c_{k_i} - eta_i) - [k_i < C-1] sigmoid(eta_i - c_{k_i + 1}))      d beta = X' g - par[0] beta
//     d c_m  = sum_i wt_i ([k_i = m-1] sigmoid(eta_i - c_m) - [k_i = m] sigmoid(c_m - eta_i)) - par[2] (c_m - par[3])
//     d gamma_1 = sum_m d c_m,   d gamma_k = exp(gamma_k) sum_{m>=k} d c_m + n_{k-1} D / expm1(D) + 1,   D = exp(gamma_k)
// Data: X [R x p] row-major with the rows GROUPED BY LABEL, every label padded to whole 32-row blocks by rows of weight 0 (R a
// multiple of 32), so that the label belongs to a row block:  p0 = off[R] | wt[R] | lab[R / 32] | par[4] | nk[C]  (OrRows below).
// Two kernels, the counterparts of nf_bnn.hip's:
//   k_target_ordinal_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_ordinal        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// A row of weight 0 contributes exactly 0 to the value and to every gradient by SELECT, at every place its values enter a sum.
// Nothing is clamped.
// Shared stages (nf_target_stages.h): tgt_stage and tgt_gemm1 (the wave's image of a row block, GEMM 1 from it), tgt_elbo_term and
// tgt_block_partial (the ELBO tail of both kernels), and the launch helpers.  The tile load, the wave-ordered combine and the flat
// kernel's y -> sY load stand here in place, as in every file of the family: as calls they change the kernels' instructions; the
// tiled epilogue between them was left where it is ("The target kernels' shared stages").
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define OR_BLOCK 256
#define OR_WAVES 4
#define OR_MAXD 256
#define OR_MAXC 16
#define OR_NC (OR_MAXC - 1)  // the most cutpoints
#define OR_CW 128            // features of X a wave's image holds at a time

// The row data, addressed inside the one buffer p0 = off[R] | wt[R] | lab[R / 32] | par[4] | nk[C]: par[0] / par[2] the prior
// precisions of beta and of the cutpoints, par[1] the additive constant the host folded, par[3] the cutpoint prior's location.
template <class T>
struct OrRows {
  const T *off, *wt, *lab, *par, *nk;
  __device__ __forceinline__ OrRows(const T *p0, int R) : off(p0), wt(p0 + R), lab(p0 + 2 * (long)R), par(p0 + 2 * (long)R + (R >> 5)), nk(p0 + 2 * (long)R + (R >> 5) + 4) {}
  // The host cannot validate device memory: a block's label is bounded to [0, C - 1] by select before it addresses anything (NaN -> 0).
  static __device__ __forceinline__ int label(T v, int C) { return v >= (T)0 ? (v <= (T)(C - 1) ? (int)v : C - 1) : 0; }
};

__device__ __forceinline__ float or_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ double or_expm1(double x) { return expm1(x); }
// log(1 - exp(-D)) and its derivative with respect to log D, D / expm1(D), for D = exp(gamma) >= 0: the expm1 form up to ln 2, the
// log1p form beyond.  The derivative tends to 1 as D -> 0 and is 0 once expm1 overflows.  The library's own transcendentals.
template <class T>
__device__ __forceinline__ void or_log1mexp(T D, T &val, T &dgam) {
  val = D <= (T)0.69314718055994530942 ? lp_log(-or_expm1(-D)) : lp_log1p(-lp_exp(-D));
  dgam = D / or_expm1(D);
}

// The epilogue of ONE sample, run by one thread: the cutpoint prior, the chain from d c to d gamma, the table term and the
// Jacobian.  dc(m), c(m), e(m), gam(m), m = 1 .. nc: the likelihood's d c_m, c_m, exp(gamma_m) and gamma_m; put(m, v) takes
// d gamma_m.  Returns what the four add to log p.  Descending m: the suffix sums of d c are running sums.
template <class T, class DC, class CM, class EM, class GM, class PUT>
__device__ __forceinline__ T or_chain(int nc, T par2, T par3, const T *__restrict__ nk, DC &&dc, CM &&c, EM &&e, GM &&gam, PUT &&put) {
  T suffix = 0, ev = 0;
  for (int m = nc; m >= 1; --m) {
    const T dev = c(m) - par3;
    suffix += dc(m) - par2 * dev;
    ev -= (T)0.5 * par2 * dev * dev;
    if (m == 1)
      put(m, suffix);
    else {
      const T D = e(m), n = nk[m - 1];
      T lv, ld;
      or_log1mexp(D, lv, ld);
      ev += (n == (T)0 ? (T)0 : n * lv) + gam(m);  // a category without weight takes no part, by select
      put(m, D * suffix + (n == (T)0 ? (T)0 : n * ld) + (T)1);
    }
  }
  return ev;
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The tile sits in LDS,
// [feature][sample], features >= d and padding samples zero, with eight zero feature rows behind the 32 DB.  The tile's cutpoints
// and exp(gamma) are formed once, [C - 1][32].  Each wave takes the row blocks rb = wave, wave + 4, ... of X (32 rows, ONE label) and
// stages its block into an image of its own, 32 rows x up to 128 features (row stride odd: GEMM 1 -- lanes along rows -- and GEMM 2
// -- lanes along features -- are both free of bank conflicts).  p > 128 (DB = 8 only) takes two chunks: GEMM 1 accumulates over them,
// GEMM 2 runs over them in reverse, so the last chunk of GEMM 1 is the first of GEMM 2 and only the other one is staged again:
//   GEMM 1   U[i][j] = off_i + sum_f X[i][f] Y[f][j]     (off is the initial accumulator)
//   the middle, in the accumulator registers: register r of a lane of half `hi` is row nf_row(r, hi) of sample l & 31; the two
//            log-sigmoid terms under the block's label (wave-uniform), wt by select, g left in the accumulator, which IS
//   GEMM 2   G[f][j] += sum_i X[i][f] g[i][j]            's B operand (the register chaining of nf_mfma.h)
// The lane's sums of the two d c contributions go to per-wave LDS slots [cutpoint][lane] owned by that lane (the bin index is
// wave-uniform: no gather, no indexed register array, no atomics).  The four waves' G, d c and log-p sums are combined through LDS
// in wave order: the same bits every launch.
template <int DB>
struct OrGeo {
  static constexpr int YT = 32 * DB * 32;  // the tile; its beta rows are reused for the reduction of G over the four waves
  static constexpr int YTP = YT + 8 * 32;  // with the eight zero feature rows behind it
  static constexpr int PMAX = 32 * DB - 1;
  __host__ __device__ static constexpr int stride(int p) { return 32 * (((p < OR_CW ? p : OR_CW) + 31) >> 5) + 1; }
  __host__ __device__ static constexpr int floats(int p) { return YTP + OR_WAVES * 32 * stride(p); }
};

template <int DB>
__global__ __launch_bounds__(OR_BLOCK, DB <= 2 ? 2 : 1) void k_target_ordinal_tiled(int d, int C, int R, long N, const float *__restrict__ yt,
                                                                                   const float *__restrict__ p0, const float *__restrict__ X,
                                                                                   const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                                   float *__restrict__ gt, float gscale, float *__restrict__ elbos_out,
                                                                                   double *__restrict__ partial, double pscale) {
  using G = OrGeo<DB>;
  const OrRows<float> rd(p0, R);
  const int nc = C - 1, p = d - nc;
  const int S = G::stride(p);
  const int nch = DB == 8 ? (p + OR_CW - 1) / OR_CW : 1;  // (p < 128 below DB = 8)
  extern __shared__ float or_lds[];
  float *sY = or_lds;
  float *sA = or_lds + G::YTP;
  __shared__ float sC[OR_NC][32], sE[OR_NC][32];  // c_m and exp(gamma_m) of the tile's samples, m - 1 the row
  __shared__ float sDc[OR_WAVES][OR_NC][64];      // [wave][cutpoint][lane]: the lane's d c_m sums
  __shared__ float sL[OR_WAVES][64];              // [wave][lane] log-p partial sums
  __shared__ float sV[32];                        // what the sample's chain adds to log p
  __shared__ float red[OR_BLOCK / 32][32];
  __shared__ double sm[OR_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YTP / OR_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * OR_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * OR_BLOCK] = yv[k];
  }
#pragma unroll
  for (int m = 0; m < OR_NC; ++m) sDc[wave][m][lane] = 0.f;
  __syncthreads();
  if (threadIdx.x < 32) {  // the ordered transform: a prefix sum of at most 15 exponentials per sample
    float c = sY[p * 32 + threadIdx.x];
    sC[0][threadIdx.x] = c;
    sE[0][threadIdx.x] = 1.f;
    for (int m = 1; m < nc; ++m) {
      const float e = lp_exp(sY[(p + m) * 32 + threadIdx.x]);
      c += e;
      sC[m][threadIdx.x] = c;
      sE[m][threadIdx.x] = e;
    }
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
  for (int rb = wave; rb < nrb; rb += OR_WAVES) {
    const int i0 = rb * 32;
    const int k = OrRows<float>::label(rd.lab[rb], C);  // the block's label (wave-uniform)
    float wt[16];  // (requested before the staging loads: in by the time the image is)
    f32x16 U;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + nf_row(r, hi);
      U[r] = rd.off[i];
      wt[r] = rd.wt[i];
    }
    for (int ch = 0; ch < nch; ++ch) {
      const int f0 = ch * OR_CW, pc = p - f0 < OR_CW ? p - f0 : OR_CW;
      tgt_stage(img, S, X, i0, p, f0, pc, lane);
      wave_lds_fence();
      U = tgt_gemm1(U, img, S, sY + f0 * 32, pc, l31, hi);
      if (ch + 1 < nch) wave_lds_fence();  // the next chunk overwrites the image
    }

    // the middle: at most two log-sigmoid terms per row under the block's label; g stays in U
    const bool hasU = k < nc, hasL = k > 0;
    const float cu = sC[hasU ? k : 0][l31], cl = sC[hasL ? k - 1 : 0][l31];
    float su = 0.f, sl = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float eta = U[r];
      float ph = 0.f, du = 0.f, dl = 0.f, t;
      if (hasU) {
        PhiLogSigmoid::eval(cu - eta, 0.f, t, du);  // log sigmoid(c_{k+1} - eta) ; sigmoid(eta - c_{k+1})
        ph = t;
      }
      if (hasL) {
        PhiLogSigmoid::eval(eta - cl, 0.f, t, dl);  // log sigmoid(eta - c_k) ; sigmoid(c_k - eta)
        ph += t;
      }
      const bool live = wt[r] != 0.f;
      lp += live ? wt[r] * ph : 0.f;
      su += live ? wt[r] * du : 0.f;
      sl += live ? wt[r] * dl : 0.f;
      U[r] = live ? wt[r] * (dl - du) : 0.f;
    }
    if (hasU) sDc[wave][k][lane] += su;       // d c_{k+1}
    if (hasL) sDc[wave][k - 1][lane] -= sl;   // d c_k

    for (int ch = nch - 1; ch >= 0; --ch) {
      const int f0 = ch * OR_CW, pc = p - f0 < OR_CW ? p - f0 : OR_CW;
      if (ch != nch - 1) {
        wave_lds_fence();
        tgt_stage(img, S, X, i0, p, f0, pc, lane);
        wave_lds_fence();
      }
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        if (b * 32 >= f0 && b * 32 < f0 + pc) {  // (wave-uniform) block b holds coefficients of this chunk
          const float *pa = img + (4 * hi) * S + (b * 32 - f0) + l31;
#pragma unroll
          for (int t = 0; t < 16; ++t) Gacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[((t & 3) + 8 * (t >> 2)) * S], U[t], Gacc[b], 0, 0, 0);
        }
      }
    }
    wave_lds_fence();  // the next staging overwrites the image
  }

  // the four waves' gradients, combined in wave order into the feature rows < p of the tile (the gamma rows keep gamma)
  sL[wave][lane] = lp;
  for (int w = 0; w < OR_WAVES; ++w) {
    __syncthreads();  // (first pass: every wave is done reading the tile)
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < DB; ++b)
        if (b * 32 < p) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int f = b * 32 + nf_row(r, hi);
            float *q = sY + f * 32 + l31;
            if (f < p) *q = w == 0 ? Gacc[b][r] : *q + Gacc[b][r];
          }
        }
    }
  }
  __syncthreads();

  // one thread per sample: d c over the waves and the lane halves in a fixed order, then the chain; d gamma replaces gamma in the tile
  const float pwb = rd.par[0], pwc = rd.par[2], loc = rd.par[3];
  if (threadIdx.x < 32) {
    const int s = threadIdx.x;
    sV[s] = or_chain<float>(
        nc, pwc, loc, rd.nk,
        [&](int m) {
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < OR_WAVES; ++w) t += sDc[w][m - 1][s] + sDc[w][m - 1][32 + s];
          return t;
        },
        [&](int m) { return sC[m - 1][s]; }, [&](int m) { return sE[m - 1][s]; }, [&](int m) { return sY[(p + m - 1) * 32 + s]; },
        [&](int m, float v) { sY[(p + m - 1) * 32 + s] = v; });
  }
  __syncthreads();

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s; beta under par[0]
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (OR_BLOCK / 32);
      yv[k] = (valid && i < p) ? yb[i * 32 + s] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (OR_BLOCK / 32);
      yy += yv[k] * yv[k];
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] - pwb * yv[k]) : 0.f;
    }
  }
  red[q][s] = yy;
  __syncthreads();
  double contrib = 0.0;
  if (q == 0 && valid) {
    float tb = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < OR_BLOCK / 32; ++k) tb += red[k][s];
#pragma unroll
    for (int w = 0; w < OR_WAVES; ++w) l += sL[w][s] + sL[w][32 + s];
    float e = rd.par[1] + l + sV[s] - 0.5f * pwb * tb;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  X passes through LDS in blocks of
// 16 rows (half a label block): lane q of a sample takes row q -- eta, the two terms, g --, g goes through LDS as [sample][row], and
// lane q then owns the features q, q + 16, ... of d beta.  The two d c contributions of a block are summed over the sample's 16
// lanes and added by lane 0 to the sample's LDS bins (the bin index is block-uniform).  One lane per sample runs the chain.
#define ORF_LANES 16
#define ORF_SPB (OR_BLOCK / ORF_LANES)
#define ORF_RB 16

template <class T>
__global__ __launch_bounds__(OR_BLOCK) void k_target_ordinal(int d, int C, int R, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                             const T *__restrict__ X, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                             T *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  const OrRows<T> rd(p0, R);
  const T pwb = rd.par[0], pwc = rd.par[2], loc = rd.par[3];
  const int nc = C - 1, p = d - nc;
  extern __shared__ double orf_lds[];
  const int S = d + 1, SP = p + 1, SD = ORF_RB + 1;
  T *sY = (T *)orf_lds;              // [sample][d + 1]
  T *sA = sY + ORF_SPB * S;          // [row][p + 1]
  T *sD = sA + ORF_RB * SP;          // [sample][row] g
  T *sCt = sD + ORF_SPB * SD;        // [sample][16] c_m, m - 1 the column
  T *sEx = sCt + ORF_SPB * OR_MAXC;  // [sample][16] exp(gamma_m)
  T *sDc = sEx + ORF_SPB * OR_MAXC;  // [sample][16] d c_m, then d gamma_m
  __shared__ double sm[OR_BLOCK / 64];
  const int q = threadIdx.x & (ORF_LANES - 1), sl = threadIdx.x / ORF_LANES;
  const long j = (long)blockIdx.x * ORF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < ORF_SPB * d; idx += OR_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * ORF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  sDc[sl * OR_MAXC + q] = (T)0;
  __syncthreads();
  const T *py = sY + sl * S;
  if (q == 0) {  // the ordered transform
    T c = py[p];
    sCt[sl * OR_MAXC] = c;
    sEx[sl * OR_MAXC] = (T)1;
    for (int m = 1; m < nc; ++m) {
      const T e = lp_exp(py[p + m]);
      c += e;
      sCt[sl * OR_MAXC + m] = c;
      sEx[sl * OR_MAXC + m] = e;
    }
  }
  T g[OR_MAXD / ORF_LANES];
#pragma unroll
  for (int k = 0; k < OR_MAXD / ORF_LANES; ++k) g[k] = (T)0;
  T lp = 0;
  for (int i0 = 0; i0 < R; i0 += ORF_RB) {
    const int k = OrRows<T>::label(rd.lab[i0 >> 5], C);  // the block's label (uniform)
    const T of = rd.off[i0 + q], wv = rd.wt[i0 + q];     // (requested with the block of X)
    __syncthreads();  // the cutpoints (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < ORF_RB * p; idx += OR_BLOCK) {
      const int row = idx / p, f = idx - row * p;
      sA[row * SP + f] = X[(long)(i0 + row) * p + f];
    }
    __syncthreads();
    T eta = of;
    for (int f = 0; f < p; ++f) eta += sA[q * SP + f] * py[f];
    const bool hasU = k < nc, hasL = k > 0;
    T ph = 0, du = 0, dl = 0, t;
    if (hasU) {
      PhiLogSigmoid::eval(sCt[sl * OR_MAXC + k] - eta, (T)0, t, du);
      ph = t;
    }
    if (hasL) {
      PhiLogSigmoid::eval(eta - sCt[sl * OR_MAXC + k - 1], (T)0, t, dl);
      ph += t;
    }
    const bool on = wv != (T)0;
    lp += on ? wv * ph : (T)0;
    sD[sl * SD + q] = on ? wv * (dl - du) : (T)0;
    const T su = group16_sum(on ? wv * du : (T)0), sw = group16_sum(on ? wv * dl : (T)0);
    if (q == 0) {
      if (hasU) sDc[sl * OR_MAXC + k] += su;
      if (hasL) sDc[sl * OR_MAXC + k - 1] -= sw;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < OR_MAXD / ORF_LANES; ++kk) {
      const int f = kk * ORF_LANES + q;
      if (f < p) {
        T acc = g[kk];
        const T *pd = sD + sl * SD;
        const T *px = sA + f;
#pragma unroll
        for (int r = 0; r < ORF_RB; ++r) acc += px[r * SP] * pd[r];
        g[kk] = acc;
      }
    }
  }
  lp = group16_sum(lp);
  __syncthreads();
  T ev = 0;
  if (q == 0) {
    const T *cs = sCt + sl * OR_MAXC, *es = sEx + sl * OR_MAXC;
    T *ds = sDc + sl * OR_MAXC;
    ev = or_chain<T>(
        nc, pwc, loc, rd.nk, [&](int m) { return ds[m - 1]; }, [&](int m) { return cs[m - 1]; }, [&](int m) { return es[m - 1]; },
        [&](int m) { return py[p + m - 1]; }, [&](int m, T v) { ds[m - 1] = v; });
  }
  __syncthreads();
  T yy = 0;
#pragma unroll
  for (int kk = 0; kk < OR_MAXD / ORF_LANES; ++kk) {
    const int f = kk * ORF_LANES + q;
    if (f < d && valid) {
      T gv;
      if (f < p) {
        const T yv = y[j * d + f];
        yy += yv * yv;
        gv = g[kk] - pwb * yv;
      } else
        gv = sDc[sl * OR_MAXC + f - p];
      if (grad_out) grad_out[j * d + f] = gscale * gv;
    }
  }
  yy = group16_sum(yy);
  double contrib = 0.0;
  if (valid && q == 0) {
    T e = rd.par[1] + lp + ev - (T)0.5 * pwb * yy;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = R, a multiple of 32; s1 = C; d >= C)
// ---------------------------------------------------------------------------------------------------------------------
template <int DB>
static int launch_ordinal_tiled(const TgtTiledArgs &a) {
  using G = OrGeo<DB>;
  const int C = (int)a.t->s1, p = a.d - (C - 1);
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_ordinal_tiled<DB>>(ctx, G::floats(G::PMAX) * sizeof(float)));
  ProfScope ps(ctx, "target_ordinal");
  return tgt_launch_tiled<k_target_ordinal_tiled<DB>>(a, (size_t)G::floats(p) * sizeof(float), a.d, C, (int)a.t->s0, a.N, a.yt,
                                                      (const float *)a.t->p0, (const float *)a.t->p1);
}

int nf_launch_target_ordinal_tiled(const TgtTiledArgs &a) {
  if (a.d > OR_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_db(a.d, [&](auto db) { return launch_ordinal_tiled<db()>(a); });
}

// elements of LDS the flat kernel takes at (d, p)
static size_t ordinal_flat_lds(int d, int p) {
  return (size_t)(ORF_SPB * (d + 1) + ORF_RB * (p + 1) + ORF_SPB * (ORF_RB + 1) + 3 * ORF_SPB * OR_MAXC);
}

template <class T>
static int launch_ordinal_flat(const TgtFlatArgs &a) {
  const int C = (int)a.t->s1;
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_ordinal<T>>(ctx, ordinal_flat_lds(OR_MAXD, OR_MAXD - 1) * sizeof(T)));  // the most any served target takes
  ProfScope ps(ctx, "target_ordinal");
  return tgt_launch_flat<k_target_ordinal<T>, T>(a, ordinal_flat_lds(a.d, a.d - (C - 1)) * sizeof(T), a.d, C, (int)a.t->s0, a.N, (const T *)a.y,
                                                 (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_ordinal(const TgtFlatArgs &a) {
  if (a.d > OR_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_ordinal_flat<decltype(e)>(a); });
}
