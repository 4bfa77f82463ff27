// nf_correff.hip -- GLM targets with CORRELATED random effects (NF_TARGET_CRE_*; gfx950): lme4's y ~ x + (1 + x | g).  The effects
// b_g in R^k of a level share a learned covariance D R D, D = diag exp(tau), R = L L' a correlation matrix under an LKJ prior:
//     log p(y) = par[1] + sum_i wt_i phi(u_i; par[0] [, lambda]) + lin . y - 1/2 sum_j fom_j y_j^2             u = A y + off
//              + sum_f [ -1/2 sum_g |L^-1 D^-1 b_g|^2 - G (sum_i tau_i + sum_i log L_ii)
//                        + sum_i h_i(tau_i - hm_i) + sum_{i>j} c_ij log(1 - tanh^2 omega_ij) ]    [ + h(lambda - hm) ]
// over y = [beta ; (b^f [G x k, level-major] ; tau^f [k] ; omega^f [k (k - 1) / 2]) f = 1 .. F ; (lambda)], k <= 4, F <= 4, d <= 256.
// L is built from z = tanh omega by stick-breaking (torch's CorrCholeskyTransform), omega in row-major strict-lower order.
// Data: A [rows x d] row-major and ONE buffer (CreRows / CreTerm below)
//     p0 = lin[d] | off[rows] | wt[rows] | par[4] | fom[d] | tab[4][24] | lamh[4].
// Two kernels, the counterparts of nf_linpred.hip's:
//   k_target_correff_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_correff        flat layout, float / double, every sum in double: vector pipe (Float64 flows, nf_target_logp)
// The GLM part is nf_mixglm.hip's pipeline with ragged row blocks: a wave stages a 32-row block, GEMM 1 starts from the offsets,
// the row function runs in the accumulator registers (the dispersion kinds' phi(u exp(-lambda)) through DispLane), its derivative
// IS the B operand of GEMM 2, and the four waves' G are combined through the tile in wave order.
// The prior is this file's own (CreArm).  Nothing of it forms Sigma^-1 or divides by a difference:
//   with e = exp(-2 |omega|):  z = tanh omega = -+expm1(-2 |omega|) / (1 + e),   c = sech omega = 2 exp(-|omega|) / (1 + e),
//   log c = log 2 - |omega| - log1p(e);   row i of L:  s_0 = 1,  L_ij = z_ij s_j,  s_{j+1} = s_j c_ij,  L_ii = s_i
//   (the stick's remainder is a PRODUCT of sech's, never 1 - sum), so  -G sum_i log L_ii + sum c_ij log(1 - z_ij^2) =
//   sum_{i>j} (2 c_ij - G) log c_ij  and its derivative is (G - 2 c_ij) z_ij.
//   phase 1, per level g:  a = exp(-tau) o b_g,  z = L^-1 a (forward substitution),  v = L^-T z;  value -= |z|^2 / 2,
//            grad b_g = -exp(-tau) o v,  W += z z' (lower triangle),  t += v o a.
//   phase 2, per term, from W and t alone:  with Q = sum_g |z_g|^2:  dQ/dL = -2 tril(L^-T W),  dQ/dtau_i = -2 t_i, then the
//            stick-breaking pullback  zbar_ij = M_ij s_j,  cbar_ij = sbar_{j+1} s_j,  sbar_j = M_ij z_ij + sbar_{j+1} c_ij  (sbar_i = M_ii,
//            M = tril(L^-T W)),  grad omega_ij = c_ij (zbar_ij c_ij - cbar_ij z_ij) + (G - 2 c_ij) z_ij.
// No level is visited twice.  k is uniform over the launch: one branch per term to a fully unrolled K-templated arm.
// Tiled epilogue, thread (q, s): every feature's lin - fom y goes into the gradient tile (G, in LDS); then thread (q, s) takes the
// levels q, q + 8, ... of sample s, adds each level's gradient to the tile, and leaves its partial (W, t) in the row images' LDS;
// partial m is summed over q = 0 .. 7 ascending by thread (m & 7, s); every thread reads the totals, and the thread q == i / q ==
// (k + n) & 7 adds tau_i's / omega_n's gradient.  No atomics: one owner per sum, a fixed order, the same bits on every launch.
// Every index read from the buffer is bounded by select before it addresses anything (CreTerm): a garbage table gives wrong
// numbers or skips the term, never an access outside y's d features.  A row of weight 0 is dropped by select; nothing is clamped.
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define CE_BLOCK 256
#define CE_WAVES 4
#define CE_MAXD 256
#define CE_CW 128   // features of A a wave's image holds at a time
#define CE_MAXK 4   // effects per level
#define CE_MAXF 4   // terms
#define CE_TERM 24  // table entries per term: k | G | ib | itau | iom | c[6] | hk[4] | hm[4] | his[4] | 0

__device__ __forceinline__ float ce_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ double ce_expm1(double x) { return expm1(x); }

// The row data, addressed inside the one buffer.
template <class T>
struct CreRows {
  const T *lin, *off, *wt, *par, *fom, *tab, *lamh;
  __device__ __forceinline__ CreRows(const T *p0, int d, int rows)
      : lin(p0), off(p0 + d), wt(p0 + d + rows), par(p0 + d + 2 * (long)rows), fom(par + 4), tab(fom + d), lamh(tab + CE_MAXF * CE_TERM) {}
};

// One term of the table in the arithmetic type R.  k == 0 after the checks: the term is skipped.
template <class R>
struct CreTerm {
  int k, G, ib, it, io;
  R c[6], hk[CE_MAXK], hm[CE_MAXK], hs[CE_MAXK];
  template <class T>
  __device__ __forceinline__ CreTerm(const T *__restrict__ e, int d) {
    const int kk = HierRows<T>::index_in(e[0], CE_MAXK + 1), g = HierRows<T>::index_in(e[1], d + 1);
    const int b = HierRows<T>::index_in(e[2], d + 1), t = HierRows<T>::index_in(e[3], d + 1), o = HierRows<T>::index_in(e[4], d + 1);
    const bool ok = kk >= 1 && g >= 0 && b >= 0 && t >= 0 && o >= 0 && b + g * kk <= d && t + kk <= d && o + (kk * (kk - 1)) / 2 <= d;
    k = ok ? kk : 0, G = ok ? g : 0, ib = ok ? b : 0, it = ok ? t : 0, io = ok ? o : 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = (R)e[5 + i];
#pragma unroll
    for (int i = 0; i < CE_MAXK; ++i) hk[i] = (R)e[11 + i], hm[i] = (R)e[15 + i], hs[i] = (R)e[19 + i];
  }
};

// h(t - hm) and its derivative: the hierarchical kinds' three hyper-priors on a log-scale (HierRows::hyper's forms)
template <class R>
__device__ __forceinline__ void ce_hyper(R kind, R hm, R hs, R t, R &hv, R &hd) {
  const R x = t - hm;
  if (kind == (R)0) {
    const R z = x * hs;
    hv = (R)-0.5 * z * z;
    hd = -z * hs;
  } else if (kind == (R)1) {
    const R e = lp_exp((R)2 * x);
    hv = (R)-0.5 * e;
    hd = -e;
  } else {
    R dp;
    PhiLogSigmoid::eval((R)-2 * x, (R)0, hv, dp);
    hd = (R)-2 * dp;
  }
}

// f(std::integral_constant<int, K>) for the term's k (uniform over the launch); k == 0 runs nothing
template <class F>
__device__ __forceinline__ void ce_with_k(int k, F &&f) {
  if (k == 1)
    f(std::integral_constant<int, 1>());
  else if (k == 2)
    f(std::integral_constant<int, 2>());
  else if (k == 3)
    f(std::integral_constant<int, 3>());
  else if (k == 4)
    f(std::integral_constant<int, 4>());
}

// One term at a compile-time k: every array below is indexed by unrolled loop counters only, so it lives in registers.
template <class R, int K>
struct CreArm {
  static constexpr int NW = K * (K + 1) / 2, NP = NW + K;  // partial sums of a term: tril(W) row-major, then t
  R tau[K], einv[K], il[K], L[K][K], z[K][K], c[K][K], lc[K][K], s[K][K];

  // exp(-tau), L and what the pullback needs of the stick, from the sample's y
  template <class Y>
  __device__ __forceinline__ void factor(const CreTerm<R> &tm, Y &&y) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      tau[i] = y(tm.it + i);
      einv[i] = lp_exp(-tau[i]);
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
      s[i][0] = (R)1;
#pragma unroll
      for (int j = 0; j < i; ++j) {
        const R w = y(tm.io + (i * (i - 1)) / 2 + j), aw = w < (R)0 ? -w : w;
        const R em = ce_expm1((R)-2 * aw), den = (R)2 + em;  // e - 1, 1 + e
        const R zt = -em / den;
        z[i][j] = w < (R)0 ? -zt : zt;
        c[i][j] = (R)2 * lp_exp(-aw) / den;
        lc[i][j] = (R)0.69314718055994530942 - aw - lp_log1p(em + (R)1);
        L[i][j] = z[i][j] * s[i][j];
        if (j + 1 < K) s[i][j + 1] = s[i][j] * c[i][j];
      }
      L[i][i] = s[i][i];
      il[i] = (R)1 / L[i][i];
    }
  }

  // phase 1: the levels g0, g0 + gs, ... of the sample; gadd(feature, value) receives a level's gradient
  template <class Y, class GA>
  __device__ __forceinline__ void levels(const CreTerm<R> &tm, int g0, int gs, Y &&y, GA &&gadd, R &val, R (&P)[NP]) const {
    for (int g = g0; g < tm.G; g += gs) {
      const int base = tm.ib + g * K;
      R a[K], zz[K], v[K];
#pragma unroll
      for (int i = 0; i < K; ++i) a[i] = einv[i] * y(base + i);
#pragma unroll
      for (int i = 0; i < K; ++i) {
        R acc = a[i];
#pragma unroll
        for (int j = 0; j < i; ++j) acc -= L[i][j] * zz[j];
        zz[i] = acc * il[i];
      }
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {
        R acc = zz[i];
#pragma unroll
        for (int l = i + 1; l < K; ++l) acc -= L[l][i] * v[l];
        v[i] = acc * il[i];
      }
      R qq = (R)0;
#pragma unroll
      for (int i = 0; i < K; ++i) qq += zz[i] * zz[i];
      val -= (R)0.5 * qq;
#pragma unroll
      for (int i = 0; i < K; ++i) gadd(base + i, -einv[i] * v[i]);
#pragma unroll
      for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) P[(i * (i + 1)) / 2 + j] += zz[i] * zz[j];
        P[NW + i] += v[i] * a[i];
      }
    }
  }

  // phase 2: the term's hyper value, and gadd(feature, value, owner) for tau_i (owner i) and omega_n (owner K + n), from the totals
  template <class GA>
  __device__ __forceinline__ R hyper(const CreTerm<R> &tm, const R (&P)[NP], GA &&gadd) const {
    const R Gf = (R)tm.G;
    R val = (R)0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      R hv, hd;
      ce_hyper(tm.hk[i], tm.hm[i], tm.hs[i], tau[i], hv, hd);
      val += hv - Gf * tau[i];
      gadd(tm.it + i, P[NW + i] - Gf + hd, i);
    }
    R M[K][K];  // tril(L^-T W): column j by back substitution, rows K - 1 .. j
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
      for (int i = K - 1; i >= j; --i) {
        R acc = P[(i * (i + 1)) / 2 + j];
#pragma unroll
        for (int l = i + 1; l < K; ++l) acc -= L[l][i] * M[l][j];
        M[i][j] = acc * il[i];
      }
    }
#pragma unroll
    for (int i = 1; i < K; ++i) {
      R sb = M[i][i];
#pragma unroll
      for (int j = i - 1; j >= 0; --j) {
        const int n = (i * (i - 1)) / 2 + j;
        const R zb = M[i][j] * s[i][j], cb = sb * s[i][j];
        sb = M[i][j] * z[i][j] + sb * c[i][j];
        const R w = (R)2 * tm.c[n] - Gf;
        val += w * lc[i][j];
        gadd(tm.io + n, c[i][j] * (zb * c[i][j] - cb * z[i][j]) - w * z[i][j], K + n);
      }
    }
    return val;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
template <int DB>
struct CeGeo {
  static constexpr int YT = 32 * DB * 32;  // the tile; reused for the reduction of G over the four waves and as the gradient tile
  __host__ __device__ static constexpr int stride(int d) { return 32 * (((d < CE_CW ? d : CE_CW) + 31) >> 5) + 1; }
  // the four images; the epilogue keeps the terms' partials there: [14][8][32] + [14][32] floats <= 4 * 32 * 33
  __host__ __device__ static constexpr int floats(int d) { return YT + CE_WAVES * 32 * stride(d); }
};
#define CE_NP (CE_MAXK * (CE_MAXK + 1) / 2 + CE_MAXK)

// rows [i0, i0 + 32) x features [f0, f0 + pc) of A [rows x d] -> the wave's image, zero beyond the matrix and up to the end of
// pc's last 32-feature block (tgt_stage bounds no rows, tgt_stage_rows takes no chunk: a ragged last block at d > 128 needs both)
__device__ __forceinline__ void ce_stage(float *__restrict__ img, int S, const float *__restrict__ A, int i0, int rows, int d, int f0, int pc, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  for (int cb = 0; cb * 32 < pc; ++cb) {
    const int col = cb * 32 + l31;
    float v[16];
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) {
      const int i = i0 + 2 * rp + hi;
      v[rp] = (i < rows && col < pc) ? A[(long)i * d + f0 + col] : 0.f;
    }
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) img[(2 * rp + hi) * S + col] = v[rp];
  }
}

// one term of the tiled epilogue (every thread of the workgroup calls it: it holds two barriers)
template <int K, class Y>
__device__ __forceinline__ void ce_term_tiled(const CreTerm<float> &tm, Y &&y, float *__restrict__ sG, float *__restrict__ sP, float *__restrict__ sT,
                                              int q, int s, float &yy) {
  using Arm = CreArm<float, K>;
  Arm arm;
  arm.factor(tm, y);
  float P[Arm::NP];
#pragma unroll
  for (int m = 0; m < Arm::NP; ++m) P[m] = 0.f;
  arm.levels(tm, q, CE_BLOCK / 32, y, [&](int f, float v) { sG[f * 32 + s] += v; }, yy, P);
#pragma unroll
  for (int m = 0; m < Arm::NP; ++m) sP[(m * 8 + q) * 32 + s] = P[m];
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // partial m = q, q + 8 over the eight threads of the sample, ascending
    const int m = q + 8 * h;
    if (m < Arm::NP) {
      float t = 0.f;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) t += sP[(m * 8 + qq) * 32 + s];
      sT[m * 32 + s] = t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < Arm::NP; ++m) P[m] = sT[m * 32 + s];
  const float hv = arm.hyper(tm, P, [&](int f, float v, int owner) {
    if (q == (owner & 7)) sG[f * 32 + s] += v;
  });
  yy += q == 0 ? hv : 0.f;
}

template <int DB, class PHI, bool DISP>
__global__ __launch_bounds__(CE_BLOCK) void k_target_correff_tiled(int d, int rows, int F, long N, const float *__restrict__ yt,
                                                                   const float *__restrict__ p0, const float *__restrict__ A,
                                                                   const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                   float *__restrict__ gt, float gscale, float *__restrict__ elbos_out,
                                                                   double *__restrict__ partial, double pscale) {
  using G = CeGeo<DB>;
  const CreRows<float> rd(p0, d, rows);
  const float par0 = rd.par[0];
  const int S = G::stride(d);
  const int nch = DB == 8 ? (d + CE_CW - 1) / CE_CW : 1;  // (d <= 128 below DB = 8)
  extern __shared__ float ce_lds[];
  float *sY = ce_lds;
  float *sA = ce_lds + G::YT;
  __shared__ float sL[CE_WAVES][64];               // [wave][lane] log-p partial sums
  __shared__ float sDL[DISP ? CE_WAVES : 1][64];   // dispersion kinds: [wave][lane] partial sums of wt d phi / d lambda
  __shared__ float red[CE_BLOCK / 32][32], redl[CE_BLOCK / 32][32];
  __shared__ double sm[CE_WAVES];
  const long tile = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YT / CE_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * CE_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * CE_BLOCK] = yv[k];
  }
  __syncthreads();
  // dispersion kinds: every row a lane evaluates belongs to sample l31, so lambda and exp(-lambda) are per-lane scalars
  DispLane<float> dlane = {0.f, 0.f, 0.f};
  if constexpr (DISP) dlane = PHI::lane(sY[(d - 1) * 32 + l31]);

  float *img = sA + wave * 32 * S;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f, dl = 0.f;
  const int nrb = (rows + 31) >> 5;
  for (int rb = wave; rb < nrb; rb += CE_WAVES) {
    const int i0 = rb * 32;
    float wt[16];
    f32x16 U;
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // (requested before the staging loads; rows >= rows read off = 0, wt = 0, which masks them)
      const int i = i0 + nf_row(r, hi);
      U[r] = i < rows ? rd.off[i] : 0.f;
      wt[r] = i < rows ? rd.wt[i] : 0.f;
    }
    for (int ch = 0; ch < nch; ++ch) {
      const int f0 = ch * CE_CW, pc = d - f0 < CE_CW ? d - f0 : CE_CW;
      ce_stage(img, S, A, i0, rows, d, f0, pc, lane);
      wave_lds_fence();
      U = tgt_gemm1(U, img, S, sY + f0 * 32, pc, l31, hi);
      if (ch + 1 < nch) wave_lds_fence();  // the next chunk overwrites the image
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ph, dp;
      if constexpr (DISP) {
        float dlr;
        PHI::eval(U[r], 0.f, par0, dlane, ph, dp, dlr);
        disp_weigh(wt[r], ph, dp, dlr);
        dl += dlr;
      } else {
        PHI::eval(U[r], par0, ph, dp);
        glm_weigh(wt[r], ph, dp);
      }
      lp += ph;
      U[r] = dp;
    }
    for (int ch = nch - 1; ch >= 0; --ch) {  // in reverse: GEMM 1's last chunk is still staged
      const int f0 = ch * CE_CW, pc = d - f0 < CE_CW ? d - f0 : CE_CW;
      if (ch != nch - 1) {
        wave_lds_fence();
        ce_stage(img, S, A, i0, rows, d, f0, pc, lane);
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
    wave_lds_fence();  // the next staging overwrites the image
  }

  // the four waves' G and log-p sums, combined in wave order
  sL[wave][lane] = lp;
  if constexpr (DISP) sDL[wave][lane] = dl;
  for (int w = 0; w < CE_WAVES; ++w) {
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

  // epilogue: thread (q, s) owns features q, q + 8, ... of sample s, then the levels q, q + 8, ... of every term
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f, ly = 0.f;  // yy collects the prior's share of log p itself
#pragma unroll
  for (int k = 0; k < 4 * DB; ++k) {
    const int i = q + k * (CE_BLOCK / 32);
    if (i < d) {
      const float yv = valid ? yb[i * 32 + s] : 0.f, lv = rd.lin[i], om = rd.fom[i];
      ly += lv * yv;
      yy -= 0.5f * om * (yv * yv);
      float gb = lv - om * yv;
      if constexpr (DISP) {
        if (i == d - 1) {  // lambda: its hyper-prior and the rows' d phi / d lambda in sL's order
          float pv, pg;
          ce_hyper(rd.lamh[0], rd.lamh[1], rd.lamh[2], yv, pv, pg);
#pragma unroll
          for (int w = 0; w < CE_WAVES; ++w) pg += sDL[w][s] + sDL[w][32 + s];
          yy += pv;
          gb += pg;
        }
      }
      sY[i * 32 + s] += gb;
    }
  }
  __syncthreads();  // the levels' gradients go to features other threads of the sample own
  {
    const auto y = [&](int f) { return valid ? yb[f * 32 + s] : 0.f; };  // the tile's lines, just read by this workgroup
    float *sP = sA, *sT = sA + CE_NP * CE_BLOCK;
    const int nf = F < CE_MAXF ? F : CE_MAXF;
    for (int f = 0; f < nf; ++f) {
      const CreTerm<float> tm(rd.tab + f * CE_TERM, d);
      ce_with_k(__builtin_amdgcn_readfirstlane(tm.k), [&](auto kc) { ce_term_tiled<decltype(kc)::value>(tm, y, sY, sP, sT, q, s, yy); });
    }
  }
  __syncthreads();
  if (gt) {
#pragma unroll
    for (int k = 0; k < 4 * DB; ++k) {
      const int i = q + k * (CE_BLOCK / 32);
      if (i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * sY[i * 32 + s] : 0.f;
    }
  }
  red[q][s] = yy;
  redl[q][s] = ly;
  __syncthreads();
  double contrib = 0.0;
  if (q == 0 && valid) {
    float t = 0.f, tl = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < CE_BLOCK / 32; ++k) t += red[k][s];
#pragma unroll
    for (int k = 0; k < CE_BLOCK / 32; ++k) tl += redl[k][s];
#pragma unroll
    for (int w = 0; w < CE_WAVES; ++w) l += sL[w][s] + sL[w][32 + s];
    const float e = rd.par[1] + l + tl + t;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  A passes through LDS in blocks of
// 16 rows: lane q of a sample takes row q, phi' goes through LDS, and lane q then owns the features q, q + 16, ...  Every sum -- the
// predictor, the gradient, the value -- is kept in double, and the whole prior is evaluated in double (CreArm<double>), for
// either element type: lane q takes the levels q, q + 16, ..., the sixteen partial (W, t) are summed in lane order by shuffles,
// and lane 0 adds the hyper-gradients.  The prior's share of the gradient passes through the row block's LDS, [sample][d + 1].
#define CEF_LANES 16
#define CEF_SPB (CE_BLOCK / CEF_LANES)
#define CEF_RB 16

template <class T, class PHI, bool DISP>
__global__ __launch_bounds__(CE_BLOCK) void k_target_correff(int d, int rows, int F, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                             const T *__restrict__ A, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale, T *__restrict__ elbos_out,
                                                             double *__restrict__ partial, double pscale) {
  const CreRows<T> rd(p0, d, rows);
  const T par0 = rd.par[0];
  extern __shared__ double cef_lds[];
  const int S = d + 1, SD = CEF_RB + 1;
  T *sY = (T *)cef_lds;      // [sample][d + 1]
  T *sA = sY + CEF_SPB * S;  // [row][d + 1]; after the rows: [sample][d + 1], the prior's share of the gradient
  T *sD = sA + CEF_RB * S;   // [sample][17] wt phi'
  __shared__ double sm[CE_BLOCK / 64];
  const int q = threadIdx.x & (CEF_LANES - 1), sl = threadIdx.x / CEF_LANES;
  const long j = (long)blockIdx.x * CEF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < CEF_SPB * d; idx += CE_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * CEF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  double g[CE_MAXD / CEF_LANES];
#pragma unroll
  for (int k = 0; k < CE_MAXD / CEF_LANES; ++k) g[k] = 0.0;
  double lp = 0.0, dl = 0.0;
  DispLane<T> dlane = {(T)0, (T)0, (T)0};
  if constexpr (DISP) {  // lambda of the lane's sample and exp(-lambda), once
    __syncthreads();
    dlane = PHI::lane(sY[sl * S + d - 1]);
  }
  for (int i0 = 0; i0 < rows; i0 += CEF_RB) {
    const bool live = i0 + q < rows;
    const T ov = live ? rd.off[i0 + q] : (T)0, wv = live ? rd.wt[i0 + q] : (T)0;  // (requested with the block of A)
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < CEF_RB * d; idx += CE_BLOCK) {
      const int row = idx / d, f = idx - row * d;
      sA[row * S + f] = i0 + row < rows ? A[(long)(i0 + row) * d + f] : (T)0;
    }
    __syncthreads();
    double u = (double)ov;
    for (int f = 0; f < d; ++f) u += (double)sA[q * S + f] * (double)sY[sl * S + f];
    T ph, dp;
    if constexpr (DISP) {
      T dlr;
      PHI::eval((T)u, (T)0, par0, dlane, ph, dp, dlr);
      disp_weigh(wv, ph, dp, dlr);
      dl += (double)dlr;
    } else {
      PHI::eval((T)u, par0, ph, dp);
      glm_weigh(wv, ph, dp);
    }
    lp += (double)ph;
    sD[sl * SD + q] = dp;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CE_MAXD / CEF_LANES; ++k) {
      const int f = k * CEF_LANES + q;
      if (f < d) {
        double a = g[k];
#pragma unroll
        for (int r = 0; r < CEF_RB; ++r) a += (double)sA[r * S + f] * (double)sD[sl * SD + r];
        g[k] = a;
      }
    }
  }

  // the prior: its share of the gradient through sG (the row block's LDS, every lane is done with it)
  __syncthreads();
  T *sG = sA;
  for (int f = q; f < d; f += CEF_LANES) sG[sl * S + f] = (T)0;
  __syncthreads();
  double pv = 0.0;
  {
    const auto ys = [&](int f) { return (double)sY[sl * S + f]; };  // the sample's LDS row (zero for a padding sample)
    const auto gadd = [&](int f, double v) { sG[sl * S + f] += (T)v; };
    const int nf = F < CE_MAXF ? F : CE_MAXF;
    for (int f = 0; f < nf; ++f) {
      const CreTerm<double> tm(rd.tab + f * CE_TERM, d);
      ce_with_k(tm.k, [&](auto kc) {
        using Arm = CreArm<double, decltype(kc)::value>;
        Arm arm;
        arm.factor(tm, ys);
        double P[Arm::NP];
#pragma unroll
        for (int m = 0; m < Arm::NP; ++m) P[m] = 0.0;
        arm.levels(tm, q, CEF_LANES, ys, gadd, pv, P);
        double tot[Arm::NP];
#pragma unroll
        for (int m = 0; m < Arm::NP; ++m) tot[m] = 0.0;
#pragma unroll 1
        for (int l = 0; l < CEF_LANES; ++l) {  // the sixteen partials in lane order (a rolled loop: unrolled, hipcc issues every
                                               // shuffle of the term before the first sum and spills)
#pragma unroll
          for (int m = 0; m < Arm::NP; ++m) tot[m] += __shfl(P[m], l, CEF_LANES);
        }
#pragma unroll
        for (int m = 0; m < Arm::NP; ++m) P[m] = tot[m];
        const double hv = arm.hyper(tm, P, [&](int ft, double v, int) {
          if (q == 0) gadd(ft, v);
        });
        pv += q == 0 ? hv : 0.0;
      });
    }
  }
  if constexpr (DISP) {  // every lane of the sample gets the rows' d phi / d lambda, summed in lane order
    double t = 0.0;
#pragma unroll
    for (int l = 0; l < CEF_LANES; ++l) t += __shfl(dl, l, CEF_LANES);
    dl = t;
  }
  __syncthreads();
  double ly = 0.0;
#pragma unroll
  for (int k = 0; k < CE_MAXD / CEF_LANES; ++k) {
    const int f = k * CEF_LANES + q;
    if (f < d && valid) {
      const double yv = (double)sY[sl * S + f], lv = (double)rd.lin[f], om = (double)rd.fom[f];
      ly += lv * yv;
      pv -= 0.5 * om * (yv * yv);
      double gg = g[k] + lv - om * yv + (double)sG[sl * S + f];
      if constexpr (DISP) {
        if (f == d - 1) {  // lambda: its hyper-prior and the rows' d phi / d lambda
          double hv, hd;
          ce_hyper((double)rd.lamh[0], (double)rd.lamh[1], (double)rd.lamh[2], yv, hv, hd);
          pv += hv;
          gg += hd + dl;
        }
      }
      if (grad_out) grad_out[j * d + f] = gscale * (T)gg;
    }
  }
  lp = group16_sum(lp);
  pv = group16_sum(pv);
  ly = group16_sum(ly);
  double contrib = 0.0;
  if (valid && q == 0) {
    const T e = (T)((double)rd.par[1] + lp + ly + pv);
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = rows, s1 = F in 1 .. 4)
// ---------------------------------------------------------------------------------------------------------------------
// f(PHI(), std::bool_constant<DISP>()) for the row function of the kind
template <class F>
static int correff_dispatch_kind(int kind, F &&f) {
  switch (kind) {
    case NF_TARGET_CRE_LOGIT: return f(PhiLogSigmoid(), std::false_type());
    case NF_TARGET_CRE_PROBIT: return f(PhiLogNormCdf(), std::false_type());
    case NF_TARGET_CRE_POISSON: return f(PhiNegExp(), std::false_type());
    case NF_TARGET_CRE_STUDENT: return f(PhiStudent(), std::false_type());
    case NF_TARGET_CRE_NORMAL: return f(PhiHalfSquare(), std::false_type());
    case NF_TARGET_CRE_DNORMAL: return f(DispScale<PhiHalfSquare>(), std::true_type());
    case NF_TARGET_CRE_DSTUDENT: return f(DispScale<PhiStudent>(), std::true_type());
    default: return NF_ERR_ARG;
  }
}

template <int DB, class PHI, bool DISP>
static int launch_correff_tiled(const TgtTiledArgs &a) {
  using G = CeGeo<DB>;
  nf_ctx *ctx = a.ctx;
  NF_TRY((nf_lds_once<k_target_correff_tiled<DB, PHI, DISP>>(ctx, G::floats(32 * DB) * sizeof(float))));
  ProfScope ps(ctx, "target_correff");
  return tgt_launch_tiled<k_target_correff_tiled<DB, PHI, DISP>>(a, (size_t)G::floats(a.d) * sizeof(float), a.d, (int)a.t->s0, (int)a.t->s1, a.N, a.yt,
                                                                 (const float *)a.t->p0, (const float *)a.t->p1);
}

int nf_launch_target_correff_tiled(const TgtTiledArgs &a) {
  if (a.d > CE_MAXD) return NF_ERR_UNSUPPORTED;
  return correff_dispatch_kind(a.t->kind, [&](auto phi, auto disp) {
    return tgt_dispatch_db(a.d, [&](auto db) { return launch_correff_tiled<decltype(db)::value, decltype(phi), decltype(disp)::value>(a); });
  });
}

// elements of LDS the flat kernel takes at d
static size_t correff_flat_lds(int d) { return (size_t)((CEF_SPB + CEF_RB) * (d + 1) + CEF_SPB * (CEF_RB + 1)); }

template <class T, class PHI, bool DISP>
static int launch_correff_flat(const TgtFlatArgs &a) {
  nf_ctx *ctx = a.ctx;
  NF_TRY((nf_lds_once<k_target_correff<T, PHI, DISP>>(ctx, correff_flat_lds(CE_MAXD) * sizeof(T))));  // the most any served target takes
  ProfScope ps(ctx, "target_correff");
  return tgt_launch_flat<k_target_correff<T, PHI, DISP>, T>(a, correff_flat_lds(a.d) * sizeof(T), a.d, (int)a.t->s0, (int)a.t->s1, a.N, (const T *)a.y,
                                                           (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_correff(const TgtFlatArgs &a) {
  if (a.d > CE_MAXD) return NF_ERR_UNSUPPORTED;
  return correff_dispatch_kind(a.t->kind, [&](auto phi, auto disp) {
    return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_correff_flat<decltype(e), decltype(phi), decltype(disp)::value>(a); });
  });
}
