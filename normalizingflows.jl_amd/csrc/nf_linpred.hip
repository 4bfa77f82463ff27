// nf_linpred.hip -- the linear-predictor targets (NF_TARGET_DENSEGAUSS, NF_TARGET_LOGREG, NF_TARGET_GLM_*, NF_TARGET_HGLM_*,
// NF_TARGET_DGLM_*; gfx950):
//     centred      log p(y) = c + sum_i phi(u_i) - pw |y|^2 / 2,   u = A (y - mu),   grad = A' phi'(u) - pw y
//     generalised  log p(y) = par[1] + c + sum_i wt_i phi(u_i; par[0]) + lin . y - pw |y|^2 / 2,   u = A y + off,
//                  grad = A' (wt o phi'(u)) + lin - pw y
//     hierarchical the generalised form with the structured prior of nf_linpred.h (HierRows: y = [beta ; tau], groups of
//                  coefficients under learned scales exp(tau_g) with hyper-priors) in place of - pw |y|^2 / 2
//     dispersion   the hierarchical form over y = [beta ; tau ; lambda] with phi_i(u_i, lambda): the log-dispersion lambda = y[d - 1]
//                  is a per-sample scalar inside the row function (DispScale / DispNegBin), with a hyper-prior of its own and, for
//                  the negative binomial, the table term T(lambda) (DispRows)
// with A [rows x d] row-major: MvNormal(mu, Sigma) through W = inv(chol(Sigma)), Bayesian logistic regression through the
// label-folded data matrix, and the regression posteriors with exposures, trial counts, subsampling weights and a family
// parameter through the generalised form.  Two kernel bodies, each templated on the row function phi and on the form
// (nf_linpred.h); the centred instantiations compile every line of the row data away:
//   lp_tiled_body  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//                  (k_target_linpred_tiled: centred, k_target_glm_tiled: generalised, k_target_hier_tiled: hierarchical,
//                  k_target_disp_tiled: dispersion)
//   lp_flat_body   flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
//                  (k_target_linpred, k_target_glm, k_target_hier, k_target_disp)
// Shared stages (nf_target_stages.h): tgt_elbo_term (both bodies; the centred flat kernels keep it in place), tgt_block_partial (the
// flat body; the tiled one keeps it in place) and the launch helpers.
// lp_stage bounds both rows and features of a chunk and is this file's own; what else stands here in place does so for
// nf_ordinal.hip's reason.
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The centred
// tile Y - mu sits in LDS once, [feature][sample], features >= d and padding samples zero.  Each wave takes the row blocks
// rb = wave, wave + 4, ... of A (32 rows each) and stages its block into an LDS image of its own (no workgroup barrier
// inside the row loop):
//   GEMM 1   U[i][j] = sum_f A[i][f] Y[f][j]      A operand: lane <-> row i, B operand: lane <-> sample j, k-step t
//                                                 contracts features 2 t + hi
//   phi      in the accumulator registers: register r of a lane of half `hi` is row nf_row(r, hi) of sample l & 31
//   GEMM 2   G[f][j] += sum_i A[i][f] phi'(U)[i][j]   k-step t contracts the row pair nf_row(t, 0) / nf_row(t, 1): its B
//                                                 operand IS accumulator register t of GEMM 1 (the register chaining of
//                                                 nf_mfma.h), so U never passes through LDS or a shuffle
// Rows >= rows of the last block are masked after phi: a zero row of A gives u = 0, and phi(0) = log 1/2 for LOGREG.
// Generalised form: the tile is staged uncentred; a lane's 16 offsets and 16 weights of a row block are requested with the
// block's staging loads (before the first of them, so they are in by the time the image is); the offsets ARE the initial
// accumulator of GEMM 1, the weights multiply phi and phi' in the accumulator registers (0 by select), and rows >= rows
// read off = 0, wt = 0, which masks them.  lin enters the epilogue beside pw y.
// Hierarchical form: both GEMMs, the offsets, the weights and the wave-ordered combination are the generalised form's; the
// prior lives in the epilogue.  The thread that owns feature i of sample s re-reads y as before; for a coefficient it fetches
// tau of its group from the tile's lines (yb[(p + g) * 32 + s], just read by this workgroup), for a log-scale it walks its
// group's member list over the same lines.  The prior's share of log p takes the path |y|^2 takes (no atomics: one owner per
// sum, in a fixed order).
// Dispersion form: the hierarchical form's, and a lane's 16 accumulator registers all belong to sample lane & 31, so lambda is ONE
// LDS read per lane per tile (sY[(d - 1) * 32 + (lane & 31)], after the tile is staged) and exp(-lambda) / exp(lambda) are formed once;
// NEGBIN's 16 counts are requested with the block's offsets and weights.  The row function returns phi, d phi / d u (into U[r], the B
// operand of GEMM 2) and d phi / d lambda, which a per-lane sum carries beside lp through a second array of sL's shape, combined in
// sL's order by the epilogue thread that owns feature d - 1 of the sample; that thread adds lambda's hyper-prior and the table term,
// which the sample's eight (q, s) threads sum (j = q, q + 8, ... ascending; the partials combined q = 0 .. 7).  No atomics.
// Feature chunks: the image holds at most 128 features of the 32 rows (16.5 KB per wave); a wider target (DB = 8) runs
// GEMM 1 chunk by chunk and stages each chunk a second time for GEMM 2.
#define LP_BLOCK 256
#define LP_WAVES 4

template <int DB>
struct LpGeo {
  static constexpr int CB = DB < 4 ? DB : 4;  // 32-feature blocks per staged chunk
  static constexpr int NCH = DB / CB;         // chunks
  static constexpr int CW = 32 * CB;          // features per chunk
  static constexpr int S = CW + 1;            // row stride of the image: odd, so that GEMM 1 (lanes along rows) and GEMM 2 (lanes
                                              // along features) both read it without bank conflicts
  static constexpr int IMG = 32 * S;          // floats per wave
  static constexpr int YT = 32 * DB * 32;     // the centred tile; reused for the reduction of G over the four waves
  static constexpr int FLOATS = YT + LP_WAVES * IMG + LP_WAVES * 64;
};

// rows [i0, i0 + 32) x features [f0, f0 + CW) of A -> the wave's image, zero beyond the matrix
template <int DB>
__device__ __forceinline__ void lp_stage(float *__restrict__ img, const float *__restrict__ A, int i0, int f0, int rows, int d,
                                         int lane) {
  using G = LpGeo<DB>;
  const int l31 = lane & 31, hi = lane >> 5;
  // whole 32-feature blocks that hold a real feature; a half-wave copies 32 consecutive features of one row (128 bytes)
  for (int cb = 0; cb < G::CB && f0 + cb * 32 < d; ++cb) {
    const int col = cb * 32 + l31, f = f0 + col;
    float v[16];
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) {
      const int i = i0 + 2 * rp + hi;
      v[rp] = (i < rows && f < d) ? A[(long)i * d + f] : 0.f;
    }
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) img[(2 * rp + hi) * G::S + col] = v[rp];
  }
}

// p0: the shift mu[d] (or NULL) of the centred form, the row-data buffer of the generalised one
template <int DB, class PHI, int FORM>
__device__ __forceinline__ void lp_tiled_body(int d, int rows, long N, const float *__restrict__ yt, const float *__restrict__ p0,
                                              const float *__restrict__ A, float c0, float pw, const float *__restrict__ logq,
                                              const float *__restrict__ ladj, float *__restrict__ gt, float gscale,
                                              float *__restrict__ elbos_out, double *__restrict__ partial, double pscale, int ng) {
  using G = LpGeo<DB>;
  constexpr bool GLM = FORM != LP_CENTRED, DISP = FORM == LP_DISP, HIER = FORM == LP_HIER || DISP;
  const GlmRows<float> rd(p0, d, rows);
  const HierRows<float> hr = HierRows<float>::of_form<FORM>(p0, d, rows, ng);
  const float par0 = GLM ? rd.par[0] : 0.f;
  extern __shared__ float lp_sm[];
  float *sY = lp_sm;
  float *sA = lp_sm + G::YT;
  float *sL = sA + LP_WAVES * G::IMG;  // [wave][lane] log-p partial sums
  float *sDL = sL + LP_WAVES * 64;     // dispersion form: [wave][lane] partial sums of wt d phi / d lambda, then [2][q][s] table partials
  __shared__ float red[LP_BLOCK / 32][32];
  __shared__ float redl[GLM ? LP_BLOCK / 32 : 1][32];  // lin . y partial sums (unused, and removed, in the centred form)
  __shared__ double sm[LP_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store: one memory latency, not one per element
    constexpr int PER = G::YT / LP_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * LP_BLOCK, f = idx >> 5, s = idx & 31;
      if (GLM)
        yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
      else
        yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] - (p0 ? p0[f] : 0.f) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * LP_BLOCK] = yv[k];
  }
  __syncthreads();
  // dispersion form: every row a lane evaluates belongs to sample l31, so lambda and its exponentials are per-lane scalars
  // (one LDS read per lane per tile; a padding sample reads 0); the epilogue's sample s is l31 too
  DispLane<float> dlane = {0.f, 0.f, 0.f};
  if constexpr (DISP) dlane = PHI::lane(sY[(d - 1) * 32 + l31]);

  float *img = sA + wave * G::IMG;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f, dl = 0.f;
  const int nrb = (rows + 31) >> 5;
  for (int rb = wave; rb < nrb; rb += LP_WAVES) {
    const int i0 = rb * 32;
    f32x16 U;
    float wt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + nf_row(r, hi);
      U[r] = (GLM && i < rows) ? rd.off[i] : 0.f;
      wt[r] = (GLM && i < rows) ? rd.wt[i] : 0.f;
    }
    float kc[DISP ? 16 : 1];  // the counts of the lane's 16 rows (NEGBIN), requested with the offsets and the weights
    if constexpr (DISP) {
      if constexpr (PHI::COUNTS) {
        const DispRows<float> dr(hr, rd.par, rows, true);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = i0 + nf_row(r, hi);
          kc[r] = i < rows ? dr.cnt[i] : 0.f;
        }
      }
    }
#pragma unroll
    for (int ch = 0; ch < G::NCH; ++ch) {
      const int f0 = ch * G::CW;
      if (f0 < d) {  // (wave-uniform)
        lp_stage<DB>(img, A, i0, f0, rows, d, lane);
        wave_lds_fence();
        const int nf = d - f0 < G::CW ? d - f0 : G::CW;
        const int ng = (nf + 7) >> 3;  // groups of four k-steps = eight features; features >= d are zero on both sides
        const float *pa = img + l31 * G::S + hi;
        const float *pb = sY + (f0 + hi) * 32 + l31;
        for (int g = 0; g < ng; ++g) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            U = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[8 * g + 2 * e], pb[(8 * g + 2 * e) * 32], U, 0, 0, 0);
        }
        if (G::NCH > 1) wave_lds_fence();  // the image is restaged
      }
    }
    const bool ragged = i0 + 32 > rows;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ph, dp;
      if constexpr (DISP) {
        float dlr;
        PHI::eval(U[r], PHI::COUNTS ? kc[r] : 0.f, par0, dlane, ph, dp, dlr);
        disp_weigh(wt[r], ph, dp, dlr);
        dl += dlr;
      } else {
        PHI::eval(U[r], par0, ph, dp);
        if (GLM)
          glm_weigh(wt[r], ph, dp);
        else if (ragged && i0 + nf_row(r, hi) >= rows)
          ph = 0.f, dp = 0.f;
      }
      lp += ph;
      U[r] = dp;
    }
#pragma unroll
    for (int ch = 0; ch < G::NCH; ++ch) {
      const int f0 = ch * G::CW;
      if (f0 < d) {
        if (G::NCH > 1) {
          lp_stage<DB>(img, A, i0, f0, rows, d, lane);
          wave_lds_fence();
        }
#pragma unroll
        for (int cb = 0; cb < G::CB; ++cb) {
          if (f0 + cb * 32 < d) {
            const float *pa = img + (4 * hi) * G::S + cb * 32 + l31;
#pragma unroll
            for (int t = 0; t < 16; ++t)
              Gacc[ch * G::CB + cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[((t & 3) + 8 * (t >> 2)) * G::S], U[t], Gacc[ch * G::CB + cb], 0, 0, 0);
          }
        }
        wave_lds_fence();  // the next staging overwrites the image
      }
    }
  }

  // the four waves' G and log-p sums, combined in wave order
  sL[wave * 64 + lane] = lp;
  if constexpr (DISP) {
    sDL[wave * 64 + lane] = dl;
    if constexpr (PHI::COUNTS) {  // the table term of sample s = l31: thread (q, s) takes j = q, q + 8, ... ascending
      const DispRows<float> dr(hr, rd.par, rows, true);
      float tv, td;
      dr.table(threadIdx.x >> 5, LP_BLOCK / 32, dlane, tv, td);
      sDL[LP_WAVES * 64 + threadIdx.x] = tv;
      sDL[LP_WAVES * 64 + LP_BLOCK + threadIdx.x] = td;
    }
  }
  for (int w = 0; w < LP_WAVES; ++w) {
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
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f, ly = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER], lv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (LP_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
      lv[k] = (GLM && i < d) ? rd.lin[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (LP_BLOCK / 32);
      if (HIER) {  // yy collects the prior's share of log p itself
        float pv = 0.f, pg = 0.f;
        if (valid && i < d) {
          const auto y = [&](int f) { return yb[f * 32 + s]; };  // the tile's lines, just read by this workgroup
          if (i < hr.p)
            hr.coef(i, yv[k], y, pv, pg);
          else if constexpr (!DISP)
            hr.scale(i - hr.p, yv[k], y, pv, pg);
          else if (i < d - 1)
            hr.scale(i - hr.p, yv[k], y, pv, pg);
          else {  // lambda: the rows' d phi / d lambda in sL's order, its hyper-prior (entry G) and the table term, q = 0 .. 7 ascending
            hr.hyper(hr.G, yv[k], pv, pg);
#pragma unroll
            for (int w = 0; w < LP_WAVES; ++w) pg += sDL[w * 64 + s] + sDL[w * 64 + 32 + s];
            if constexpr (DISP) {
              if constexpr (PHI::COUNTS) {
                float tv = 0.f, td = 0.f;
#pragma unroll
                for (int qq = 0; qq < LP_BLOCK / 32; ++qq) {
                  tv += sDL[LP_WAVES * 64 + qq * 32 + s];
                  td += sDL[LP_WAVES * 64 + LP_BLOCK + qq * 32 + s];
                }
                pv += tv;
                pg += td;
              }
            }
          }
        }
        yy += pv;
        ly += lv[k] * yv[k];
        if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] + lv[k] + pg) : 0.f;
        continue;
      }
      yy += yv[k] * yv[k];
      if (GLM) {
        ly += lv[k] * yv[k];
        if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] + lv[k] - pw * yv[k]) : 0.f;
      } else if (gt && i < d)
        gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] - pw * yv[k]) : 0.f;
    }
  }
  red[q][s] = yy;
  if (GLM) redl[q][s] = ly;
  __syncthreads();
  double contrib = 0.0;
  if (q == 0 && valid) {
    float t = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < LP_BLOCK / 32; ++k) t += red[k][s];
#pragma unroll
    for (int w = 0; w < LP_WAVES; ++w) l += sL[w * 64 + s] + sL[w * 64 + 32 + s];
    float e = c0 + l - 0.5f * pw * t;
    if (GLM) {
      float tl = 0.f;
#pragma unroll
      for (int k = 0; k < LP_BLOCK / 32; ++k) tl += redl[k][s];
      e = HIER ? rd.par[1] + l + tl + t : (rd.par[1] + c0) + l + tl - 0.5f * pw * t;
    }
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  if (partial) {  // (tgt_block_partial, in place: as a call it reorders the kernels' last instructions, and k_target_glm_tiled<8> then measured 0.3 % outside the parent's spread)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o, 64);
    if (lane == 0) sm[wave] = contrib;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  }
}

template <int DB, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_linpred_tiled(int d, int rows, long N, const float *__restrict__ yt,
                                                                   const float *__restrict__ mu, const float *__restrict__ A,
                                                                   float c0, float pw, const float *__restrict__ logq,
                                                                   const float *__restrict__ ladj, float *__restrict__ gt,
                                                                   float gscale, float *__restrict__ elbos_out,
                                                                   double *__restrict__ partial, double pscale) {
  lp_tiled_body<DB, PHI, LP_CENTRED>(d, rows, N, yt, mu, A, c0, pw, logq, ladj, gt, gscale, elbos_out, partial, pscale, 0);
}
template <int DB, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_glm_tiled(int d, int rows, long N, const float *__restrict__ yt,
                                                               const float *__restrict__ rowdata, const float *__restrict__ A,
                                                               float c0, float pw, const float *__restrict__ logq,
                                                               const float *__restrict__ ladj, float *__restrict__ gt,
                                                               float gscale, float *__restrict__ elbos_out,
                                                               double *__restrict__ partial, double pscale) {
  lp_tiled_body<DB, PHI, LP_GLM>(d, rows, N, yt, rowdata, A, c0, pw, logq, ladj, gt, gscale, elbos_out, partial, pscale, 0);
}
// hierarchical form: ng = G group log-scales behind the p = d - G coefficients; the prior is read from the buffer
template <int DB, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_hier_tiled(int d, int rows, long N, const float *__restrict__ yt,
                                                                const float *__restrict__ rowdata, const float *__restrict__ A,
                                                                int ng, const float *__restrict__ logq,
                                                                const float *__restrict__ ladj, float *__restrict__ gt,
                                                                float gscale, float *__restrict__ elbos_out,
                                                                double *__restrict__ partial, double pscale) {
  lp_tiled_body<DB, PHI, LP_HIER>(d, rows, N, yt, rowdata, A, 0.f, 0.f, logq, ladj, gt, gscale, elbos_out, partial, pscale, ng);
}

// dispersion form: PHI is DispScale<..> / DispNegBin; ng = G group log-scales between the p = d - G - 1 coefficients and lambda
template <int DB, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_disp_tiled(int d, int rows, long N, const float *__restrict__ yt,
                                                                const float *__restrict__ rowdata, const float *__restrict__ A,
                                                                int ng, const float *__restrict__ logq,
                                                                const float *__restrict__ ladj, float *__restrict__ gt,
                                                                float gscale, float *__restrict__ elbos_out,
                                                                double *__restrict__ partial, double pscale) {
  lp_tiled_body<DB, PHI, LP_DISP>(d, rows, N, yt, rowdata, A, 0.f, 0.f, logq, ladj, gt, gscale, elbos_out, partial, pscale, ng);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  A passes through LDS in
// blocks of 16 rows: lane q of a sample takes row q (u, phi, phi'), phi' goes through LDS, and lane q then owns the
// features q, q + 16, ... of the gradient.
#define LPF_LANES 16
#define LPF_SPB (LP_BLOCK / LPF_LANES)
#define LPF_RB 16
#define LPF_MAXD 256

template <class T, class PHI, int FORM>
__device__ __forceinline__ void lp_flat_body(int d, int rows, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                             const T *__restrict__ A, T c0, T pw, const T *__restrict__ logq,
                                             const T *__restrict__ ladj, T *__restrict__ logp_out, T *__restrict__ grad_out,
                                             T gscale, T *__restrict__ elbos_out, double *__restrict__ partial, double pscale,
                                             int ng) {
  constexpr bool GLM = FORM != LP_CENTRED, DISP = FORM == LP_DISP, HIER = FORM == LP_HIER || DISP;
  const GlmRows<T> rd(p0, d, rows);
  const HierRows<T> hr = HierRows<T>::template of_form<FORM>(p0, d, rows, ng);
  const T par0 = GLM ? rd.par[0] : (T)0;
  extern __shared__ double lpf_sm[];
  T *sY = (T *)lpf_sm;                  // [sample][d + 1] centred
  T *sA = sY + LPF_SPB * (d + 1);       // [row][d + 1]
  T *sD = sA + LPF_RB * (d + 1);        // [sample][17] phi'
  __shared__ double sm[LP_BLOCK / 64];
  const int q = threadIdx.x & (LPF_LANES - 1), sl = threadIdx.x / LPF_LANES;
  const long j = (long)blockIdx.x * LPF_SPB + sl;
  const bool valid = j < N;
  const int S = d + 1;
  for (int idx = threadIdx.x; idx < LPF_SPB * d; idx += LP_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * LPF_SPB + si;
    if (GLM)
      sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
    else
      sY[si * S + f] = jj < N ? y[jj * d + f] - (p0 ? p0[f] : (T)0) : (T)0;
  }
  T g[LPF_MAXD / LPF_LANES];
#pragma unroll
  for (int k = 0; k < LPF_MAXD / LPF_LANES; ++k) g[k] = (T)0;
  T lp = 0, dl = 0;
  DispLane<T> dlane = {(T)0, (T)0, (T)0};
  if constexpr (DISP) {  // lambda of the lane's sample and its exponentials, once
    __syncthreads();
    dlane = PHI::lane(sY[sl * S + d - 1]);
  }
  for (int i0 = 0; i0 < rows; i0 += LPF_RB) {
    const bool live = i0 + q < rows;
    const T ov = (GLM && live) ? rd.off[i0 + q] : (T)0, wv = (GLM && live) ? rd.wt[i0 + q] : (T)0;  // (requested with the block of A)
    T kv = (T)0;
    if constexpr (DISP) {
      if constexpr (PHI::COUNTS) kv = live ? DispRows<T>(hr, rd.par, rows, true).cnt[i0 + q] : (T)0;
    }
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < LPF_RB * d; idx += LP_BLOCK) {
      const int row = idx / d, f = idx - row * d;
      sA[row * S + f] = i0 + row < rows ? A[(long)(i0 + row) * d + f] : (T)0;
    }
    __syncthreads();
    T u = ov;
    for (int f = 0; f < d; ++f) u += sA[q * S + f] * sY[sl * S + f];
    T ph, dp;
    if constexpr (DISP) {
      T dlr;
      PHI::eval(u, kv, par0, dlane, ph, dp, dlr);
      disp_weigh(wv, ph, dp, dlr);
      dl += dlr;
    } else {
      PHI::eval(u, par0, ph, dp);
      if (GLM)
        glm_weigh(wv, ph, dp);
      else if (!live)
        ph = (T)0, dp = (T)0;
    }
    lp += ph;
    sD[sl * (LPF_RB + 1) + q] = dp;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LPF_MAXD / LPF_LANES; ++k) {
      const int f = k * LPF_LANES + q;
      if (f < d) {
        T a = g[k];
#pragma unroll
        for (int r = 0; r < LPF_RB; ++r) a += sA[r * S + f] * sD[sl * (LPF_RB + 1) + r];
        g[k] = a;
      }
    }
  }
  T tv = 0, td = 0;
  if constexpr (DISP) {  // every lane of the sample gets the sums: the owner of feature d - 1 adds them below
    dl = group16_sum(dl);
    if constexpr (PHI::COUNTS) {  // the table term: lane q takes j = q, q + 16, ... ascending; the partials in lane order
      T pv_, pd_;
      DispRows<T>(hr, rd.par, rows, true).table(q, LPF_LANES, dlane, pv_, pd_);
#pragma unroll
      for (int l = 0; l < LPF_LANES; ++l) {
        tv += __shfl(pv_, l, LPF_LANES);
        td += __shfl(pd_, l, LPF_LANES);
      }
    }
  }
  T yy = 0, ly = 0;
#pragma unroll
  for (int k = 0; k < LPF_MAXD / LPF_LANES; ++k) {
    const int f = k * LPF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f];
      if (HIER) {  // yy collects the prior's share of log p itself
        const auto ys = [&](int i) { return sY[sl * S + i]; };  // the sample's LDS row (uncentred in this form)
        T pv, pg;
        if (f < hr.p)
          hr.coef(f, yv, ys, pv, pg);
        else if constexpr (!DISP)
          hr.scale(f - hr.p, yv, ys, pv, pg);
        else if (f < d - 1)
          hr.scale(f - hr.p, yv, ys, pv, pg);
        else {  // lambda: its hyper-prior (entry G), the rows' d phi / d lambda and the table term
          hr.hyper(hr.G, yv, pv, pg);
          pv += tv;
          pg += dl + td;
        }
        const T lv = rd.lin[f];
        yy += pv;
        ly += lv * yv;
        if (grad_out) grad_out[j * d + f] = gscale * (g[k] + lv + pg);
        continue;
      }
      yy += yv * yv;
      if (GLM) {
        const T lv = rd.lin[f];
        ly += lv * yv;
        if (grad_out) grad_out[j * d + f] = gscale * (g[k] + lv - pw * yv);
      } else if (grad_out)
        grad_out[j * d + f] = gscale * (g[k] - pw * yv);
    }
  }
  lp = group16_sum(lp);
  yy = group16_sum(yy);
  if (GLM) ly = group16_sum(ly);
  double contrib = 0.0;
  if (valid && q == 0) {
    T e = c0 + lp - (T)0.5 * pw * yy;
    if (GLM) e = HIER ? rd.par[1] + lp + ly + yy : (rd.par[1] + c0) + lp + ly - (T)0.5 * pw * yy;
    if (logp_out) logp_out[j] = e;
    if constexpr (GLM)
      contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
    else {  // (tgt_elbo_term, in place: as a call the four centred kernels come out in another order, and no benchmark times them)
      if (logq) e -= logq[j];
      if (ladj) e += ladj[j];
      if (elbos_out) elbos_out[j] = e;
      contrib = pscale * (double)e;
    }
  }
  tgt_block_partial(contrib, sm, partial);
}

template <class T, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_linpred(int d, int rows, long N, const T *__restrict__ y,
                                                             const T *__restrict__ mu, const T *__restrict__ A, T c0, T pw,
                                                             const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                             T *__restrict__ elbos_out, double *__restrict__ partial,
                                                             double pscale) {
  lp_flat_body<T, PHI, LP_CENTRED>(d, rows, N, y, mu, A, c0, pw, logq, ladj, logp_out, grad_out, gscale, elbos_out, partial, pscale, 0);
}
template <class T, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_glm(int d, int rows, long N, const T *__restrict__ y,
                                                         const T *__restrict__ rowdata, const T *__restrict__ A, T c0, T pw,
                                                         const T *__restrict__ logq, const T *__restrict__ ladj,
                                                         T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                         T *__restrict__ elbos_out, double *__restrict__ partial,
                                                         double pscale) {
  lp_flat_body<T, PHI, LP_GLM>(d, rows, N, y, rowdata, A, c0, pw, logq, ladj, logp_out, grad_out, gscale, elbos_out, partial, pscale, 0);
}
template <class T, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_hier(int d, int rows, long N, const T *__restrict__ y,
                                                          const T *__restrict__ rowdata, const T *__restrict__ A, int ng,
                                                          const T *__restrict__ logq, const T *__restrict__ ladj,
                                                          T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                          T *__restrict__ elbos_out, double *__restrict__ partial,
                                                          double pscale) {
  lp_flat_body<T, PHI, LP_HIER>(d, rows, N, y, rowdata, A, (T)0, (T)0, logq, ladj, logp_out, grad_out, gscale, elbos_out, partial, pscale, ng);
}
template <class T, class PHI>
__global__ __launch_bounds__(LP_BLOCK) void k_target_disp(int d, int rows, long N, const T *__restrict__ y,
                                                          const T *__restrict__ rowdata, const T *__restrict__ A, int ng,
                                                          const T *__restrict__ logq, const T *__restrict__ ladj,
                                                          T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                          T *__restrict__ elbos_out, double *__restrict__ partial,
                                                          double pscale) {
  lp_flat_body<T, PHI, LP_DISP>(d, rows, N, y, rowdata, A, (T)0, (T)0, logq, ladj, logp_out, grad_out, gscale, elbos_out, partial, pscale, ng);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check)
// ---------------------------------------------------------------------------------------------------------------------
// the kernel of a form (only the one asked for is instantiated)
template <int DB, class PHI, int FORM>
static constexpr auto tiled_kernel() {
  if constexpr (FORM == LP_DISP)
    return &k_target_disp_tiled<DB, PHI>;
  else if constexpr (FORM == LP_HIER)
    return &k_target_hier_tiled<DB, PHI>;
  else if constexpr (FORM == LP_GLM)
    return &k_target_glm_tiled<DB, PHI>;
  else
    return &k_target_linpred_tiled<DB, PHI>;
}
template <class T, class PHI, int FORM>
static constexpr auto flat_kernel() {
  if constexpr (FORM == LP_DISP)
    return &k_target_disp<T, PHI>;
  else if constexpr (FORM == LP_HIER)
    return &k_target_hier<T, PHI>;
  else if constexpr (FORM == LP_GLM)
    return &k_target_glm<T, PHI>;
  else
    return &k_target_linpred<T, PHI>;
}

template <int DB, class PHI, int FORM>
static int launch_tiled(const TgtTiledArgs &a) {
  // dispersion form: + the d phi / d lambda partial sums (sL's shape) and the table term's [2][8][32] partials
  const size_t lds = (size_t)(LpGeo<DB>::FLOATS + (FORM == LP_DISP ? LP_WAVES * 64 + 2 * LP_BLOCK : 0)) * sizeof(float);
  constexpr auto kern = tiled_kernel<DB, PHI, FORM>();
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<kern>(ctx, lds));
  const LinpredConsts k = linpred_consts(a.t, a.d);
  ProfScope ps(ctx, "target_linpred");
  if constexpr (FORM == LP_HIER || FORM == LP_DISP)
    return tgt_launch_tiled<kern>(a, lds, a.d, (int)k.rows, a.N, a.yt, (const float *)a.t->p0, (const float *)a.t->p1, (int)a.t->s1);
  else
    return tgt_launch_tiled<kern>(a, lds, a.d, (int)k.rows, a.N, a.yt, (const float *)a.t->p0, (const float *)a.t->p1, (float)k.c, (float)k.pw);
}

template <class T, class PHI, int FORM>
static int launch_flat(const TgtFlatArgs &a) {
  const size_t lds = (size_t)((LPF_SPB + LPF_RB) * (a.d + 1) + LPF_SPB * (LPF_RB + 1)) * sizeof(T);
  constexpr auto kern = flat_kernel<T, PHI, FORM>();
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<kern>(ctx, (size_t)((LPF_SPB + LPF_RB) * (LPF_MAXD + 1) + LPF_SPB * (LPF_RB + 1)) * sizeof(T)));
  const LinpredConsts k = linpred_consts(a.t, a.d);
  ProfScope ps(ctx, "target_linpred");
  if constexpr (FORM == LP_HIER || FORM == LP_DISP)
    return tgt_launch_flat<kern, T>(a, lds, a.d, (int)k.rows, a.N, (const T *)a.y, (const T *)a.t->p0, (const T *)a.t->p1, (int)a.t->s1);
  else
    return tgt_launch_flat<kern, T>(a, lds, a.d, (int)k.rows, a.N, (const T *)a.y, (const T *)a.t->p0, (const T *)a.t->p1, (T)k.c, (T)k.pw);
}

// f(PHI(), std::integral_constant<int, FORM>()) for the row function and the form of the kind
template <class F>
static int linpred_dispatch_kind(int kind, F &&f) {
  using std::integral_constant;
  switch (kind) {
    case NF_TARGET_DENSEGAUSS: return f(PhiHalfSquare(), integral_constant<int, LP_CENTRED>());
    case NF_TARGET_LOGREG: return f(PhiLogSigmoid(), integral_constant<int, LP_CENTRED>());
    case NF_TARGET_GLM_LOGIT: return f(PhiLogSigmoid(), integral_constant<int, LP_GLM>());
    case NF_TARGET_GLM_PROBIT: return f(PhiLogNormCdf(), integral_constant<int, LP_GLM>());
    case NF_TARGET_GLM_POISSON: return f(PhiNegExp(), integral_constant<int, LP_GLM>());
    case NF_TARGET_GLM_STUDENT: return f(PhiStudent(), integral_constant<int, LP_GLM>());
    case NF_TARGET_GLM_NORMAL: return f(PhiHalfSquare(), integral_constant<int, LP_GLM>());
    case NF_TARGET_HGLM_LOGIT: return f(PhiLogSigmoid(), integral_constant<int, LP_HIER>());
    case NF_TARGET_HGLM_PROBIT: return f(PhiLogNormCdf(), integral_constant<int, LP_HIER>());
    case NF_TARGET_HGLM_POISSON: return f(PhiNegExp(), integral_constant<int, LP_HIER>());
    case NF_TARGET_HGLM_STUDENT: return f(PhiStudent(), integral_constant<int, LP_HIER>());
    case NF_TARGET_HGLM_NORMAL: return f(PhiHalfSquare(), integral_constant<int, LP_HIER>());
    case NF_TARGET_DGLM_NORMAL: return f(DispScale<PhiHalfSquare>(), integral_constant<int, LP_DISP>());
    case NF_TARGET_DGLM_STUDENT: return f(DispScale<PhiStudent>(), integral_constant<int, LP_DISP>());
    case NF_TARGET_DGLM_NEGBIN: return f(DispNegBin(), integral_constant<int, LP_DISP>());
    default: return NF_ERR_ARG;
  }
}

int nf_launch_target_linpred_tiled(const TgtTiledArgs &a) {
  if (a.d > LPF_MAXD) return NF_ERR_UNSUPPORTED;
  return linpred_dispatch_kind(a.t->kind, [&](auto phi, auto form) {
    return tgt_dispatch_db(a.d, [&](auto db) { return launch_tiled<db(), decltype(phi), form()>(a); });
  });
}

int nf_launch_target_linpred(const TgtFlatArgs &a) {
  if (a.d > LPF_MAXD) return NF_ERR_UNSUPPORTED;
  return linpred_dispatch_kind(a.t->kind, [&](auto phi, auto form) {
    return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_flat<decltype(e), decltype(phi), form()>(a); });
  });
}
