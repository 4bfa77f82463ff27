// nf_distreg.hip -- the distributional regression targets (NF_TARGET_DR_NORMAL / STUDENT / ZIPOISSON / WEIBULL; gfx950): TWO linear
// predictors per data row, joined inside a bivariate row function,
//     y = [beta (p) ; gamma (q)], d = p + q,    u = X beta + offu,   v = Z gamma + offv,
//     log p(y) = par[1] + sum_i wt_i phi(u_i, v_i; a_i, par[3]) + lin . y - par[0] |beta|^2 / 2 - par[2] |gamma|^2 / 2,
//     grad     = [X' (wt o phi_u) ; Z' (wt o phi_v)] + lin - [par[0] beta ; par[2] gamma].
// Data: A = [X | Z] [R x d] row-major (the shape the GLM kinds take), s0 = R, s1 = p, and ONE buffer
//     p0 = offu[R] | offv[R] | wt[R] | aux[R] | lin[d] | par[4]         (DrRows below; aux: a 0 / 1 flag per row).
// The row functions (the host folded signs, normalisers and everything linear in y):
//     NORMAL     z = u exp(-v):              -z^2 / 2 - v                                       (u the residual, sigma = exp(v))
//     STUDENT    z = u exp(-v):              -(nu + 1)/2 log1p(z^2 / nu) - v                    (nu = par[3])
//     ZIPOISSON  m = exp(u):                 (a ? logaddexp(v, -m) : -m) - softplus(v)          (a = [count == 0], v the logit of the structural zero)
//     WEIBULL    w = u exp(v):               a (v + w) - exp(w)                                 (a the event flag, u = log t - x . beta, v = log shape)
// Two kernels, the counterparts of nf_linpred.hip's:
//   k_target_distreg_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_distreg        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// A row of weight 0 contributes exactly 0 to the value and to both gradient blocks by SELECT; rows >= R read weight 0.  Nothing is
// clamped.  z and w are formed BEFORE they are squared or exponentiated (u^2 exp(-2 v) would overflow float32 where z^2 does not);
// every exponential of ZIPOISSON's zero branch has a non-positive argument (exp(-|v + m|), exp(-|v|)).  No atomics: two launches give
// the same bits.
// Shared stages: tgt_gemm1 (both predictors' k-loops), tgt_elbo_term, tgt_block_partial and the launch helpers (nf_target_stages.h),
// glm_weigh and the lp_* transcendentals (nf_linpred.h).  The staging of [X | Z] with the gap between the parts, the tile load with
// its zero rows, the wave-ordered combine, the two-precision epilogue and the flat kernel's y -> sY load stand here in place.
// This file's device code is compiled without packed fp32 arithmetic (the attribute below, device pass only, this translation unit
// only), as nf_mixglm.hip's is: the middle is scalar code per accumulator register next to MFMAs.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define DR_BLOCK 256
#define DR_WAVES 4
#define DR_MAXD 256
#define DR_CW 128  // features of A a wave's image holds at a time

#define DR_NORMAL 0
#define DR_STUDENT 1
#define DR_ZIPOISSON 2
#define DR_WEIBULL 3

// The row data, addressed inside the one buffer p0 = offu[R] | offv[R] | wt[R] | aux[R] | lin[d] | par[4].
template <class T>
struct DrRows {
  const T *offu, *offv, *wt, *aux, *lin, *par;
  __device__ __forceinline__ DrRows(const T *p0, int d, int R)
      : offu(p0), offv(p0 + R), wt(p0 + 2 * (long)R), aux(p0 + 3 * (long)R), lin(p0 + 4 * (long)R), par(p0 + 4 * (long)R + d) {}
};

// ---------------------------------------------------------------------------------------------------------------------
// row functions: phi, d phi / d u, d phi / d v of ONE row
// ---------------------------------------------------------------------------------------------------------------------
// log1p(exp(-|x|)), sigmoid(x), sigmoid(-x): e = exp(-|x|) is in (0, 1], nothing overflows for any finite x.  float: the hardware
// exponential, logarithm and reciprocal, as PhiLogSigmoid (1 + e is in (1, 2]: an absolute error of one ulp of 1).
struct DrSig {
  static __device__ __forceinline__ void eval(double x, double &l, double &s, double &sm) {
    const double e = exp(-fabs(x)), r = 1.0 / (1.0 + e);
    l = log1p(e);
    s = x >= 0.0 ? r : e * r;
    sm = x >= 0.0 ? e * r : r;
  }
  static __device__ __forceinline__ void eval(float x, float &l, float &s, float &sm) {
    const float e = nf_exp(-fabsf(x)), t = 1.f + e, r = __builtin_amdgcn_rcpf(t);
    l = nf_log(t);
    s = x >= 0.f ? r : e * r;
    sm = x >= 0.f ? e * r : r;
  }
};

// the reciprocal by element type: the hardware's in float (1 ulp), a division in double
__device__ __forceinline__ float dr_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double dr_rcp(double x) { return 1.0 / x; }

template <int FAM>
struct DrPhi {
  static constexpr bool FLAG = FAM == DR_ZIPOISSON || FAM == DR_WEIBULL;  // the family reads aux
  template <class T>
  static __device__ __forceinline__ void eval(T u, T v, bool a, T nu, T &phi, T &du, T &dv) {
    if constexpr (FAM == DR_NORMAL) {
      const T ei = lp_exp(-v), z = u * ei;
      phi = (T)-0.5 * z * z - v;
      du = -z * ei;
      dv = z * z - (T)1;
    } else if constexpr (FAM == DR_STUDENT) {
      // ONE reciprocal per row, r = 1 / (nu + z^2) (1 / nu is uniform over the launch: hoisted); z^2 / (nu + z^2) is written
      // 1 - nu r: where z^2 overflows it tends to its limit, not to inf / inf
      const T ei = lp_exp(-v), z = u * ei, z2 = z * z, r = dr_rcp(nu + z2);
      phi = (T)-0.5 * (nu + (T)1) * lp_log1p(z2 * dr_rcp(nu)) - v;
      du = -(nu + (T)1) * z * ei * r;
      dv = (nu + (T)1) * ((T)1 - nu * r) - (T)1;
    } else if constexpr (FAM == DR_ZIPOISSON) {
      // a = 0:  -m - softplus(v) ;  -m ;  -sigmoid(v)
      // a = 1:  logaddexp(v, -m) - softplus(v), with t = v + m:  max(v, -m) + log1p(exp(-|t|)) - max(v, 0) - log1p(exp(-|v|)) ;
      //         -m sigmoid(-t) ;  sigmoid(t) - sigmoid(v) = sigmoid(-v) - sigmoid(-t) (the second form for v >= 0: no cancellation near 1)
      const T m = lp_exp(u);
      T lv, sv, smv, lt, st, smt;
      DrSig::eval(v, lv, sv, smv);
      DrSig::eval(v + m, lt, st, smt);
      const T sp = (v > (T)0 ? v : (T)0) + lv;  // softplus(v)
      const T hd = v > (T)0 ? (T)0 : (v > -m ? v : -m);  // max(v, -m) - max(v, 0)  (m > 0)
      phi = a ? hd + (lt - lv) : -m - sp;
      du = a ? -m * smt : -m;
      dv = a ? (v >= (T)0 ? smv - smt : st - sv) : -sv;
    } else {
      const T ev = lp_exp(v), w = u * ev, ew = lp_exp(w), f = (a ? (T)1 : (T)0) - ew;
      phi = (a ? v + w : (T)0) - ew;
      du = f * ev;
      dv = (a ? (T)1 : (T)0) + w * f;
    }
  }
};

// phi, phi_u, phi_v of one row under its weight: exactly 0 for weight 0, by select
template <class T>
__device__ __forceinline__ void dr_weigh(T w, T &phi, T &du, T &dv) {
  glm_weigh(w, phi, du);
  dv = w == (T)0 ? (T)0 : w * dv;
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The tile sits in LDS,
// [feature][sample], features >= d and padding samples zero, with eight zero feature rows behind the 32 DB (V's k-loop runs up to 7
// features past d).  Each wave takes the row blocks rb = wave, wave + 4, ... of A (32 rows) and stages its block into an image of its
// own, one chunk of at most 128 features at a time (d <= 128: the whole block, once).  A chunk [f0, f0 + pc) holds px features of X
// and qz of Z (either may be 0); in the image the X part sits at column 0 and the Z part at column PX8, the next multiple of 8 past
// px, with zero columns between and behind, up to a multiple of 8:
//     image columns   [0, px) X | [px, PX8) 0 | [PX8, PX8 + qz) Z | .. W8) 0          row stride S odd: both GEMMs free of bank conflicts
// so both k-loops of GEMM 1 run in whole 8-feature groups for ANY p: a zero image column meets whatever tile row stands there.
//   GEMM 1   U[i][j] = offu_i + sum_f X[i][f] Y[f][j],   V[i][j] = offv_i + sum_f Z[i][f] Y[p + f][j]     (the offsets are the initial
//            accumulators; the two sets are filled from ONE staging of the block, tgt_gemm1 at image column 0 / PX8)
//   phi      in the accumulator registers, ONE pass with both predictors live: register r of a lane of half `hi` is row nf_row(r, hi)
//            of sample l & 31; wt by select; wt phi_u replaces U, wt phi_v replaces V, which ARE
//   GEMM 2   G[f][j] += sum_i X[i][f] (wt phi_u)[i][j]  (f < p),   G[f][j] += sum_i Z[i][f - p] (wt phi_v)[i][j]  (f >= p)    's B operands
//            (the register chaining of nf_mfma.h).  The outputs are the global 32-feature blocks of y: a block that straddles p takes
//            one MFMA set per part, the A operand read at the part's image column, lanes outside the part zero.
// d > 128 (DB = 8 only) takes two chunks: GEMM 1 accumulates over them, GEMM 2 runs over them in reverse, so the last chunk of
// GEMM 1 is the first of GEMM 2 and only the other one is staged again.  The 16 weights of a lane stay in registers across the
// middle; the 16 aux flags are ONE register (bit r).  The four waves' G and log-p sums are combined through LDS in wave order.
// Up to DB = 4 the kernel is held to 256 registers (two workgroups per CU where their LDS fits, d <= 102: one's row functions run
// under the other's matrix instructions); DB = 8 carries 128 gradient accumulators and keeps the whole register file.
template <int DB>
struct DrGeo {
  static constexpr int YT = 32 * DB * 32;  // the tile; reused for the reduction of G over the four waves
  static constexpr int YTP = YT + 8 * 32;  // with the eight zero feature rows behind it
  // px + 7 + qz + 7 >= W8: the odd stride past the widest image of a chunk of min(d, 128) features
  __host__ __device__ static constexpr int stride(int d) { return ((d < DR_CW ? d : DR_CW) + 15) | 1; }
  __host__ __device__ static constexpr int floats(int d) { return YTP + DR_WAVES * 32 * stride(d); }
};

// where a chunk's parts stand: in y (f0, px features of X; zlo, qz features of Z) and in the image (0; PX8; W8 columns in all)
struct DrChunk {
  int f0, pc, px, qz, zlo, PX8, W8;
  __device__ __forceinline__ DrChunk(int ch, int d, int p) {
    f0 = ch * DR_CW;
    pc = d - f0 < DR_CW ? d - f0 : DR_CW;
    px = p - f0 < 0 ? 0 : (p - f0 < pc ? p - f0 : pc);
    qz = pc - px;
    zlo = f0 + px;
    PX8 = (px + 7) & ~7;
    W8 = PX8 + ((qz + 7) & ~7);
  }
};

// rows [i0, i0 + 32) of A, the chunk's features -> the wave's image, the gap and the tail zero, rows >= R zero.  A half-wave copies
// 32 consecutive image columns of one row; every load of a column block is issued before its first store.
__device__ __forceinline__ void dr_stage(float *__restrict__ img, int S, const float *__restrict__ A, int i0, int R, int d, const DrChunk &c, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  for (int cb = 0; cb * 32 < c.W8; ++cb) {
    const int col = cb * 32 + l31;
    const int f = col < c.px ? c.f0 + col : (col >= c.PX8 && col - c.PX8 < c.qz) ? c.zlo + col - c.PX8 : -1;
    float v[16];
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) {
      const int i = i0 + 2 * rp + hi;
      v[rp] = (f >= 0 && i < R) ? A[(long)i * d + f] : 0.f;
    }
    if (col < c.W8) {
#pragma unroll
      for (int rp = 0; rp < 16; ++rp) img[(2 * rp + hi) * S + col] = v[rp];
    }
  }
}

// G += part' D for the features [lo, hi_) of output block b, feature `lo` standing at image column `c0`: lanes outside the part read
// column c0 and multiply by zero
__device__ __forceinline__ f32x16 dr_gemm2(f32x16 G, const float *__restrict__ img, int S, int b, int lo, int hi_, int c0, const f32x16 &D, int l31,
                                           int hi) {
  const int f = b * 32 + l31;
  const bool in = f >= lo && f < hi_;
  const float *pa = img + (4 * hi) * S + c0 + (in ? f - lo : 0);
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float a = pa[((t & 3) + 8 * (t >> 2)) * S];
    G = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? a : 0.f, D[t], G, 0, 0, 0);
  }
  return G;
}

template <int FAM, int DB>
__global__ __launch_bounds__(DR_BLOCK, DB <= 4 ? 2 : 1) void k_target_distreg_tiled(int d, int p, int R, long N, const float *__restrict__ yt,
                                                                                   const float *__restrict__ p0, const float *__restrict__ A,
                                                                                   const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                                   float *__restrict__ gt, float gscale, float *__restrict__ elbos_out,
                                                                                   double *__restrict__ partial, double pscale) {
  using G = DrGeo<DB>;
  using PHI = DrPhi<FAM>;
  const DrRows<float> rd(p0, d, R);
  const int S = G::stride(d);
  const int nch = DB == 8 ? (d + DR_CW - 1) / DR_CW : 1;  // (d <= 128 below DB = 8)
  extern __shared__ float dr_lds[];
  float *sY = dr_lds;
  float *sA = dr_lds + G::YTP;
  __shared__ float sL[DR_WAVES][64];  // [wave][lane] log-p partial sums
  __shared__ float redb[DR_BLOCK / 32][32], redg[DR_BLOCK / 32][32], redl[DR_BLOCK / 32][32];
  __shared__ double sm[DR_WAVES];
  const long tile = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // a scalar: so are rb and every chunk's geometry
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;
  const float nu = rd.par[3];

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YTP / DR_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * DR_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * DR_BLOCK] = yv[k];
  }
  __syncthreads();

  float *img = sA + wave * 32 * S;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f;
  const int nrb = (R + 31) >> 5;
  for (int rb = wave; rb < nrb; rb += DR_WAVES) {
    const int i0 = rb * 32;
    float wt[16];
    unsigned flags = 0;  // bit r: the aux flag of row nf_row(r, hi)
    f32x16 U, V;
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // (requested before the staging loads: in by the time the image is)
      const int i = i0 + nf_row(r, hi);
      U[r] = i < R ? rd.offu[i] : 0.f;
      V[r] = i < R ? rd.offv[i] : 0.f;
      wt[r] = i < R ? rd.wt[i] : 0.f;
      if constexpr (PHI::FLAG) flags |= (i < R && rd.aux[i] != 0.f) ? 1u << r : 0u;
    }
    for (int ch = 0; ch < nch; ++ch) {
      const DrChunk c(ch, d, p);
      dr_stage(img, S, A, i0, R, d, c, lane);
      wave_lds_fence();
      U = tgt_gemm1(U, img, S, sY + c.f0 * 32, c.px, l31, hi);
      V = tgt_gemm1(V, img + c.PX8, S, sY + c.zlo * 32, c.qz, l31, hi);
      if (ch + 1 < nch) wave_lds_fence();  // the next chunk overwrites the image
    }

    // the middle: both predictors of a row are live; the two partial derivatives replace them
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ph, du, dv;
      PHI::eval(U[r], V[r], (bool)((flags >> r) & 1u), nu, ph, du, dv);
      dr_weigh(wt[r], ph, du, dv);
      lp += ph;
      U[r] = du;
      V[r] = dv;
    }

    for (int ch = nch - 1; ch >= 0; --ch) {
      const DrChunk c(ch, d, p);
      if (ch != nch - 1) {
        wave_lds_fence();
        dr_stage(img, S, A, i0, R, d, c, lane);
        wave_lds_fence();
      }
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        if (b * 32 >= c.f0 && b * 32 < c.f0 + c.pc) {  // (wave-uniform) block b holds features of this chunk
          if (b * 32 < c.zlo) Gacc[b] = dr_gemm2(Gacc[b], img, S, b, c.f0, c.zlo, 0, U, l31, hi);                            // its X part
          if (b * 32 + 32 > c.zlo && c.qz > 0) Gacc[b] = dr_gemm2(Gacc[b], img, S, b, c.zlo, c.f0 + c.pc, c.PX8, V, l31, hi);  // its Z part
        }
      }
    }
    wave_lds_fence();  // the next staging overwrites the image
  }

  // the four waves' G and log-p sums, combined in wave order
  sL[wave][lane] = lp;
  for (int w = 0; w < DR_WAVES; ++w) {
    __syncthreads();  // (first pass: every wave is done reading the tile)
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < DB; ++b)
        if (b * 32 < d) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float *q = sY + (b * 32 + nf_row(r, hi)) * 32 + l31;
            *q = w == 0 ? Gacc[b][r] : *q + Gacc[b][r];
          }
        }
    }
  }
  __syncthreads();

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s; the prior has one precision per part
  const float pwb = rd.par[0], pwg = rd.par[2];
  const int s = threadIdx.x & 31, qf = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yb2 = 0.f, yg2 = 0.f, ly = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER], lv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = qf + k * (DR_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
      lv[k] = i < d ? rd.lin[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = qf + k * (DR_BLOCK / 32);
      const float y2 = yv[k] * yv[k];
      yb2 += i < p ? y2 : 0.f;
      yg2 += i < p ? 0.f : y2;
      ly += lv[k] * yv[k];
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] + lv[k] - (i < p ? pwb : pwg) * yv[k]) : 0.f;
    }
  }
  redb[qf][s] = yb2;
  redg[qf][s] = yg2;
  redl[qf][s] = ly;
  __syncthreads();
  double contrib = 0.0;
  if (qf == 0 && valid) {
    float tb = 0.f, tg = 0.f, tl = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < DR_BLOCK / 32; ++k) tb += redb[k][s];
#pragma unroll
    for (int k = 0; k < DR_BLOCK / 32; ++k) tg += redg[k][s];
#pragma unroll
    for (int k = 0; k < DR_BLOCK / 32; ++k) tl += redl[k][s];
#pragma unroll
    for (int w = 0; w < DR_WAVES; ++w) l += sL[w][s] + sL[w][32 + s];
    const float e = rd.par[1] + l + tl - 0.5f * pwb * tb - 0.5f * pwg * tg;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  A passes through LDS in blocks of
// 16 rows: lane q of a sample takes row q (u over the features < p, v over the rest, phi and its two derivatives), the derivatives
// go through LDS, and lane q then owns the features q, q + 16, ... of the gradient, each under its own part's derivative.
// The three sums over features / rows (u, v, g) are kept in DOUBLE in either element type: phi_u and phi_v carry exp(-2 v), which
// multiplies the rounding of a sequential float sum of v by two -- 75 features at float put the score's rms error at the tolerance
// itself, where the same form summed pairwise sits at a tenth of it.  This is the path of nf_target_logp and Float64 flows, not the hot one.
#define DRF_LANES 16
#define DRF_SPB (DR_BLOCK / DRF_LANES)
#define DRF_RB 16

template <int FAM, class T>
__global__ __launch_bounds__(DR_BLOCK) void k_target_distreg(int d, int p, int R, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                             const T *__restrict__ A, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale, T *__restrict__ elbos_out,
                                                             double *__restrict__ partial, double pscale) {
  using PHI = DrPhi<FAM>;
  const DrRows<T> rd(p0, d, R);
  extern __shared__ double drf_lds[];
  const int S = d + 1, SD = DRF_RB + 1;
  T *sY = (T *)drf_lds;          // [sample][d + 1]
  T *sA = sY + DRF_SPB * S;      // [row][d + 1]
  T *sDu = sA + DRF_RB * S;      // [sample][17] wt phi_u
  T *sDv = sDu + DRF_SPB * SD;   // [sample][17] wt phi_v
  __shared__ double sm[DR_BLOCK / 64];
  const int q = threadIdx.x & (DRF_LANES - 1), sl = threadIdx.x / DRF_LANES;
  const long j = (long)blockIdx.x * DRF_SPB + sl;
  const bool valid = j < N;
  const T nu = rd.par[3], pwb = rd.par[0], pwg = rd.par[2];
  for (int idx = threadIdx.x; idx < DRF_SPB * d; idx += DR_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * DRF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  double g[DR_MAXD / DRF_LANES];
#pragma unroll
  for (int k = 0; k < DR_MAXD / DRF_LANES; ++k) g[k] = 0.0;
  T lp = 0;
  for (int i0 = 0; i0 < R; i0 += DRF_RB) {
    const bool live = i0 + q < R;  // (requested with the block of A)
    const T ou = live ? rd.offu[i0 + q] : (T)0, ov = live ? rd.offv[i0 + q] : (T)0, wv = live ? rd.wt[i0 + q] : (T)0;
    const bool av = PHI::FLAG && live && rd.aux[i0 + q] != (T)0;
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < DRF_RB * d; idx += DR_BLOCK) {
      const int row = idx / d, f = idx - row * d;
      sA[row * S + f] = i0 + row < R ? A[(long)(i0 + row) * d + f] : (T)0;
    }
    __syncthreads();
    double u = ou, v = ov;
    for (int f = 0; f < p; ++f) u += (double)sA[q * S + f] * (double)sY[sl * S + f];
    for (int f = p; f < d; ++f) v += (double)sA[q * S + f] * (double)sY[sl * S + f];
    T ph, du, dv;
    PHI::eval((T)u, (T)v, av, nu, ph, du, dv);
    dr_weigh(wv, ph, du, dv);
    lp += ph;
    sDu[sl * SD + q] = du;
    sDv[sl * SD + q] = dv;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DR_MAXD / DRF_LANES; ++k) {
      const int f = k * DRF_LANES + q;
      if (f < d) {
        double a = g[k];
        const T *pd = (f < p ? sDu : sDv) + sl * SD;
#pragma unroll
        for (int r = 0; r < DRF_RB; ++r) a += (double)sA[r * S + f] * (double)pd[r];
        g[k] = a;
      }
    }
  }
  T yb2 = 0, yg2 = 0, ly = 0;
#pragma unroll
  for (int k = 0; k < DR_MAXD / DRF_LANES; ++k) {
    const int f = k * DRF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f], lv = rd.lin[f];
      yb2 += f < p ? yv * yv : (T)0;
      yg2 += f < p ? (T)0 : yv * yv;
      ly += lv * yv;
      if (grad_out) grad_out[j * d + f] = gscale * ((T)g[k] + lv - (f < p ? pwb : pwg) * yv);
    }
  }
  lp = group16_sum(lp);
  yb2 = group16_sum(yb2);
  yg2 = group16_sum(yg2);
  ly = group16_sum(ly);
  double contrib = 0.0;
  if (valid && q == 0) {
    const T e = rd.par[1] + lp + ly - (T)0.5 * pwb * yb2 - (T)0.5 * pwg * yg2;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = R, s1 = p in 1 .. d - 1, d <= 256)
// ---------------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, FAM>) for the family of a distributional kind
template <class F>
static int dr_dispatch_family(int kind, F &&f) {
  switch (kind) {
    case NF_TARGET_DR_NORMAL: return f(std::integral_constant<int, DR_NORMAL>());
    case NF_TARGET_DR_STUDENT: return f(std::integral_constant<int, DR_STUDENT>());
    case NF_TARGET_DR_ZIPOISSON: return f(std::integral_constant<int, DR_ZIPOISSON>());
    default: return f(std::integral_constant<int, DR_WEIBULL>());
  }
}

template <int FAM, int DB>
static int launch_distreg_tiled(const TgtTiledArgs &a) {
  using G = DrGeo<DB>;
  nf_ctx *ctx = a.ctx;
  NF_TRY((nf_lds_once<k_target_distreg_tiled<FAM, DB>>(ctx, G::floats(32 * DB) * sizeof(float))));
  ProfScope ps(ctx, "target_distreg");
  return tgt_launch_tiled<k_target_distreg_tiled<FAM, DB>>(a, (size_t)G::floats(a.d) * sizeof(float), a.d, (int)a.t->s1, (int)a.t->s0, a.N, a.yt,
                                                           (const float *)a.t->p0, (const float *)a.t->p1);
}

int nf_launch_target_distreg_tiled(const TgtTiledArgs &a) {
  if (a.d > DR_MAXD) return NF_ERR_UNSUPPORTED;
  return dr_dispatch_family(a.t->kind, [&](auto fam) { return tgt_dispatch_db(a.d, [&](auto db) { return launch_distreg_tiled<decltype(fam)::value, decltype(db)::value>(a); }); });
}

// elements of LDS the flat kernel takes at d
static size_t distreg_flat_lds(int d) { return (size_t)((DRF_SPB + DRF_RB) * (d + 1) + 2 * DRF_SPB * (DRF_RB + 1)); }

template <int FAM, class T>
static int launch_distreg_flat(const TgtFlatArgs &a) {
  nf_ctx *ctx = a.ctx;
  NF_TRY((nf_lds_once<k_target_distreg<FAM, T>>(ctx, distreg_flat_lds(DR_MAXD) * sizeof(T))));  // the most any served target takes
  ProfScope ps(ctx, "target_distreg");
  return tgt_launch_flat<k_target_distreg<FAM, T>, T>(a, distreg_flat_lds(a.d) * sizeof(T), a.d, (int)a.t->s1, (int)a.t->s0, a.N, (const T *)a.y,
                                                      (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_distreg(const TgtFlatArgs &a) {
  if (a.d > DR_MAXD) return NF_ERR_UNSUPPORTED;
  return dr_dispatch_family(a.t->kind, [&](auto fam) {
    return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_distreg_flat<decltype(fam)::value, decltype(e)>(a); });
  });
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
