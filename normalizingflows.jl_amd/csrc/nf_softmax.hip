// nf_softmax.hip -- the softmax (multinomial-logit) regression target (NF_TARGET_SOFTMAX; gfx950):
//     y = [w_0; ...; w_{C-1}] in R^d, d = C p (class-major: vec(W) of the p x C weight matrix),   u_{i,c} = x_i . w_c,
//     log p(y) = par[1] + sum_i wt_i (u_{i,c_i} - logsumexp_c u_{i,c}) - par[0] |y|^2 / 2,
//     grad_{w_c} = sum_i wt_i (1[c_i = c] - softmax_c(u_i)) x_i - par[0] w_c
// with X [rows x p] row-major and the row data in ONE buffer p0 = lab[rows] | wt[rows] | par[2] (SmRows below).  The C predictors
// of a row are coupled through the log-sum-exp, which the one-function-per-row kernels of nf_linpred.hip cannot express.  Two
// kernels, the counterparts of nf_linpred.hip's:
//   k_target_softmax_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_softmax        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// A row of weight 0 contributes exactly 0 to the value and the gradient by SELECT (a subsampling mask may sit over a row whose
// logits are not finite); the log-sum-exp subtracts the row maximum, so nothing overflows for finite logits; nothing is clamped.
// Shared stages (nf_target_stages.h): tgt_stage_rows and tgt_gemm1_at (the wave's image of a row block; U_c from it and the tile at
// feature c p), tgt_elbo_term and tgt_block_partial (the ELBO tail of both kernels), and the launch helpers; what stands here in
// place does so for nf_ordinal.hip's reason.
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

// The row data, addressed inside the one buffer p0 = lab[rows] | wt[rows] | par[2]: labels as integer-valued elements,
// par[0] the prior precision 1 / sigma^2 (0: the flat prior), par[1] the additive constant the host folded.
template <class T>
struct SmRows {
  const T *lab, *wt, *par;
  __device__ __forceinline__ SmRows(const T *p0, int rows) : lab(p0), wt(p0 + rows), par(p0 + 2 * (long)rows) {}
};

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The tile sits
// uncentred in LDS, [feature][sample], features >= d and padding samples zero, with eight zero feature rows behind the
// 32 DB (the last class's k-loop runs up to 7 features past d).  Each wave takes the row blocks rb = wave, wave + 4, ... of X
// (32 rows each) and stages its block ONCE into an image of its own, 32 rows x p features (p <= d / 2 <= 128: one chunk):
//   GEMM 1   U_c[i][j] = sum_f X[i][f] Y[c p + f][j]   the A operand is the same image for every class, the B operand pointer
//                                                      advances by 32 p floats per class.  k-steps pair features: with p odd
//                                                      the partner of the last feature belongs to the next class and meets
//                                                      the image's zero column p
//   soft-max in the accumulator registers: register r of a lane of half `hi` is row nf_row(r, hi) of sample l & 31.  TWO passes
//            over the classes, GEMM 1 recomputed in the second: pass 1 keeps a running maximum m, the sum s of exp(U_c - m)
//            (rescaled when m moves) and the label's logit; pass 2 forms phi'_c = wt (1[c_i = c] - exp(U_c - m) / s).  Three
//            register sets beside the gradient accumulators whatever C is
//   GEMM 2   G[c p + f][j] += sum_i X[i][f] phi'_c[i][j]   its B operand IS the accumulator register of GEMM 1 (the register
//                                                      chaining of nf_mfma.h).  The output blocks are the global 32-feature
//                                                      blocks of y: a block takes one MFMA set per class it overlaps, the A
//                                                      operand read at the class's column offset, lanes outside the class zero
// Rows >= rows read wt = 0, which masks them.  Combine and epilogue are lp_tiled_body's.
// Up to DB = 4 the kernel is held to 256 registers (two workgroups per CU: one's soft-max runs under the other's matrix
// instructions; measured); DB = 8 carries 128 gradient accumulators and keeps the whole register file.
#define SM_BLOCK 256
#define SM_WAVES 4

template <int DB>
struct SmGeo {
  static constexpr int CW = DB <= 2 ? 32 : 16 * DB;  // image width: p <= d / 2 <= 16 DB, in whole 32-feature blocks
  static constexpr int S = CW + 1;                   // odd row stride: GEMM 1 (lanes along rows) and GEMM 2 (lanes along features) both conflict-free
  static constexpr int IMG = 32 * S;                 // floats per wave
  static constexpr int YT = 32 * DB * 32;            // the tile; reused for the reduction of G over the four waves
  static constexpr int YTP = YT + 8 * 32;            // with the eight zero feature rows behind it
  static constexpr int FLOATS = YTP + SM_WAVES * IMG + SM_WAVES * 64;
};

template <int DB>
__global__ __launch_bounds__(SM_BLOCK, DB <= 4 ? 2 : 1) void k_target_softmax_tiled(int d, int C, int rows, long N, const float *__restrict__ yt,
                                                                   const float *__restrict__ p0, const float *__restrict__ X,
                                                                   const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                   float *__restrict__ gt, float gscale, float *__restrict__ elbos_out,
                                                                   double *__restrict__ partial, double pscale) {
  using G = SmGeo<DB>;
  const SmRows<float> rd(p0, rows);
  const float pw = rd.par[0];
  const int p = d / C;
  extern __shared__ float sm_lds[];
  float *sY = sm_lds;
  float *sA = sm_lds + G::YTP;
  float *sL = sA + SM_WAVES * G::IMG;  // [wave][lane] log-p partial sums
  __shared__ float red[SM_BLOCK / 32][32];
  __shared__ double sm[SM_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YTP / SM_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * SM_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * SM_BLOCK] = yv[k];
  }
  __syncthreads();

  float *img = sA + wave * G::IMG;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f;
  const int nrb = (rows + 31) >> 5;
  for (int rb = wave; rb < nrb; rb += SM_WAVES) {
    const int i0 = rb * 32;
    float lab[16], wt[16];  // (requested before the staging loads: in by the time the image is)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + nf_row(r, hi);
      lab[r] = i < rows ? rd.lab[i] : -1.f;
      wt[r] = i < rows ? rd.wt[i] : 0.f;
    }
    tgt_stage_rows(img, G::S, X, i0, rows, p, lane);
    wave_lds_fence();

    // pass 1: running maximum, sum of exponentials, the label's logit
    f32x16 m = tgt_gemm1_at(img, G::S, sY, 0, p, l31, hi);
    float s[16], ul[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = 1.f;
      ul[r] = m[r];  // (replaced below unless the label is 0)
    }
    for (int c = 1; c < C; ++c) {
      const f32x16 U = tgt_gemm1_at(img, G::S, sY, c * p, p, l31, hi);
      const float fc = (float)c;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool up = U[r] > m[r];
        const float e = nf_exp(up ? m[r] - U[r] : U[r] - m[r]);  // exp(-|U - m|): one exponential moves the sum either way
        s[r] = up ? fmaf(s[r], e, 1.f) : s[r] + e;
        m[r] = up ? U[r] : m[r];
        ul[r] = lab[r] == fc ? U[r] : ul[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ph = (ul[r] - m[r]) - nf_log(s[r]);
      lp += wt[r] == 0.f ? 0.f : wt[r] * ph;
      s[r] = __builtin_amdgcn_rcpf(s[r]);
    }

    // pass 2: phi'_c in GEMM 1's accumulator registers, straight into GEMM 2
    for (int c = 0; c < C; ++c) {
      f32x16 U = tgt_gemm1_at(img, G::S, sY, c * p, p, l31, hi);
      const float fc = (float)c;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sp = nf_exp(U[r] - m[r]) * s[r];
        U[r] = wt[r] == 0.f ? 0.f : wt[r] * ((lab[r] == fc ? 1.f : 0.f) - sp);
      }
      const int f_lo = c * p, f_hi = f_lo + p;  // the class's features
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        if (b * 32 < f_hi && b * 32 + 32 > f_lo) {  // (wave-uniform) block b overlaps the class
          const int col = b * 32 + l31 - f_lo;
          const bool in = col >= 0 && col < p;
          const float *pa = img + (4 * hi) * G::S + (in ? col : 0);
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const float a = pa[((t & 3) + 8 * (t >> 2)) * G::S];
            Gacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? a : 0.f, U[t], Gacc[b], 0, 0, 0);
          }
        }
      }
    }
    wave_lds_fence();  // the next staging overwrites the image
  }

  // the four waves' G and log-p sums, combined in wave order
  sL[wave * 64 + lane] = lp;
  for (int w = 0; w < SM_WAVES; ++w) {
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

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (SM_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (SM_BLOCK / 32);
      yy += yv[k] * yv[k];
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] - pw * yv[k]) : 0.f;
    }
  }
  red[q][s] = yy;
  __syncthreads();
  double contrib = 0.0;
  if (q == 0 && valid) {
    float t = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < SM_BLOCK / 32; ++k) t += red[k][s];
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) l += sL[w * 64 + s] + sL[w * 64 + 32 + s];
    float e = rd.par[1] + l - 0.5f * pw * t;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  X passes through LDS in
// blocks of 16 rows: lane q of a sample takes row q -- its C <= 16 logits in registers, the log-sum-exp and the C values
// phi'_c --, the phi' go through LDS as [sample][row][class], and lane q then owns the features q, q + 16, ... of the
// gradient.  The library's own exp / log in either element type.
#define SMF_LANES 16
#define SMF_SPB (SM_BLOCK / SMF_LANES)
#define SMF_RB 16
#define SMF_MAXD 256
#define SMF_MAXC 16

template <class T>
__global__ __launch_bounds__(SM_BLOCK) void k_target_softmax(int d, int C, int rows, long N, const T *__restrict__ y,
                                                             const T *__restrict__ p0, const T *__restrict__ X,
                                                             const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                             T *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  const SmRows<T> rd(p0, rows);
  const T pw = rd.par[0];
  const int p = d / C;
  extern __shared__ double smf_lds[];
  const int S = d + 1, SP = p + 1, SD = SMF_RB * C + 1;
  T *sY = (T *)smf_lds;            // [sample][d + 1]
  T *sA = sY + SMF_SPB * S;        // [row][p + 1]
  T *sD = sA + SMF_RB * SP;        // [sample][row][class] phi' (sample stride 16 C + 1)
  __shared__ double sm[SM_BLOCK / 64];
  const int q = threadIdx.x & (SMF_LANES - 1), sl = threadIdx.x / SMF_LANES;
  const long j = (long)blockIdx.x * SMF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < SMF_SPB * d; idx += SM_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * SMF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  T g[SMF_MAXD / SMF_LANES];
  int gx[SMF_MAXD / SMF_LANES], gc[SMF_MAXD / SMF_LANES];  // feature q + 16 k: its column of X and its class
#pragma unroll
  for (int k = 0; k < SMF_MAXD / SMF_LANES; ++k) {
    g[k] = (T)0;
    const int f = k * SMF_LANES + q, c = f / p;
    gc[k] = c;
    gx[k] = f - c * p;
  }
  T lp = 0;
  for (int i0 = 0; i0 < rows; i0 += SMF_RB) {
    const bool live = i0 + q < rows;
    const T lv = live ? rd.lab[i0 + q] : (T)-1, wv = live ? rd.wt[i0 + q] : (T)0;  // (requested with the block of X)
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < SMF_RB * p; idx += SM_BLOCK) {
      const int row = idx / p, f = idx - row * p;
      sA[row * SP + f] = i0 + row < rows ? X[(long)(i0 + row) * p + f] : (T)0;
    }
    __syncthreads();
    T u[SMF_MAXC];
    T m = 0, ul = 0;
#pragma unroll
    for (int c = 0; c < SMF_MAXC; ++c) {
      if (c < C) {
        T a = 0;
        const T *py = sY + sl * S + c * p;
        for (int f = 0; f < p; ++f) a += sA[q * SP + f] * py[f];
        u[c] = a;
        m = (c == 0 || a > m) ? a : m;
        ul = lv == (T)c ? a : ul;
      } else
        u[c] = 0;
    }
    T s = 0;
#pragma unroll
    for (int c = 0; c < SMF_MAXC; ++c) {
      if (c < C) {
        u[c] = lp_exp(u[c] - m);
        s += u[c];
      }
    }
    const T ph = (ul - m) - lp_log(s);
    lp += wv == (T)0 ? (T)0 : wv * ph;
#pragma unroll
    for (int c = 0; c < SMF_MAXC; ++c) {
      if (c < C) sD[sl * SD + q * C + c] = wv == (T)0 ? (T)0 : wv * ((lv == (T)c ? (T)1 : (T)0) - u[c] / s);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SMF_MAXD / SMF_LANES; ++k) {
      const int f = k * SMF_LANES + q;
      if (f < d) {
        T a = g[k];
        const T *pd = sD + sl * SD + gc[k];
        const T *px = sA + gx[k];
#pragma unroll
        for (int r = 0; r < SMF_RB; ++r) a += px[r * SP] * pd[r * C];
        g[k] = a;
      }
    }
  }
  T yy = 0;
#pragma unroll
  for (int k = 0; k < SMF_MAXD / SMF_LANES; ++k) {
    const int f = k * SMF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f];
      yy += yv * yv;
      if (grad_out) grad_out[j * d + f] = gscale * (g[k] - pw * yv);
    }
  }
  lp = group16_sum(lp);
  yy = group16_sum(yy);
  double contrib = 0.0;
  if (valid && q == 0) {
    T e = rd.par[1] + lp - (T)0.5 * pw * yy;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = rows, s1 = C, d % C == 0)
// ---------------------------------------------------------------------------------------------------------------------
template <int DB>
static int launch_softmax_tiled(const TgtTiledArgs &a) {
  const size_t lds = (size_t)SmGeo<DB>::FLOATS * sizeof(float);
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_softmax_tiled<DB>>(ctx, lds));
  ProfScope ps(ctx, "target_softmax");
  return tgt_launch_tiled<k_target_softmax_tiled<DB>>(a, lds, a.d, (int)a.t->s1, (int)a.t->s0, a.N, a.yt, (const float *)a.t->p0,
                                                      (const float *)a.t->p1);
}

int nf_launch_target_softmax_tiled(const TgtTiledArgs &a) {
  if (a.d > SMF_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_db(a.d, [&](auto db) { return launch_softmax_tiled<db()>(a); });
}

// floats / doubles of LDS the flat kernel takes at (d, C)
static size_t softmax_flat_lds(int d, int C) { return (size_t)(SMF_SPB * (d + 1) + SMF_RB * (d / C + 1) + SMF_SPB * (SMF_RB * C + 1)); }

template <class T>
static int launch_softmax_flat(const TgtFlatArgs &a) {
  const int C = (int)a.t->s1;
  // the most any checked target takes: d = 256, with the widest image (C = 2) and the widest phi' block (C = 16) both counted
  const size_t most = (size_t)(SMF_SPB * (SMF_MAXD + 1) + SMF_RB * (SMF_MAXD / 2 + 1) + SMF_SPB * (SMF_RB * SMF_MAXC + 1)) * sizeof(T);
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_softmax<T>>(ctx, most));
  ProfScope ps(ctx, "target_softmax");
  return tgt_launch_flat<k_target_softmax<T>, T>(a, softmax_flat_lds(a.d, C) * sizeof(T), a.d, C, (int)a.t->s0, a.N, (const T *)a.y,
                                                 (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_softmax(const TgtFlatArgs &a) {
  if (a.d > SMF_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_softmax_flat<decltype(e)>(a); });
}
