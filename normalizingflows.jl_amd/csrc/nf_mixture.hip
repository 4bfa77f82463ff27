// nf_mixture.hip -- the Gaussian-mixture target (NF_TARGET_GAUSSMIX; gfx950): K components MvNormal(mu_k, L_k L_k') with
// weights pi_k,
//     u_k = W_k (y - mbar) - b_k,   q_k = c_k - |u_k|^2 / 2,   log p(y) = logsumexp_k q_k,   grad = -sum_k r_k W_k' u_k,
// W_k = inv(L_k), mbar = sum_k pi_k mu_k, b_k = W_k (mu_k - mbar), c_k = log pi_k + log|det W_k| - d/2 log(2 pi),
// r_k = exp(q_k - log p).  A [K d x d] row-major holds the W_k stacked; p0 = mbar[d] | b[K d] | c[K].  Two kernels, the
// counterparts of nf_linpred.hip's:
//   k_target_mixture_tiled  Float32, tiled layout, d <= 64, drop-in for k_target_linpred_tiled: both GEMMs of every
//                           component on v_mfma_f32_32x32x2_f32, one pass with a running log-sum-exp per sample
//   k_target_mixture        flat layout, float / double, d <= 256, drop-in for k_target_linpred: vector pipe
// Shared stages (nf_target_stages.h): tgt_elbo_term (both kernels), tgt_block_partial (the flat kernel; the tiled one keeps it in
// place), and the launch helpers.  The image here is a whole component, staged and multiplied by its own loops.
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define MX_BLOCK 256
#define MX_WAVES 4

// exp / log of the running log-sum-exp.  double: the library functions (plain IEEE arithmetic around them); float: the
// hardware exponential and logarithm -- the sum S is in [1, K], so log S carries an absolute error of an ulp of log S.
__device__ __forceinline__ double mx_exp(double x) { return exp(x); }
__device__ __forceinline__ double mx_log(double x) { return log(x); }
__device__ __forceinline__ float mx_exp(float x) { return nf_exp(x); }
__device__ __forceinline__ float mx_log(float x) { return nf_log(x); }

// One step of the running log-sum-exp: the state (M, S) takes the term q; `sc` rescales what was accumulated under the old
// maximum, `w` weighs the new term.  M = -inf (nothing taken yet) gives sc = exp(-inf) = 0 exactly, and a term equal to the
// maximum never evaluates (-inf) - (-inf).
template <class T>
__device__ __forceinline__ void mx_take(T q, T &M, T &S, T &sc, T &w) {
  const T Mn = q > M ? q : M;
  sc = M == Mn ? (T)1 : mx_exp(M - Mn);
  w = q == Mn ? (T)1 : mx_exp(q - Mn);
  S = S * sc + w;
  M = Mn;
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile).  The centred tile Y - mbar sits in LDS
// once, [feature][sample], features >= d and padding samples zero.  Wave w takes the WHOLE components k = w, w + 4, ...
// (q_k is a sum over all rows of the component) and stages W_k into an LDS image of its own by (component, row in the
// component) -- a component starts at row k d of A, which is not a multiple of 32 -- zero beyond row d and feature d:
//   GEMM 1   U[rb][i][j] = sum_f W_k[32 rb + i][f] Y[f][j]        as k_target_linpred_tiled
//   u = U - b_k in the accumulator registers (register r of half `hi` is row 32 rb + nf_row(r, hi); rows >= d read b as
//       0), |u|^2 summed per lane and exchanged with lane ^ 32 (low half + high half, in that order, in both halves)
//   q = c_k - |u|^2 / 2 joins the lane's running (M, S); G is rescaled by exp(M - M')
//   GEMM 2   G[fb][f][j] += sum_i W_k[i][f] (-w u)[i][j]           B operand = the registers of GEMM 1
// The four waves' (M, S, G) are combined through LDS in wave order: M* = max M_w, e_w = exp(M_w - M*) (0 for a wave that
// took no component), S* = sum S_w e_w, G* = sum G_w e_w; log p = M* + log S*, grad = G* / S*.
// DB is the exact block count of d (the launcher picks DB = 1 for d <= 32, DB = 2 for 32 < d <= 64): every one of the DB x DB
// blocks of a component holds a real entry, so no loop below tests a block against d -- only rows and features inside a block.
template <int DB>
struct MxGeo {
  static constexpr int S = 32 * DB + 1;         // row stride of the image (odd: both GEMMs read it without bank conflicts)
  static constexpr int IMG = 32 * DB * S;       // floats per wave: all DB row blocks of one component
  static constexpr int YT = 32 * DB * 32;       // the centred tile; reused for the reduction of G over the four waves
  static constexpr int FLOATS = YT + MX_WAVES * IMG + 2 * MX_WAVES * 32;
};

template <int DB>
__global__ __launch_bounds__(MX_BLOCK) void k_target_mixture_tiled(int d, int K, long N, const float *__restrict__ yt,
                                                                   const float *__restrict__ p0, const float *__restrict__ A,
                                                                   const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                   float *__restrict__ gt, float gscale,
                                                                   float *__restrict__ elbos_out, double *__restrict__ partial,
                                                                   double pscale) {
  using G = MxGeo<DB>;
  extern __shared__ float mx_sm[];
  float *sY = mx_sm;
  float *sA = mx_sm + G::YT;
  float *sM = sA + MX_WAVES * G::IMG;  // [wave][sample]
  float *sS = sM + MX_WAVES * 32;
  __shared__ double sm[MX_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;
  const float *bv = p0 + d, *cv = p0 + d + (long)K * d;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YT / MX_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * MX_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] - p0[f] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * MX_BLOCK] = yv[k];
  }
  __syncthreads();

  float *img = sA + wave * G::IMG;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float M = -INFINITY, S = 0.f;
  const int ng = (d + 7) >> 3;  // groups of four k-steps = eight features; features >= d are zero on both sides
  for (int k = wave; k < K; k += MX_WAVES) {
    const float *Ak = A + (long)k * d * d;
    // rows [0, d) x features [0, d) of W_k -> the image, zero in the rest of the 32 DB x 32 DB square
#pragma unroll
    for (int rb = 0; rb < DB; ++rb) {
#pragma unroll
      for (int cb = 0; cb < DB; ++cb) {
        const int f = cb * 32 + l31;
        float v[16];
#pragma unroll
        for (int rp = 0; rp < 16; ++rp) {
          const int i = rb * 32 + 2 * rp + hi;
          v[rp] = (i < d && f < d) ? Ak[(long)i * d + f] : 0.f;
        }
#pragma unroll
        for (int rp = 0; rp < 16; ++rp) img[(rb * 32 + 2 * rp + hi) * G::S + f] = v[rp];
      }
    }
    wave_lds_fence();
    f32x16 U[DB];
    float ss = 0.f;
#pragma unroll
    for (int rb = 0; rb < DB; ++rb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) U[rb][r] = 0.f;
      const float *pa = img + (rb * 32 + l31) * G::S + hi;
      const float *pb = sY + hi * 32 + l31;
      for (int g = 0; g < ng; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          U[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[8 * g + 2 * e], pb[(8 * g + 2 * e) * 32], U[rb], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = rb * 32 + nf_row(r, hi);
        const float u = i < d ? U[rb][r] - bv[(long)k * d + i] : 0.f;
        ss += u * u;
        U[rb][r] = u;
      }
    }
    {
      const float other = __shfl_xor(ss, 32, 64);
      ss = hi ? other + ss : ss + other;  // low half + high half in both halves
    }
    float sc, w;
    mx_take(cv[k] - 0.5f * ss, M, S, sc, w);
#pragma unroll
    for (int b = 0; b < DB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) Gacc[b][r] *= sc;
#pragma unroll
    for (int rb = 0; rb < DB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) U[rb][r] *= -w;
#pragma unroll
    for (int rb = 0; rb < DB; ++rb) {
#pragma unroll
      for (int fb = 0; fb < DB; ++fb) {
        const float *pa = img + (rb * 32 + 4 * hi) * G::S + fb * 32 + l31;
#pragma unroll
        for (int t = 0; t < 16; ++t)
          Gacc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[((t & 3) + 8 * (t >> 2)) * G::S], U[rb][t], Gacc[fb], 0, 0, 0);
      }
    }
    wave_lds_fence();  // the next component overwrites the image
  }

  // the four waves' states, combined in wave order
  if (hi == 0) sM[wave * 32 + l31] = M, sS[wave * 32 + l31] = S;
  __syncthreads();  // (and every wave is done reading the tile)
  {
    float Ms = sM[l31];
#pragma unroll
    for (int w = 1; w < MX_WAVES; ++w) Ms = fmaxf(Ms, sM[w * 32 + l31]);
    const float e = M == -INFINITY ? 0.f : nf_exp(M - Ms);  // a wave without a component adds exactly 0
#pragma unroll
    for (int b = 0; b < DB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) Gacc[b][r] *= e;
  }
  for (int w = 0; w < MX_WAVES; ++w) {  // (the barrier BEHIND each turn: the one above, which the rescaling needs, already frees the tile)
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < DB; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float *p = sY + (b * 32 + nf_row(r, hi)) * 32 + l31;
          *p = w == 0 ? Gacc[b][r] : *p + Gacc[b][r];
        }
      }
    }
    __syncthreads();
  }

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float Ms = sM[s];
#pragma unroll
  for (int w = 1; w < MX_WAVES; ++w) Ms = fmaxf(Ms, sM[w * 32 + s]);
  float Ss = 0.f;
#pragma unroll
  for (int w = 0; w < MX_WAVES; ++w) {
    const float Mw = sM[w * 32 + s];
    Ss += sS[w * 32 + s] * (Mw == -INFINITY ? 0.f : nf_exp(Mw - Ms));
  }
  if (gt) {
#pragma unroll
    for (int k = 0; k < 4 * DB; ++k) {
      const int i = q + k * (MX_BLOCK / 32);
      if (i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] / Ss) : 0.f;
    }
  }
  double contrib = 0.0;
  if (q == 0 && valid) {
    float e = Ms + nf_log(Ss);
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  if (partial) {  // (tgt_block_partial, in place: as a call this kernel gains instructions)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o, 64);
    if (lane == 0) sm[wave] = contrib;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target_linpred's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  Component by
// component, W_k passes through LDS in blocks of 16 rows: lane q of a sample takes row q (u = W_k (y - mbar) - b_k), u goes
// through LDS, and lane q accumulates the features q, q + 16, ... of W_k' u.  At the component's end q_k joins the running
// (M, S) and the score accumulator takes -w W_k' u.  The value is computed by the same instructions whether or not the
// score is asked for.
#define MXF_LANES 16
#define MXF_SPB (MX_BLOCK / MXF_LANES)
#define MXF_RB 16
#define MXF_MAXD 256

template <class T>
__global__ __launch_bounds__(MX_BLOCK) void k_target_mixture(int d, int K, long N, const T *__restrict__ y,
                                                             const T *__restrict__ p0, const T *__restrict__ A,
                                                             const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                             T *__restrict__ elbos_out, double *__restrict__ partial,
                                                             double pscale) {
  extern __shared__ double mxf_sm[];
  T *sY = (T *)mxf_sm;                  // [sample][d + 1] centred
  T *sA = sY + MXF_SPB * (d + 1);       // [row][d + 1]
  T *sD = sA + MXF_RB * (d + 1);        // [sample][17] u
  __shared__ double sm[MX_BLOCK / 64];
  const int q = threadIdx.x & (MXF_LANES - 1), sl = threadIdx.x / MXF_LANES;
  const long j = (long)blockIdx.x * MXF_SPB + sl;
  const bool valid = j < N;
  const int S = d + 1;
  const T *bv = p0 + d, *cv = p0 + d + (long)K * d;
  for (int idx = threadIdx.x; idx < MXF_SPB * d; idx += MX_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * MXF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] - p0[f] : (T)0;
  }
  T g[MXF_MAXD / MXF_LANES], gk[MXF_MAXD / MXF_LANES];
#pragma unroll
  for (int k = 0; k < MXF_MAXD / MXF_LANES; ++k) g[k] = (T)0;
  T M = -(T)INFINITY, Ssum = (T)0;
  for (int kc = 0; kc < K; ++kc) {
    const T *Ak = A + (long)kc * d * d;
    T ss = (T)0;
#pragma unroll
    for (int k = 0; k < MXF_MAXD / MXF_LANES; ++k) gk[k] = (T)0;
    for (int i0 = 0; i0 < d; i0 += MXF_RB) {
      __syncthreads();  // the tile (first pass); the previous block's readers
      for (int idx = threadIdx.x; idx < MXF_RB * d; idx += MX_BLOCK) {
        const int row = idx / d, f = idx - row * d;
        sA[row * S + f] = i0 + row < d ? Ak[(long)(i0 + row) * d + f] : (T)0;
      }
      __syncthreads();
      T u = (T)0;
      for (int f = 0; f < d; ++f) u += sA[q * S + f] * sY[sl * S + f];
      u = i0 + q < d ? u - bv[(long)kc * d + i0 + q] : (T)0;
      ss += u * u;
      if (grad_out) {  // (uniform over the launch)
        sD[sl * (MXF_RB + 1) + q] = u;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MXF_MAXD / MXF_LANES; ++k) {
          const int f = k * MXF_LANES + q;
          if (f < d) {
            T a = gk[k];
#pragma unroll
            for (int r = 0; r < MXF_RB; ++r) a += sA[r * S + f] * sD[sl * (MXF_RB + 1) + r];
            gk[k] = a;
          }
        }
      }
    }
    ss = group16_sum(ss);
    T sc, w;
    mx_take(cv[kc] - (T)0.5 * ss, M, Ssum, sc, w);
#pragma unroll
    for (int k = 0; k < MXF_MAXD / MXF_LANES; ++k) g[k] = g[k] * sc - w * gk[k];
  }
  if (grad_out && valid) {
#pragma unroll
    for (int k = 0; k < MXF_MAXD / MXF_LANES; ++k) {
      const int f = k * MXF_LANES + q;
      if (f < d) grad_out[j * d + f] = gscale * (g[k] / Ssum);
    }
  }
  double contrib = 0.0;
  if (valid && q == 0) {
    T e = M + mx_log(Ssum);
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check)
// ---------------------------------------------------------------------------------------------------------------------
template <int DB>
static int launch_mixture_tiled(const TgtTiledArgs &a) {
  const size_t lds = (size_t)MxGeo<DB>::FLOATS * sizeof(float);
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_mixture_tiled<DB>>(ctx, lds));
  ProfScope ps(ctx, "target_mixture");
  return tgt_launch_tiled<k_target_mixture_tiled<DB>>(a, lds, a.d, (int)a.t->s0, a.N, a.yt, (const float *)a.t->p0, (const float *)a.t->p1);
}

// d <= 64 only (two U and two G blocks in registers): the ELBO entry points refuse Float32 coupling flows beyond it first
int nf_launch_target_mixture_tiled(const TgtTiledArgs &a) {
  if (a.d > NF_MIXTURE_TILED_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_db<2>(a.d, [&](auto db) { return launch_mixture_tiled<db()>(a); });
}

template <class T>
static int launch_mixture_flat(const TgtFlatArgs &a) {
  const size_t most = (size_t)((MXF_SPB + MXF_RB) * (MXF_MAXD + 1) + MXF_SPB * (MXF_RB + 1)) * sizeof(T);
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_mixture<T>>(ctx, most));
  ProfScope ps(ctx, "target_mixture");
  return tgt_launch_flat<k_target_mixture<T>, T>(a, (size_t)((MXF_SPB + MXF_RB) * (a.d + 1) + MXF_SPB * (MXF_RB + 1)) * sizeof(T), a.d,
                                                 (int)a.t->s0, a.N, (const T *)a.y, (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_mixture(const TgtFlatArgs &a) {
  if (a.d > MXF_MAXD) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_mixture_flat<decltype(e)>(a); });
}
