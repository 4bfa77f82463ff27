// nf_bnn.hip -- the one-hidden-layer Bayesian neural-network targets (NF_TARGET_BNN_LOGIT .. NF_TARGET_BNN_NORMAL; gfx950):
//     y = [w_0; ...; w_{H-1}; v; c] in R^d, d = H (p + 1) + 1 (hidden-unit-major: w_k the p input weights of unit k, v the H output
//     weights, c the output bias),
//     a_{ik} = tanh(x_i . w_k),   f_i = c + sum_k v_k a_{ik},   u_i = scl_i f_i + off_i,
//     log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) - par[2] / 2 sum_k |w_k|^2 - par[3] / 2 (|v|^2 + c^2),
//     g_i = wt_i phi'(u_i; par[0]) scl_i,   d/dc = sum_i g_i - par[3] c,   d/dv_k = sum_i g_i a_{ik} - par[3] v_k,
//     d/dw_k = sum_i g_i v_k (1 - a_{ik}^2) x_i - par[2] w_k
// with X [rows x p] row-major, the row data in ONE buffer p0 = scl[rows] | off[rows] | wt[rows] | par[4] (BnRows below) and phi one
// of the five row functions of nf_linpred.h.  The hidden layer is nf_softmax.hip's first GEMM with "class" read as "hidden unit";
// what is new is that v and c -- coordinates of y -- enter as per-sample scalars whose gradients are reductions over the data
// rows, not GEMM outputs.  Two kernels, the counterparts of nf_softmax.hip's:
//   k_target_bnn_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32
//   k_target_bnn        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// A row of weight 0 contributes exactly 0 to the value and to every gradient by SELECT, at every place its values enter a sum
// (phi, g_i, the g a products of d/dv, the second GEMM's operand): a subsampling mask may sit over a row of huge features or one
// whose phi overflows.  Nothing is clamped.
// Shared stages (nf_target_stages.h): tgt_stage_rows and tgt_gemm1_at (the wave's image of a row block; U_k from it and the tile at
// feature k p), tgt_elbo_term and tgt_block_partial (the ELBO tail of both kernels), and the launch helpers; what stands here in
// place does so for nf_ordinal.hip's reason.
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define BN_BLOCK 256
#define BN_WAVES 4
#define BN_MAXD 256
#define BN_MAXH 16
#define BN_MAXP 128

// The row data, addressed inside the one buffer p0 = scl[rows] | off[rows] | wt[rows] | par[4]: par[0] the family parameter,
// par[1] the additive constant the host folded, par[2] / par[3] the prior precisions of the hidden weights and of [v; c].
template <class T>
struct BnRows {
  const T *scl, *off, *wt, *par;
  __device__ __forceinline__ BnRows(const T *p0, int rows) : scl(p0), off(p0 + rows), wt(p0 + 2 * (long)rows), par(p0 + 3 * (long)rows) {}
};

// tanh and its derivative 1 - tanh^2 from ONE exponential e = exp(-2 |x|) in (0, 1]:
//     tanh = sign(x) (1 - e) / (1 + e),   1 - tanh^2 = 4 e / (1 + e)^2
// The derivative is a product -- no 1 - a^2 cancellation.  tanh is exactly +-1 once e is below half an ulp of 1 (|x| beyond 8.4)
// and the derivative exactly 0 once e underflows (|x| beyond 44 to 52, by whether the exponential keeps denormals): no finite
// (or infinite) x gives a non-finite result.  Absolute error of tanh about 1e-7 (the rounding of e next
// to 1), of the size of float32's own at |tanh| near 1.
__device__ __forceinline__ void bnn_tanh(float x, float &a, float &da) {
  const float e = nf_exp(-2.f * fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  a = copysignf((1.f - e) * r, x);
  da = 4.f * e * r * r;
}
// flat kernel: the library's tanh in either element type; (1 - a)(1 + a) is in [0, 1] for every a in [-1, 1]
__device__ __forceinline__ void bnn_tanh_lib(float x, float &a, float &da) {
  a = tanhf(x);
  da = (1.f - a) * (1.f + a);
}
__device__ __forceinline__ void bnn_tanh_lib(double x, double &a, double &da) {
  a = tanh(x);
  da = (1.0 - a) * (1.0 + a);
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The tile sits
// uncentred in LDS, [feature][sample], features >= d and padding samples zero, with eight zero feature rows behind the
// 32 DB (a unit's k-loop runs up to 7 features past its own).  Each wave takes the row blocks rb = wave, wave + 4, ... of X
// (32 rows each) and stages its block ONCE into an image of its own, 32 rows x p features (p <= 128: one chunk; the row
// stride S = 32 ceil(p / 32) + 1 is odd, so GEMM 1 -- lanes along rows -- and GEMM 2 -- lanes along features -- are both free of
// bank conflicts):
//   GEMM 1   U_k[i][j] = sum_f X[i][f] Y[k p + f][j]   the A operand is the same image for every unit, the B operand pointer
//                                                      advances by 32 p floats per unit.  k-steps pair features: with p odd
//                                                      the partner of a unit's last feature belongs to the next unit (or is
//                                                      v_0) and meets the image's zero column p
//   the middle, in the accumulator registers: register r of a lane of half `hi` is row nf_row(r, hi) of sample l & 31.  TWO
//            passes over the units, GEMM 1 recomputed in the second, so the register count does not grow with H:
//            pass 1  a = tanh(U_k), f += v_k a (v_k of the lane's sample from the tile, feature H p + k); after the last unit
//                    phi, phi', g of the 16 rows, added to the lane's log-p sum and sum of g
//            pass 2  a again; g a into the lane's d/dv_k partial; g v_k (1 - a^2) over the accumulator, which IS
//   GEMM 2   G[k p + f][j] += sum_i X[i][f] (g v_k (1 - a^2))[i][j]   's B operand (the register chaining of nf_mfma.h).  The
//                                                      output blocks are the global 32-feature blocks of y: a block takes
//                                                      one MFMA set per unit it overlaps, lanes outside the unit zero
// Rows >= rows read wt = 0, which masks them.  The four waves' G, d/dv, d/dc and log-p sums are combined through LDS in wave
// order (the two lane halves first, by one shuffle: a + b gives the same bits in both): no atomics, the same bits every launch.
// Up to DB = 2 the kernel is held to 256 registers (two workgroups per CU: one's tanh runs under the other's matrix
// instructions).  At DB = 4 that bound costs 12 to 132 bytes of scratch, whichever the row function (the 64 gradient accumulators,
// the 16 d/dv partials and three register sets of the middle do not fit 256), so DB = 4 keeps one workgroup per CU like DB = 8,
// which carries 128 gradient accumulators and the whole register file.
template <int DB>
struct BnGeo {
  static constexpr int YT = 32 * DB * 32;  // the tile; reused for the reduction of the gradient over the four waves
  static constexpr int YTP = YT + 8 * 32;  // with the eight zero feature rows behind it
  static constexpr int PMAX = 32 * DB < BN_MAXP ? 32 * DB : BN_MAXP;  // p <= d - 2
  __host__ __device__ static constexpr int stride(int p) { return 32 * ((p + 31) >> 5) + 1; }
  __host__ __device__ static constexpr int floats(int p) { return YTP + BN_WAVES * 32 * stride(p) + BN_WAVES * 64; }
};

template <class PHI, int DB>
__global__ __launch_bounds__(BN_BLOCK, DB <= 2 ? 2 : 1) void k_target_bnn_tiled(int d, int H, int rows, long N, const float *__restrict__ yt,
                                                                               const float *__restrict__ p0, const float *__restrict__ X,
                                                                               const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                               float *__restrict__ gt, float gscale, float *__restrict__ elbos_out,
                                                                               double *__restrict__ partial, double pscale) {
  using G = BnGeo<DB>;
  const BnRows<float> rd(p0, rows);
  const float par0 = rd.par[0];
  const int p = (d - 1) / H - 1, HP = H * p;
  const int S = G::stride(p);
  extern __shared__ float bn_lds[];
  float *sY = bn_lds;
  float *sA = bn_lds + G::YTP;
  float *sL = sA + BN_WAVES * 32 * S;  // [wave][lane] log-p partial sums
  __shared__ float red[2][BN_BLOCK / 32][32];
  __shared__ double sm[BN_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YTP / BN_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * BN_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * BN_BLOCK] = yv[k];
  }
  __syncthreads();

  float *img = sA + wave * 32 * S;
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float dv[BN_MAXH];  // the lane's d/dv_k partials (static indices only)
#pragma unroll
  for (int k = 0; k < BN_MAXH; ++k) dv[k] = 0.f;
  float lp = 0.f, sg = 0.f;
  const float cj = sY[(d - 1) * 32 + l31];  // the output bias of the lane's sample
  const int nrb = (rows + 31) >> 5;
  for (int rb = wave; rb < nrb; rb += BN_WAVES) {
    const int i0 = rb * 32;
    float scl[16], off[16], wt[16];  // (requested before the staging loads: in by the time the image is)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + nf_row(r, hi);
      scl[r] = i < rows ? rd.scl[i] : 0.f;
      off[r] = i < rows ? rd.off[i] : 0.f;
      wt[r] = i < rows ? rd.wt[i] : 0.f;
    }
    tgt_stage_rows(img, S, X, i0, rows, p, lane);
    wave_lds_fence();

    // pass 1: the network's output f, then phi, phi' and g of the lane's 16 rows
    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) g[r] = cj;  // (f until the row function has been evaluated)
    for (int k = 0; k < H; ++k) {
      const f32x16 U = tgt_gemm1_at(img, S, sY, k * p, p, l31, hi);
      const float vk = sY[(HP + k) * 32 + l31];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float a, da;
        bnn_tanh(U[r], a, da);
        g[r] = fmaf(vk, a, g[r]);
      }
    }
    unsigned dead = 0;  // bit r: row r has weight 0
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float ph, dp;
      PHI::eval(fmaf(scl[r], g[r], off[r]), par0, ph, dp);
      const bool live = wt[r] != 0.f;
      lp += live ? wt[r] * ph : 0.f;
      g[r] = live ? wt[r] * dp * scl[r] : 0.f;
      sg += g[r];
      dead |= live ? 0u : 1u << r;
    }

    // pass 2: d/dv_k in the lane, g v_k (1 - a^2) in GEMM 1's accumulator registers, straight into GEMM 2
    for (int k = 0; k < H; ++k) {
      f32x16 U = tgt_gemm1_at(img, S, sY, k * p, p, l31, hi);
      const float vk = sY[(HP + k) * 32 + l31];
      float part = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float a, da;
        bnn_tanh(U[r], a, da);
        const bool dr = (dead >> r) & 1u;
        part += dr ? 0.f : g[r] * a;
        U[r] = dr ? 0.f : g[r] * vk * da;
      }
#pragma unroll
      for (int kk = 0; kk < BN_MAXH; ++kk) dv[kk] += kk == k ? part : 0.f;
      const int f_lo = k * p, f_hi = f_lo + p;  // the unit's features
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        if (b * 32 < f_hi && b * 32 + 32 > f_lo) {  // (wave-uniform) block b overlaps the unit
          const int col = b * 32 + l31 - f_lo;
          const bool in = col >= 0 && col < p;
          const float *pa = img + (4 * hi) * S + (in ? col : 0);
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const float a = pa[((t & 3) + 8 * (t >> 2)) * S];
            Gacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? a : 0.f, U[t], Gacc[b], 0, 0, 0);
          }
        }
      }
    }
    wave_lds_fence();  // the next staging overwrites the image
  }

  // the four waves' gradients and log-p sums, combined in wave order: G into the feature rows < H p of the tile, the d/dv and
  // d/dc partials (the two lane halves first) into the rows H p .. d - 1
  sL[wave * 64 + lane] = lp;
  for (int w = 0; w < BN_WAVES; ++w) {
    __syncthreads();  // (first pass: every wave is done reading the tile)
    if (wave == w) {
#pragma unroll
      for (int b = 0; b < DB; ++b)
        if (b * 32 < HP) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int f = b * 32 + nf_row(r, hi);
            float *q = sY + f * 32 + l31;
            if (f < HP) *q = w == 0 ? Gacc[b][r] : *q + Gacc[b][r];
          }
        }
#pragma unroll
      for (int k = 0; k < BN_MAXH; ++k) {
        if (k < H) {
          const float t = dv[k] + __shfl_xor(dv[k], 32);
          float *q = sY + (HP + k) * 32 + l31;
          if (hi == 0) *q = w == 0 ? t : *q + t;
        }
      }
      const float t = sg + __shfl_xor(sg, 32);
      float *q = sY + (d - 1) * 32 + l31;
      if (hi == 0) *q = w == 0 ? t : *q + t;
    }
  }
  __syncthreads();

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s; the hidden weights
  // (features < H p) under par[2], [v; c] under par[3]
  const float pwh = rd.par[2], pwo = rd.par[3];
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yyh = 0.f, yyo = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (BN_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (BN_BLOCK / 32);
      const bool hid = i < HP;
      yyh += hid ? yv[k] * yv[k] : 0.f;
      yyo += hid ? 0.f : yv[k] * yv[k];
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] - (hid ? pwh : pwo) * yv[k]) : 0.f;
    }
  }
  red[0][q][s] = yyh;
  red[1][q][s] = yyo;
  __syncthreads();
  double contrib = 0.0;
  if (q == 0 && valid) {
    float th = 0.f, to = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < BN_BLOCK / 32; ++k) {
      th += red[0][k][s];
      to += red[1][k][s];
    }
#pragma unroll
    for (int w = 0; w < BN_WAVES; ++w) l += sL[w * 64 + s] + sL[w * 64 + 32 + s];
    float e = rd.par[1] + l - 0.5f * pwh * th - 0.5f * pwo * to;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// flat kernel (vector pipe)
// ---------------------------------------------------------------------------------------------------------------------
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  X passes through LDS in
// blocks of 16 rows: lane q of a sample takes row q -- its H <= 16 activations in registers, f, phi, g, its share of d/dv and
// d/dc --, the values g v_k (1 - a^2) go through LDS as [sample][row][unit], and lane q then owns the features q, q + 16, ...
// of the hidden weights' gradient.  d/dv and d/dc are summed over the sample's 16 lanes at the end.  The library's own
// tanh / exp / log in either element type.
#define BNF_LANES 16
#define BNF_SPB (BN_BLOCK / BNF_LANES)
#define BNF_RB 16

template <class PHI, class T>
__global__ __launch_bounds__(BN_BLOCK) void k_target_bnn(int d, int H, int rows, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                         const T *__restrict__ X, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                         T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                         T *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  const BnRows<T> rd(p0, rows);
  const T par0 = rd.par[0], pwh = rd.par[2], pwo = rd.par[3];
  const int p = (d - 1) / H - 1, HP = H * p;
  extern __shared__ double bnf_lds[];
  const int S = d + 1, SP = p + 1, SD = BNF_RB * H + 1;
  T *sY = (T *)bnf_lds;            // [sample][d + 1]
  T *sA = sY + BNF_SPB * S;        // [row][p + 1]
  T *sD = sA + BNF_RB * SP;        // [sample][row][unit] g v_k (1 - a^2) (sample stride 16 H + 1)
  __shared__ double sm[BN_BLOCK / 64];
  const int q = threadIdx.x & (BNF_LANES - 1), sl = threadIdx.x / BNF_LANES;
  const long j = (long)blockIdx.x * BNF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < BNF_SPB * d; idx += BN_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * BNF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  T g[BN_MAXD / BNF_LANES];
  int gx[BN_MAXD / BNF_LANES], gk[BN_MAXD / BNF_LANES];  // feature q + 16 k: its column of X and its unit
#pragma unroll
  for (int k = 0; k < BN_MAXD / BNF_LANES; ++k) {
    g[k] = (T)0;
    const int f = k * BNF_LANES + q, u = f / p;
    gk[k] = u;
    gx[k] = f - u * p;
  }
  T dv[BN_MAXH];  // the lane's share of d/dv_k (static indices only)
#pragma unroll
  for (int k = 0; k < BN_MAXH; ++k) dv[k] = (T)0;
  T lp = 0, sg = 0;
  for (int i0 = 0; i0 < rows; i0 += BNF_RB) {
    const bool live = i0 + q < rows;
    const T sc = live ? rd.scl[i0 + q] : (T)0, of = live ? rd.off[i0 + q] : (T)0, wv = live ? rd.wt[i0 + q] : (T)0;  // (requested with the block of X)
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < BNF_RB * p; idx += BN_BLOCK) {
      const int row = idx / p, f = idx - row * p;
      sA[row * SP + f] = i0 + row < rows ? X[(long)(i0 + row) * p + f] : (T)0;
    }
    __syncthreads();
    const T *py = sY + sl * S;
    T a[BN_MAXH], da[BN_MAXH];
    T fo = py[d - 1];
#pragma unroll
    for (int k = 0; k < BN_MAXH; ++k) {
      if (k < H) {
        T u = 0;
        const T *pw = py + k * p;
        for (int f = 0; f < p; ++f) u += sA[q * SP + f] * pw[f];
        bnn_tanh_lib(u, a[k], da[k]);
        fo += py[HP + k] * a[k];
      } else
        a[k] = da[k] = (T)0;
    }
    T ph, dp;
    PHI::eval(sc * fo + of, par0, ph, dp);
    const bool on = wv != (T)0;
    lp += on ? wv * ph : (T)0;
    const T gi = on ? wv * dp * sc : (T)0;
    sg += gi;
#pragma unroll
    for (int k = 0; k < BN_MAXH; ++k) {
      if (k < H) {
        dv[k] += on ? gi * a[k] : (T)0;
        sD[sl * SD + q * H + k] = on ? gi * py[HP + k] * da[k] : (T)0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BN_MAXD / BNF_LANES; ++k) {
      const int f = k * BNF_LANES + q;
      if (f < HP) {
        T acc = g[k];
        const T *pd = sD + sl * SD + gk[k];
        const T *px = sA + gx[k];
#pragma unroll
        for (int r = 0; r < BNF_RB; ++r) acc += px[r * SP] * pd[r * H];
        g[k] = acc;
      }
    }
  }
  lp = group16_sum(lp);
  sg = group16_sum(sg);
#pragma unroll
  for (int k = 0; k < BN_MAXH; ++k)
    if (k < H) dv[k] = group16_sum(dv[k]);
  T yyh = 0, yyo = 0;
#pragma unroll
  for (int k = 0; k < BN_MAXD / BNF_LANES; ++k) {
    const int f = k * BNF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f];
      T gv = g[k], pw = pwh;
      if (f < HP)
        yyh += yv * yv;
      else {
        yyo += yv * yv;
        pw = pwo;
        gv = sg;  // f == d - 1: the output bias
#pragma unroll
        for (int u = 0; u < BN_MAXH; ++u) gv = (u < H && f - HP == u) ? dv[u] : gv;
      }
      if (grad_out) grad_out[j * d + f] = gscale * (gv - pw * yv);
    }
  }
  yyh = group16_sum(yyh);
  yyo = group16_sum(yyo);
  double contrib = 0.0;
  if (valid && q == 0) {
    T e = rd.par[1] + lp - (T)0.5 * pwh * yyh - (T)0.5 * pwo * yyo;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = rows, s1 = H, (d - 1) % H == 0)
// ---------------------------------------------------------------------------------------------------------------------
// what no kernel here serves: the tile and the flat kernel's registers stop at d = 256, the one-chunk image at p = 128
static inline bool bnn_unsupported(const nf_target *t, int d) { return d > BN_MAXD || (d - 1) / (int)t->s1 - 1 > BN_MAXP; }

// f(PHI()) for the row function of the kind
template <class F>
static int bnn_dispatch_phi(int kind, F &&f) {
  switch (kind) {
    case NF_TARGET_BNN_LOGIT: return f(PhiLogSigmoid());
    case NF_TARGET_BNN_PROBIT: return f(PhiLogNormCdf());
    case NF_TARGET_BNN_POISSON: return f(PhiNegExp());
    case NF_TARGET_BNN_STUDENT: return f(PhiStudent());
    default: return f(PhiHalfSquare());
  }
}

template <class PHI, int DB>
static int launch_bnn_tiled(const TgtTiledArgs &a) {
  using G = BnGeo<DB>;
  const int H = (int)a.t->s1, p = (a.d - 1) / H - 1;
  nf_ctx *ctx = a.ctx;
  NF_TRY((nf_lds_once<k_target_bnn_tiled<PHI, DB>>(ctx, G::floats(G::PMAX) * sizeof(float))));
  ProfScope ps(ctx, "target_bnn");
  return tgt_launch_tiled<k_target_bnn_tiled<PHI, DB>>(a, (size_t)G::floats(p) * sizeof(float), a.d, H, (int)a.t->s0, a.N, a.yt,
                                                       (const float *)a.t->p0, (const float *)a.t->p1);
}

int nf_launch_target_bnn_tiled(const TgtTiledArgs &a) {
  if (bnn_unsupported(a.t, a.d)) return NF_ERR_UNSUPPORTED;
  return bnn_dispatch_phi(a.t->kind, [&](auto phi) {
    return tgt_dispatch_db(a.d, [&](auto db) { return launch_bnn_tiled<decltype(phi), db()>(a); });
  });
}

// elements of LDS the flat kernel takes at (d, H)
static size_t bnn_flat_lds(int d, int H) { return (size_t)(BNF_SPB * (d + 1) + BNF_RB * ((d - 1) / H) + BNF_SPB * (BNF_RB * H + 1)); }

template <class PHI, class T>
static int launch_bnn_flat(const TgtFlatArgs &a) {
  const int H = (int)a.t->s1;
  // the most any served target takes: d = 256, with the widest image (p = 128) and the widest [row][unit] block (H = 16) both counted
  const size_t most = (size_t)(BNF_SPB * (BN_MAXD + 1) + BNF_RB * (BN_MAXP + 1) + BNF_SPB * (BNF_RB * BN_MAXH + 1)) * sizeof(T);
  nf_ctx *ctx = a.ctx;
  NF_TRY((nf_lds_once<k_target_bnn<PHI, T>>(ctx, most)));
  ProfScope ps(ctx, "target_bnn");
  return tgt_launch_flat<k_target_bnn<PHI, T>, T>(a, bnn_flat_lds(a.d, H) * sizeof(T), a.d, H, (int)a.t->s0, a.N, (const T *)a.y,
                                                  (const T *)a.t->p0, (const T *)a.t->p1);
}

int nf_launch_target_bnn(const TgtFlatArgs &a) {
  if (bnn_unsupported(a.t, a.d)) return NF_ERR_UNSUPPORTED;
  return bnn_dispatch_phi(a.t->kind, [&](auto phi) {
    return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_bnn_flat<decltype(phi), decltype(e)>(a); });
  });
}
