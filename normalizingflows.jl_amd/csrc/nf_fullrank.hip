// nf_fullrank.hip -- NF_KIND_FULLRANK: y = mu + L x with L lower triangular (Shift o Scale(LowerTriangular), the
// full-rank Gaussian family of ADVI; gfx950).  theta = [mu(d) ; L as a d x d column-major matrix]; the strict upper
// triangle belongs to theta (the parent matrix of LowerTriangular) and is NEVER read: every load of L is guarded by a
// select on (column <= row), so whatever it holds -- NaN included -- no output changes a bit, and its gradient is 0.0.
//
// Float32 (matrix pipe, v_mfma_f32_32x32x2_f32 through the builtin):
//   k_fr_gemm   one workgroup of four waves per 32-sample tile.  The tile sits in LDS [feature][sample] (row stride 33,
//               features padded to whole 32-blocks with zeros); wave w takes the output blocks fb = w, w + 4, ... and
//               contracts ONLY the blocks kb <= fb (kb >= fb for the transposed walk), each staged into the wave's own
//               33-stride LDS image (the next block's loads in flight meanwhile), the diagonal block masked while staging; the
//               results leave straight from the accumulator registers.  Three uses: forward (M = L, then + mu),
//               pullback of the cotangent (M = L', the upper-triangular walk of the same blocks) and inverse (M = inv(L)
//               from k_fr_tri_inverse, on the tile with mu subtracted while it is staged).  Reads and writes either
//               batch layout (standard d x N column-major, or the tiled one of nf_elementwise.hip).
//   k_fr_bwd    grid-stride over tiles; x and ybar tiles in LDS, gL[fb][kb] += sum_samples ybar x' for kb <= fb only, 16
//               MFMAs per block and tile, the accumulators in registers across the workgroup's tiles, the lower blocks
//               dealt round-robin to the four waves (36 blocks at d = 256: nine per wave).  g_mu from the same tile.  No
//               atomics: one slab per workgroup (theta's layout), reduced in block order by nf_launch_reduce_slabs.  The
//               log-det term (sum_j lbar_j) / L_ii enters once per workgroup, when the slab is written.
//   k_fr_bwd_x  k_fr_bwd on tiled x and ybar that ALSO leaves xbar = L' ybar from the ybar tile it has staged (k_fr_gemm's
//               transposed walk, a matrix-block image per wave behind the two tiles): the whole reverse pass of the layer in one
//               launch, for flows that continue the reverse pass below it (NF_KIND_PRECOND).  Same arithmetic, same order as
//               k_fr_bwd followed by k_fr_gemm(trans): the same bits.
//   k_fr_tri_inverse   inv(L) once per call: one workgroup, thread c runs forward substitution on column c of the identity.
// The log-det sum_i log|L_ii| is a function of theta alone: computed once per workgroup, written per sample.
// The shift is added AFTER the product (not as the initial accumulator): the whole map and Shift applied to Scale's
// output then agree bit for bit.
//
// Float64 (vector pipe, standard layout): one thread per sample for the forward, the forward substitution and the
// cotangent pullback (k_fr_apply_flat); the parameter gradient is one thread per parameter and sample chunk
// (k_fr_grad_flat), the chunks' slabs reduced in order like the Float32 ones.
#include "nf_common.h"
#include "nf_launchers.h"
#include "nf_mfma.h"

#define FR_BLOCK 256
#define FR_WAVES 4
#define FR_MAXD 256
#define FR_XS 33  // row stride of a tile in LDS: odd, so lanes along samples AND lanes along features are conflict-free
#define FR_IS 33  // row stride of a wave's matrix-block image

template <int DB>
struct FrGeo {
  static constexpr int ROWS = 32 * DB;
  static constexpr int TILE = ROWS * FR_XS;
  static constexpr int IMG = 32 * FR_IS;
  static constexpr int PER = ROWS * 32 / FR_BLOCK;  // tile elements per thread
};

// position p of a tile sweep -> (feature, sample) and the element's offset from the tile's base (tile * d * 32 in both
// layouts): tiled = [feature][32 samples], standard = [sample][d].  Consecutive threads touch consecutive addresses.
template <int DB>
__device__ __forceinline__ void fr_pos(int p, bool tiled, int d, int &f, int &s, int &off) {
  if (tiled) {
    f = p >> 5, s = p & 31, off = p;
  } else {
    s = p / FrGeo<DB>::ROWS, f = p % FrGeo<DB>::ROWS, off = s * d + f;
  }
}

// global tile -> LDS [feature][sample], zero beyond d and N; sub (optional) is subtracted per feature
template <int DB>
__device__ __forceinline__ void fr_load_tile(float *__restrict__ sT, const float *__restrict__ src, bool tiled, int d, long N,
                                             long tile, const float *__restrict__ sub) {
  using G = FrGeo<DB>;
  const float *base = src + tile * d * 32;
  // eight elements per thread in flight: all of a group's loads before its first LDS store.  The group loop stays rolled,
  // so that the positions are not kept in registers across a caller's tile loop.
  constexpr int CH = G::PER < 8 ? G::PER : 8;
#pragma unroll 1
  for (int k0 = 0; k0 < G::PER; k0 += CH) {
    float v[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      int f, s, off;
      fr_pos<DB>(threadIdx.x + (k0 + k) * FR_BLOCK, tiled, d, f, s, off);
      const bool ok = f < d && tile * 32 + s < N;
      v[k] = ok ? base[off] - (sub ? sub[f] : 0.f) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      int f, s, off;
      fr_pos<DB>(threadIdx.x + (k0 + k) * FR_BLOCK, tiled, d, f, s, off);
      sT[f * FR_XS + s] = v[k];
    }
  }
}

// Block (fb, kb) of M -> the wave's image img[row][col] in two halves, global -> registers and registers -> LDS, so that the next
// block's loads are in flight while the current one is multiplied.  By select: zero beyond d and on the masked side of the
// diagonal.  trans == 0: M[r][c] = L[r + c d] for c <= r (lanes along rows, the contiguous direction of a column-major
// matrix); trans != 0: M[r][c] = L[c + r d] for c >= r (lanes along columns).
__device__ __forceinline__ void fr_stage_load(float (&v)[16], const float *__restrict__ L, int d, int fb, int kb, int trans, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  if (!trans) {
    const int r = fb * 32 + l31;
#pragma unroll
    for (int cp = 0; cp < 16; ++cp) {
      const int c = kb * 32 + 2 * cp + hi;
      v[cp] = (r < d && c <= r) ? L[r + (long)c * d] : 0.f;
    }
  } else {
    const int c = kb * 32 + l31;
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) {
      const int r = fb * 32 + 2 * rp + hi;
      v[rp] = (c < d && c >= r) ? L[c + (long)r * d] : 0.f;
    }
  }
}
__device__ __forceinline__ void fr_stage_store(float *__restrict__ img, const float (&v)[16], int trans, int lane) {
  const int l31 = lane & 31, hi = lane >> 5;
  if (!trans) {
#pragma unroll
    for (int cp = 0; cp < 16; ++cp) img[l31 * FR_IS + 2 * cp + hi] = v[cp];
  } else {
#pragma unroll
    for (int rp = 0; rp < 16; ++rp) img[(2 * rp + hi) * FR_IS + l31] = v[rp];
  }
}

// out = M (in - sub) + add per 32-sample tile, M the triangular matrix behind Lm (see fr_stage).  ladj (optional) receives
// lsign * sum_i log|Ld_ii| for every sample of the tile.  out may alias in (a workgroup reads its whole tile first).
template <int DB>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_gemm(int d, long N, const float *__restrict__ Lm, int trans,
                                                      const float *__restrict__ sub, const float *__restrict__ add,
                                                      const float *__restrict__ Ld, float lsign, const float *in, int in_tiled,
                                                      float *out, int out_tiled, float *__restrict__ ladj) {
  using G = FrGeo<DB>;
  extern __shared__ float fr_sm[];
  float *sX = fr_sm;
  float *sA = sX + G::TILE;
  __shared__ double sm[FR_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  fr_load_tile<DB>(sX, in, in_tiled != 0, d, N, tile, sub);
  __syncthreads();  // every read of the tile from global memory is done: from here on out may be written (out may alias in)

  float *img = sA + wave * G::IMG;
  float *obase = out + tile * d * 32;
  const bool valid = tile * 32 + l31 < N;
  const int nblk = (d + 31) >> 5;
  for (int fb = wave; fb < nblk; fb += FR_WAVES) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int k0 = trans ? fb : 0, k1 = trans ? nblk - 1 : fb;
    float v[16];
    fr_stage_load(v, Lm, d, fb, k0, trans, lane);
    for (int kb = k0; kb <= k1; ++kb) {
      fr_stage_store(img, v, trans, lane);
      wave_lds_fence();
      if (kb < k1) fr_stage_load(v, Lm, d, fb, kb + 1, trans, lane);  // in flight during this block's products
      const int nf = d - kb * 32 < 32 ? d - kb * 32 : 32;
      const int ng = (nf + 7) >> 3;  // groups of four k-steps = eight features; features >= d are zero on both sides
      const float *pa = img + l31 * FR_IS + hi;
      const float *pb = sX + (kb * 32 + hi) * FR_XS + l31;
      for (int g = 0; g < ng; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[8 * g + 2 * e], pb[(8 * g + 2 * e) * FR_XS], acc, 0, 0, 0);
      }
      wave_lds_fence();  // the next staging overwrites the image
    }
    // straight from the accumulator registers: register r of a lane of half `hi` is feature nf_row(r, hi) of sample l & 31.
    // Tiled output: 128-byte runs along the samples (padding samples written as zeros); standard layout: a stride of d.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = fb * 32 + nf_row(r, hi);
      if (f < d) {
        const float y = add ? acc[r] + add[f] : acc[r];
        if (out_tiled)
          obase[f * 32 + l31] = valid ? y : 0.f;
        else if (valid)
          obase[l31 * d + f] = y;
      }
    }
  }
  if (ladj) {  // (uniform)
    const int i = threadIdx.x;
    const double c = block_sum<FR_WAVES, false>(i < d ? (double)logf(fabsf(Ld[i + (long)i * d])) : 0.0, sm);
    __shared__ float sc;
    if (threadIdx.x == 0) sc = lsign * (float)c;
    __syncthreads();
    if (threadIdx.x < 32 && tile * 32 + threadIdx.x < N) ladj[tile * 32 + threadIdx.x] = sc;
  }
}

// lower block number b = fb (fb + 1) / 2 + kb -> (fb, kb)
__device__ __forceinline__ void fr_block_of(int b, int &fb, int &kb) {
  fb = 0;
  while ((fb + 1) * (fb + 2) / 2 <= b) ++fb;
  kb = b - fb * (fb + 1) / 2;
}

// slab[blockIdx.x] = this workgroup's share of [g_mu ; g_L] (theta's layout, zeros above the diagonal):
//   g_mu[f] = sum_j ybar[f][j],   g_L[f][k] = sum_j ybar[f][j] x[k][j]  (k <= f)  +  [f == k] (sum_j lbar_j) / L_ff
// The accumulator of block (fb, kb) is held TRANSPOSED (rows k, lanes along f), so that the slab write runs along the
// contiguous direction of the column-major matrix.
template <int DB>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_bwd(int d, long N, long ntiles, const float *__restrict__ L,
                                                     const float *__restrict__ x, int x_tiled, const float *__restrict__ ybar,
                                                     int y_tiled, const float *__restrict__ lbar, float lbar_const,
                                                     float *__restrict__ slabs) {
  using G = FrGeo<DB>;
  constexpr int NBLK = DB * (DB + 1) / 2, MB = (NBLK + FR_WAVES - 1) / FR_WAVES;
  extern __shared__ float fr_sm[];
  float *sX = fr_sm;
  float *sG = sX + G::TILE;
  __shared__ float sls;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  f32x16 acc[MB];
  int fbs[MB], kbs[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    fr_block_of(wave + FR_WAVES * i, fbs[i], kbs[i]);
  }
  float gmu = 0.f, ls = 0.f;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers
    fr_load_tile<DB>(sX, x, x_tiled != 0, d, N, tile, nullptr);
    fr_load_tile<DB>(sG, ybar, y_tiled != 0, d, N, tile, nullptr);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      if (wave + FR_WAVES * i < NBLK && fbs[i] * 32 < d) {  // (wave-uniform)
        const float *pa = sX + (kbs[i] * 32 + l31) * FR_XS + hi;
        const float *pb = sG + (fbs[i] * 32 + l31) * FR_XS + hi;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t], pb[2 * t], acc[i], 0, 0, 0);
      }
    }
    if ((int)threadIdx.x < d) {
      const float *pg = sG + threadIdx.x * FR_XS;
      float a = 0.f;
#pragma unroll
      for (int s = 0; s < 32; ++s) a += pg[s];
      gmu += a;
    }
    if (threadIdx.x < 32) {
      const long j = tile * 32 + threadIdx.x;
      ls += j < N ? (lbar ? lbar[j] : lbar_const) : 0.f;
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) ls += __shfl_xor(ls, o, 64);
    if (lane == 0) sls = ls;
  }
  __syncthreads();
  const long P = (long)d + (long)d * d;
  float *slab = slabs + (long)blockIdx.x * P;
  if ((int)threadIdx.x < d) slab[threadIdx.x] = gmu;
  // blocks above the diagonal: zeros (the lower blocks, the diagonal ones' upper halves included, are written below)
  for (int idx = threadIdx.x; idx < d * d; idx += FR_BLOCK) {
    const int k = idx / d, f = idx - k * d;
    if ((k >> 5) > (f >> 5)) slab[d + idx] = 0.f;
  }
  const float lsum = sls;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (wave + FR_WAVES * i < NBLK && fbs[i] * 32 < d) {
      const int f = fbs[i] * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = kbs[i] * 32 + nf_row(r, hi);
        if (f < d && k < d) {
          float v = 0.f;
          if (k < f) v = acc[i][r];
          if (k == f) v = acc[i][r] + lsum / L[f + (long)f * d];
          slab[d + f + (long)k * d] = v;
        }
      }
    }
  }
}

// k_fr_bwd on tiled x and ybar that also leaves the layer's input cotangent: from the same staged ybar tile xbar = L' ybar,
// k_fr_gemm's transposed block walk (the same staging, the same k order: the same bits as the two launches), written from the
// accumulator registers in the tiled layout.  xbar may alias ybar: a workgroup has its tile in LDS before it writes anything.
// The gradient part is k_fr_bwd's text, kept apart so that k_fr_bwd keeps its instruction stream.
template <int DB>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_bwd_x(int d, long N, long ntiles, const float *__restrict__ L,
                                                       const float *__restrict__ x, const float *ybar,
                                                       const float *__restrict__ lbar, float lbar_const,
                                                       float *__restrict__ slabs, float *xbar) {
  using G = FrGeo<DB>;
  constexpr int NBLK = DB * (DB + 1) / 2, MB = (NBLK + FR_WAVES - 1) / FR_WAVES;
  extern __shared__ float fr_sm[];
  float *sX = fr_sm;
  float *sG = sX + G::TILE;
  __shared__ float sls;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  f32x16 acc[MB];
  int fbs[MB], kbs[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    fr_block_of(wave + FR_WAVES * i, fbs[i], kbs[i]);
  }
  float gmu = 0.f, ls = 0.f;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers
    fr_load_tile<DB>(sX, x, true, d, N, tile, nullptr);
    fr_load_tile<DB>(sG, ybar, true, d, N, tile, nullptr);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      if (wave + FR_WAVES * i < NBLK && fbs[i] * 32 < d) {  // (wave-uniform)
        const float *pa = sX + (kbs[i] * 32 + l31) * FR_XS + hi;
        const float *pb = sG + (fbs[i] * 32 + l31) * FR_XS + hi;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t], pb[2 * t], acc[i], 0, 0, 0);
      }
    }
    if ((int)threadIdx.x < d) {
      const float *pg = sG + threadIdx.x * FR_XS;
      float a = 0.f;
#pragma unroll
      for (int s = 0; s < 32; ++s) a += pg[s];
      gmu += a;
    }
    if (threadIdx.x < 32) {
      const long j = tile * 32 + threadIdx.x;
      ls += j < N ? (lbar ? lbar[j] : lbar_const) : 0.f;
    }
    {  // xbar = L' ybar from the staged tile
      float *img = sG + G::TILE + wave * G::IMG;
      float *obase = xbar + tile * d * 32;
      const bool valid = tile * 32 + l31 < N;
      const int nblk = (d + 31) >> 5;
      for (int fb = wave; fb < nblk; fb += FR_WAVES) {
        f32x16 ax;
#pragma unroll
        for (int r = 0; r < 16; ++r) ax[r] = 0.f;
        float v[16];
        fr_stage_load(v, L, d, fb, fb, 1, lane);
        for (int kb = fb; kb < nblk; ++kb) {
          fr_stage_store(img, v, 1, lane);
          wave_lds_fence();
          if (kb < nblk - 1) fr_stage_load(v, L, d, fb, kb + 1, 1, lane);  // in flight during this block's products
          const int nf = d - kb * 32 < 32 ? d - kb * 32 : 32;
          const int ng = (nf + 7) >> 3;
          const float *pa = img + l31 * FR_IS + hi;
          const float *pb = sG + (kb * 32 + hi) * FR_XS + l31;
          for (int g = 0; g < ng; ++g) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              ax = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[8 * g + 2 * e], pb[(8 * g + 2 * e) * FR_XS], ax, 0, 0, 0);
          }
          wave_lds_fence();  // the next staging overwrites the image
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = fb * 32 + nf_row(r, hi);
          if (f < d) obase[f * 32 + l31] = valid ? ax[r] : 0.f;
        }
      }
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) ls += __shfl_xor(ls, o, 64);
    if (lane == 0) sls = ls;
  }
  __syncthreads();
  const long P = (long)d + (long)d * d;
  float *slab = slabs + (long)blockIdx.x * P;
  if ((int)threadIdx.x < d) slab[threadIdx.x] = gmu;
  // blocks above the diagonal: zeros (the lower blocks, the diagonal ones' upper halves included, are written below)
  for (int idx = threadIdx.x; idx < d * d; idx += FR_BLOCK) {
    const int k = idx / d, f = idx - k * d;
    if ((k >> 5) > (f >> 5)) slab[d + idx] = 0.f;
  }
  const float lsum = sls;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (wave + FR_WAVES * i < NBLK && fbs[i] * 32 < d) {
      const int f = fbs[i] * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = kbs[i] * 32 + nf_row(r, hi);
        if (f < d && k < d) {
          float v = 0.f;
          if (k < f) v = acc[i][r];
          if (k == f) v = acc[i][r] + lsum / L[f + (long)f * d];
          slab[d + f + (long)k * d] = v;
        }
      }
    }
  }
}

// W = inv(L), both lower triangular, d x d column-major: thread c solves L w = e_c by forward substitution
__global__ __launch_bounds__(FR_BLOCK) void k_fr_tri_inverse(int d, const float *__restrict__ L, float *W) {
  const int c = threadIdx.x;
  if (c >= d) return;
  float *w = W + (long)c * d;
  for (int i = c; i < d; ++i) {
    float a = i == c ? 1.f : 0.f;
    for (int k = c; k < i; ++k) a -= L[i + (long)k * d] * w[k];
    w[i] = a / L[i + (long)i * d];
  }
}

// the Shift layer alone: y = x + sign mu, log-det 0 (standard layout, either element type)
template <class T>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_shift(int d, long N, const T *__restrict__ mu, T sign, const T *x, T *y,
                                                       T *__restrict__ ladj) {
  const long idx = (long)blockIdx.x * FR_BLOCK + threadIdx.x;
  if (idx < N) ladj[idx] = (T)0;
  if (idx < N * d) y[idx] = x[idx] + sign * mu[idx % d];
}

// One thread per sample, standard layout.  mode 0: y = L x (+ mu); 1: x = inv(L) (y (- mu)) by forward substitution;
// 2: xbar = L' ybar.  Each walks its features in the order that lets out alias in.
template <class T>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_apply_flat(int d, long N, const T *__restrict__ mu, const T *__restrict__ L,
                                                            int mode, const T *in, T *out, T *__restrict__ ladj) {
  __shared__ double sm[FR_WAVES];
  __shared__ double sc;
  if (ladj) {  // (uniform)
    const int i = threadIdx.x;
    const double c = block_sum<FR_WAVES, false>(i < d ? (double)log(fabs(L[i + (long)i * d])) : 0.0, sm);
    if (threadIdx.x == 0) sc = mode == 1 ? -c : c;
    __syncthreads();
  }
  const long j = (long)blockIdx.x * FR_BLOCK + threadIdx.x;
  if (j >= N) return;
  const T *xi = in + j * d;
  T *yo = out + j * d;
  if (mode == 0) {
    for (int i = d - 1; i >= 0; --i) {
      T a = 0;
      for (int k = 0; k <= i; ++k) a += L[i + (long)k * d] * xi[k];
      yo[i] = mu ? a + mu[i] : a;
    }
  } else if (mode == 1) {
    for (int i = 0; i < d; ++i) {
      T a = mu ? xi[i] - mu[i] : xi[i];
      for (int k = 0; k < i; ++k) a -= L[i + (long)k * d] * yo[k];
      yo[i] = a / L[i + (long)i * d];
    }
  } else {
    for (int k = 0; k < d; ++k) {
      T a = 0;
      for (int i = k; i < d; ++i) a += L[i + (long)k * d] * xi[i];
      yo[k] = a;
    }
  }
  if (ladj) ladj[j] = (T)sc;
}

// slab[blockIdx.y][p]: parameter p's sum over the samples of chunk blockIdx.y (the terms of k_fr_bwd), standard layout
template <class T>
__global__ __launch_bounds__(FR_BLOCK) void k_fr_grad_flat(int d, long N, long chunk, const T *__restrict__ L,
                                                           const T *__restrict__ x, const T *__restrict__ ybar,
                                                           const T *__restrict__ lbar, T lbar_const, T *__restrict__ slabs) {
  const long P = (long)d + (long)d * d;
  const long p = (long)blockIdx.x * FR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const long j0 = (long)blockIdx.y * chunk, j1 = j0 + chunk < N ? j0 + chunk : N;
  T a = 0;
  if (p < d) {
    for (long j = j0; j < j1; ++j) a += ybar[j * d + p];
  } else {
    const int k = (int)((p - d) / d), i = (int)((p - d) - (long)k * d);
    if (k <= i) {
      for (long j = j0; j < j1; ++j) a += ybar[j * d + i] * x[j * d + k];
      if (k == i) {
        T ls = 0;
        for (long j = j0; j < j1; ++j) ls += lbar ? lbar[j] : lbar_const;
        a += ls / L[i + (long)i * d];
      }
    }
  }
  slabs[(long)blockIdx.y * P + p] = a;
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
bool nf_fr_supported(const nf_flow_desc *desc) { return desc->d >= 1 && desc->d <= FR_MAXD; }

static inline long fr_params(int d) { return (long)d + (long)d * d; }

template <int DB>
static int fr_gemm_db(nf_ctx *ctx, int d, long N, const float *Lm, int trans, const float *sub, const float *add, const float *Ld,
                      float lsign, const float *in, int in_tiled, float *out, int out_tiled, float *ladj) {
  const size_t lds = (size_t)(FrGeo<DB>::TILE + FR_WAVES * FrGeo<DB>::IMG) * sizeof(float);
  NF_TRY(nf_lds_once<&k_fr_gemm<DB>>(ctx, lds));
  ProfScope ps(ctx, "fr_gemm");
  hipLaunchKernelGGL(k_fr_gemm<DB>, dim3((unsigned)((N + 31) / 32)), dim3(FR_BLOCK), lds, ctx->stream, d, N, Lm, trans, sub, add, Ld,
                     lsign, in, in_tiled, out, out_tiled, ladj);
  return (int)hipGetLastError();
}
static int fr_gemm(nf_ctx *ctx, int d, long N, const float *Lm, int trans, const float *sub, const float *add, const float *Ld,
                   float lsign, const float *in, int in_tiled, float *out, int out_tiled, float *ladj) {
  if (d <= 32) return fr_gemm_db<1>(ctx, d, N, Lm, trans, sub, add, Ld, lsign, in, in_tiled, out, out_tiled, ladj);
  if (d <= 64) return fr_gemm_db<2>(ctx, d, N, Lm, trans, sub, add, Ld, lsign, in, in_tiled, out, out_tiled, ladj);
  if (d <= 128) return fr_gemm_db<4>(ctx, d, N, Lm, trans, sub, add, Ld, lsign, in, in_tiled, out, out_tiled, ladj);
  return fr_gemm_db<8>(ctx, d, N, Lm, trans, sub, add, Ld, lsign, in, in_tiled, out, out_tiled, ladj);
}

template <int DB>
static int fr_bwd_db(nf_ctx *ctx, int d, long N, int grid, const float *L, const float *x, int x_tiled, const float *ybar,
                     int y_tiled, const float *lbar, float lbar_const, float *slabs) {
  const size_t lds = (size_t)(2 * FrGeo<DB>::TILE) * sizeof(float);
  NF_TRY(nf_lds_once<&k_fr_bwd<DB>>(ctx, lds));
  ProfScope ps(ctx, "fr_bwd");
  hipLaunchKernelGGL(k_fr_bwd<DB>, dim3((unsigned)grid), dim3(FR_BLOCK), lds, ctx->stream, d, N, (N + 31) / 32, L, x, x_tiled, ybar,
                     y_tiled, lbar, lbar_const, slabs);
  return (int)hipGetLastError();
}

template <int DB>
static int fr_bwd_x_db(nf_ctx *ctx, int d, long N, int grid, const float *L, const float *x, const float *ybar, const float *lbar,
                       float lbar_const, float *slabs, float *xbar) {
  const size_t lds = (size_t)(2 * FrGeo<DB>::TILE + FR_WAVES * FrGeo<DB>::IMG) * sizeof(float);
  NF_TRY(nf_lds_once<&k_fr_bwd_x<DB>>(ctx, lds));
  ProfScope ps(ctx, "fr_bwd_x");
  hipLaunchKernelGGL(k_fr_bwd_x<DB>, dim3((unsigned)grid), dim3(FR_BLOCK), lds, ctx->stream, d, N, (N + 31) / 32, L, x, ybar, lbar,
                     lbar_const, slabs, xbar);
  return (int)hipGetLastError();
}

// workgroups (= gradient slabs) of the Float32 reverse kernel: one per compute unit at most, each walking its tiles
int nf_fr_bwd_grid(nf_ctx *ctx, long N) {
  const long nt = (N + 31) / 32;
  return (int)(nt < ctx->num_cu ? (nt < 1 ? 1 : nt) : ctx->num_cu);
}
// sample chunks (= gradient slabs) of the Float64 gradient kernel
static inline int fr_flat_slabs(long N) {
  const long n = (N + 63) / 64;
  return (int)(n < 1 ? 1 : n > 64 ? 64 : n);
}

// Float32 parameter gradient from x and ybar in either layout: slabs (nf_fr_bwd_grid(N) x P floats), then their sum
int nf_fr_grad(nf_ctx *ctx, const nf_flow_desc *desc, const float *theta, const float *x, int x_tiled, const float *ybar,
               int y_tiled, const float *lbar, float lbar_const, long N, float *slabs, float *gtheta_out) {
  const int d = desc->d, grid = nf_fr_bwd_grid(ctx, N);
  const float *L = theta + d;
  int st;
  if (d <= 32) st = fr_bwd_db<1>(ctx, d, N, grid, L, x, x_tiled, ybar, y_tiled, lbar, lbar_const, slabs);
  else if (d <= 64) st = fr_bwd_db<2>(ctx, d, N, grid, L, x, x_tiled, ybar, y_tiled, lbar, lbar_const, slabs);
  else if (d <= 128) st = fr_bwd_db<4>(ctx, d, N, grid, L, x, x_tiled, ybar, y_tiled, lbar, lbar_const, slabs);
  else st = fr_bwd_db<8>(ctx, d, N, grid, L, x, x_tiled, ybar, y_tiled, lbar, lbar_const, slabs);
  NF_TRY(st);
  return nf_launch_reduce_slabs(ctx, NF_DTYPE_F32, slabs, grid, fr_params(d), gtheta_out);
}

// The layer's whole reverse pass on tiled buffers in one launch: the parameter gradient as nf_fr_grad, and xbar = L' ybar
// (xbar may alias ybar)
int nf_fr_bwd_x_tiled(nf_ctx *ctx, const nf_flow_desc *desc, const float *theta, const float *xt, const float *ybar,
                      const float *lbar, float lbar_const, long N, float *slabs, float *gtheta_out, float *xbar) {
  const int d = desc->d, grid = nf_fr_bwd_grid(ctx, N);
  const float *L = theta + d;
  int st;
  if (d <= 32) st = fr_bwd_x_db<1>(ctx, d, N, grid, L, xt, ybar, lbar, lbar_const, slabs, xbar);
  else if (d <= 64) st = fr_bwd_x_db<2>(ctx, d, N, grid, L, xt, ybar, lbar, lbar_const, slabs, xbar);
  else if (d <= 128) st = fr_bwd_x_db<4>(ctx, d, N, grid, L, xt, ybar, lbar, lbar_const, slabs, xbar);
  else st = fr_bwd_x_db<8>(ctx, d, N, grid, L, xt, ybar, lbar, lbar_const, slabs, xbar);
  NF_TRY(st);
  return nf_launch_reduce_slabs(ctx, NF_DTYPE_F32, slabs, grid, fr_params(d), gtheta_out);
}
// xbar = L' ybar alone, tiled in and out (the second launch of the two-launch reverse pass; xbar may alias ybar)
int nf_fr_pull_tiled(nf_ctx *ctx, const nf_flow_desc *desc, const float *theta, const float *ybar, long N, float *xbar) {
  const int d = desc->d;
  return fr_gemm(ctx, d, N, theta + d, 1, nullptr, nullptr, nullptr, 0.f, ybar, 1, xbar, 1, nullptr);
}

// Float32 forward on tiled buffers (the ELBO sequence): yt = mu + L xt, ladj = sum log|L_ii|
int nf_fr_fwd_tiled(nf_ctx *ctx, const nf_flow_desc *desc, const float *theta, const float *xt, long N, float *yt, float *ladj) {
  const int d = desc->d;
  return fr_gemm(ctx, d, N, theta + d, 0, nullptr, theta, theta + d, 1.f, xt, 1, yt, 1, ladj);
}

// what nf_fr_apply needs at the front of the context workspace: inv(L) for a Float32 inverse that includes the Scale layer
size_t nf_fr_apply_ws_bytes(const nf_flow_desc *desc, bool inverse) {
  return (inverse && desc->dtype == NF_DTYPE_F32) ? carve_bytes((size_t)desc->d * desc->d * sizeof(float)) : 0;
}

// layers [lo, hi) of (0 = Shift, 1 = Scale) in the standard layout; y may alias x; ladj is overwritten
int nf_fr_apply(nf_ctx *ctx, const nf_flow_desc *desc, int lo, int hi, bool inverse, const void *theta, const void *x, long N,
                void *y, void *ladj) {
  const int d = desc->d;
  const bool shift = lo <= 0 && hi >= 1, scale = lo <= 1 && hi >= 2;
  if (N <= 0) return NF_OK;
  if (!scale) {
    const unsigned nb = (unsigned)(((long)N * d + FR_BLOCK - 1) / FR_BLOCK);
    if (desc->dtype == NF_DTYPE_F32)
      hipLaunchKernelGGL(k_fr_shift<float>, dim3(nb), dim3(FR_BLOCK), 0, ctx->stream, d, N, (const float *)theta, inverse ? -1.f : 1.f,
                         (const float *)x, (float *)y, (float *)ladj);
    else
      hipLaunchKernelGGL(k_fr_shift<double>, dim3(nb), dim3(FR_BLOCK), 0, ctx->stream, d, N, (const double *)theta, inverse ? -1.0 : 1.0,
                         (const double *)x, (double *)y, (double *)ladj);
    return (int)hipGetLastError();
  }
  if (desc->dtype == NF_DTYPE_F64) {
    const double *mu = (const double *)theta, *L = mu + d;
    ProfScope ps(ctx, "fr_apply_flat");
    hipLaunchKernelGGL(k_fr_apply_flat<double>, dim3((unsigned)((N + FR_BLOCK - 1) / FR_BLOCK)), dim3(FR_BLOCK), 0, ctx->stream, d, N,
                       shift ? mu : nullptr, L, inverse ? 1 : 0, (const double *)x, (double *)y, (double *)ladj);
    return (int)hipGetLastError();
  }
  const float *mu = (const float *)theta, *L = mu + d;
  if (!inverse) return fr_gemm(ctx, d, N, L, 0, nullptr, shift ? mu : nullptr, L, 1.f, (const float *)x, 0, (float *)y, 0, (float *)ladj);
  NF_TRY(nf_ws_reserve(ctx, nf_fr_apply_ws_bytes(desc, true)));
  float *W = (float *)ctx->ws;
  hipLaunchKernelGGL(k_fr_tri_inverse, dim3(1), dim3(FR_BLOCK), 0, ctx->stream, d, L, W);
  NF_HIP(hipGetLastError());
  return fr_gemm(ctx, d, N, W, 0, shift ? mu : nullptr, nullptr, L, -1.f, (const float *)x, 0, (float *)y, 0, (float *)ladj);
}

// the pullback's workspace: the gradient slabs
size_t nf_fr_bwd_ws_bytes(nf_ctx *ctx, const nf_flow_desc *desc, long N) {
  const long P = fr_params(desc->d);
  if (desc->dtype == NF_DTYPE_F32) return carve_bytes((size_t)nf_fr_bwd_grid(ctx, N) * P * sizeof(float));
  return carve_bytes((size_t)fr_flat_slabs(N) * P * sizeof(double));
}

// pullback in the standard layout from the flow input x: gtheta_out[P] (overwritten), and xbar_out = L' ybar unless NULL
// (xbar_out may alias ybar: the parameter gradient reads ybar first).  lbar == NULL: every sample's log-det cotangent is
// lbar_const.
int nf_fr_bwd(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *x, const void *ybar, const void *lbar,
              double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws) {
  const int d = desc->d;
  if (desc->dtype == NF_DTYPE_F32) {
    const float *L = (const float *)theta + d;
    NF_TRY(nf_fr_grad(ctx, desc, (const float *)theta, (const float *)x, 0, (const float *)ybar, 0, (const float *)lbar,
                      (float)lbar_const, N, (float *)ws, (float *)gtheta_out));
    if (!xbar_out) return NF_OK;
    return fr_gemm(ctx, d, N, L, 1, nullptr, nullptr, nullptr, 0.f, (const float *)ybar, 0, (float *)xbar_out, 0, nullptr);
  }
  const double *L = (const double *)theta + d;
  const long P = fr_params(d);
  const int ns = fr_flat_slabs(N);
  const long chunk = (N + ns - 1) / ns;
  {
    ProfScope ps(ctx, "fr_grad_flat");
    hipLaunchKernelGGL(k_fr_grad_flat<double>, dim3((unsigned)((P + FR_BLOCK - 1) / FR_BLOCK), (unsigned)ns), dim3(FR_BLOCK), 0,
                       ctx->stream, d, N, chunk, L, (const double *)x, (const double *)ybar, (const double *)lbar, lbar_const,
                       (double *)ws);
    NF_HIP(hipGetLastError());
  }
  NF_TRY(nf_launch_reduce_slabs(ctx, NF_DTYPE_F64, ws, ns, P, gtheta_out));
  if (!xbar_out) return NF_OK;
  hipLaunchKernelGGL(k_fr_apply_flat<double>, dim3((unsigned)((N + FR_BLOCK - 1) / FR_BLOCK)), dim3(FR_BLOCK), 0, ctx->stream, d, N,
                     (const double *)nullptr, L, 2, (const double *)ybar, (double *)xbar_out, (double *)nullptr);
  return (int)hipGetLastError();
}
