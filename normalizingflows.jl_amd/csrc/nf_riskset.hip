// nf_riskset.hip -- the risk-set regression target (NF_TARGET_RISKSET; gfx950): Cox partial likelihood, conditional logit, rankings.
//     y = beta in R^d (d = p);   eta_i = x_i . y + off_i,   a_i = eta_i + logw_i,   seg(i) the contiguous segment of row i,
//     c_i      = log sum_{j in seg(i), j <= i} w_j exp(eta_j)        (inclusive prefix log-sum-exp inside the segment)
//     log p(y) = par[1] + lin . y - sum_i m_i c_i - par[0]/2 |y|^2
// The first target whose rows interact.  Score with respect to eta_j:  r_j = -exp(a_j - c_j) V_j,
//     V_j = m_j + V_{j+1} exp(c_j - c_{j+1})   backwards inside the segment,   V = m on the segment's last row;   d y = X' r + lin - par[0] y.
// c is non-decreasing inside a segment and a_j <= c_j: every exponential has an argument <= 0.  Forward: c_i = logaddexp(c_{i-1}, a_i).
// Nothing is clamped and no ratio of sums is formed.
// Data: X [R x p] row-major in the host's order, the tail padded to a multiple of 32 by rows of weight 0 (a segment may start at any
// row);  p0 = off[R] | logw[R] | m[R] | segstart[R] | lin[d] | par[2]  (RsRows below).  A row of logw = -inf is dropped from every risk
// set by SELECT: its predictor is never consumed.  Every flag read from the buffer is bounded by select before it steers anything.
// Two kernels, the counterparts of nf_ordinal.hip's:
//   k_target_riskset_tiled  Float32, tiled layout, drop-in for k_target_tiled: both GEMMs on v_mfma_f32_32x32x2_f32, the two
//                           recurrences as scans over the accumulator registers between them
//   k_target_riskset        flat layout, float / double, drop-in for k_target: vector pipe (Float64 flows, nf_target_logp)
// Both scans are associative: the forward one over (c, "a segment starts in the range"), the backward one over the affine maps
// V_in -> A + F V_in, so a range of rows is summarised by two numbers and ranges are combined in row order -- no atomics, the same bits
// on every launch.
#include <math.h>

#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define RS_BLOCK 256
#define RS_WAVES 4
#define RS_MAXD 256
#define RS_CW 128  // features of X a wave's image holds at a time

// The row data, addressed inside the one buffer p0 = off[R] | logw[R] | m[R] | segstart[R] | lin[d] | par[2].
template <class T>
struct RsRows {
  const T *off, *logw, *m, *seg, *lin, *par;
  __device__ __forceinline__ RsRows(const T *p0, int R, int d)
      : off(p0), logw(p0 + R), m(p0 + 2 * (long)R), seg(p0 + 3 * (long)R), lin(p0 + 4 * (long)R), par(p0 + 4 * (long)R + d) {}
  // The host cannot validate device memory: these bound what the buffer holds by select (NaN: a dropped row, no mass, a start).
  static __device__ __forceinline__ bool live(T lw) { return lw > -(T)INFINITY; }
  static __device__ __forceinline__ T mass(T v) { return v > (T)0 ? v : (T)0; }
  static __device__ __forceinline__ bool start(T v) { return !(v == (T)0); }
};

// log(exp(a) + exp(b)); -inf (the empty sum) is the identity, by select
template <class T>
__device__ __forceinline__ T rs_lae(T a, T b) {
  const T hi = a > b ? a : b, lo = a > b ? b : a;
  return lo == -(T)INFINITY ? hi : hi + lp_log1p(lp_exp(lo - hi));
}
// exp(c - cn), the factor V takes from row j + 1 to row j: 0 where row j + 1 starts a segment or row j's prefix is empty
template <class T>
__device__ __forceinline__ T rs_link(bool startnext, T c, T cn) {
  return (startnext || c == -(T)INFINITY) ? (T)0 : lp_exp(c - cn);
}

// ---------------------------------------------------------------------------------------------------------------------
// tiled kernel
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 32-sample tile (one double partial per tile, as k_target_tiled leaves).  The tile sits in LDS,
// [feature][sample], features >= d and padding samples zero, with eight zero feature rows behind the 32 DB.  The 32-row blocks of X are
// taken four at a time ("super-block"): wave w owns block 4 k + w, stages it into an image of its own (nf_ordinal.hip's geometry) and
// runs GEMM 1, U = off + X Y, in the C layout: register r of a lane of half `hi` is row nf_row(r, hi) of sample l & 31.
//   sweep 1, k ascending: the block's (c, start) aggregate by a scan over the lane's registers (groups of four rows), across the two
//            half-waves (the eight group totals) -- published through LDS, combined in wave order after ONE barrier per super-block;
//            the carry INTO each block is kept in LDS, [block][sample] (4 R bytes: NF_RISKSET_MAXR bounds it to 32 KB).
//   sweep 2, k descending: GEMM 1 again (the recompute of nf_bnn.hip), c of every row from the stored carry, then the block's V as
//            A + F V_in by the same two-level scan backwards; (A, F, c_first, c_last) of the block's first row are published, combined
//            in reverse wave order after one barrier, r = -exp(a - c) (A + F V_in) is left in the accumulator registers, which ARE
//            GEMM 2's B operand:  G += X' r.
// Interleaving the blocks over the waves (not one contiguous range per wave) is what keeps this at two GEMM 1 and one GEMM 2: the V
// that enters a contiguous range is known only when the whole range behind it has been swept, so ranges would either run one after
// the other or carry a second accumulator set for the part of G that is linear in the entering V.
// Shared stages (nf_target_stages.h): tgt_stage and tgt_gemm1 (the wave's image of a row block, GEMM 1 from it), tgt_elbo_term (both
// kernels), tgt_block_partial (the flat kernel; the tiled one keeps it in place), and the launch helpers; what else stands here in
// place does so for nf_ordinal.hip's reason.
template <int DB>
struct RsGeo {
  static constexpr int YT = 32 * DB * 32;
  static constexpr int YTP = YT + 8 * 32;
  static constexpr int PMAX = 32 * DB;
  __host__ __device__ static constexpr int stride(int p) { return 32 * (((p < RS_CW ? p : RS_CW) + 31) >> 5) + 1; }
  __host__ __device__ static constexpr int floats(int p, int R) { return YTP + RS_WAVES * 32 * stride(p) + R; }  // + [R / 32][32] carries
};

// a = eta + logw of the block's rows, -inf by select where the row is dropped; the image is left holding the LAST chunk
__device__ __forceinline__ f32x16 rs_block_a(float *__restrict__ img, int S, const float *__restrict__ X, const float *__restrict__ sY,
                                             const RsRows<float> &rd, int i0, int p, int nch, int lane, int l31, int hi) {
  float lw[16];  // (requested before the staging loads: in by the time the image is)
  f32x16 U;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + nf_row(r, hi);
    U[r] = rd.off[i];
    lw[r] = rd.logw[i];
  }
  for (int ch = 0; ch < nch; ++ch) {
    const int f0 = ch * RS_CW, pc = p - f0 < RS_CW ? p - f0 : RS_CW;
    tgt_stage(img, S, X, i0, p, f0, pc, lane);
    wave_lds_fence();
    U = tgt_gemm1(U, img, S, sY + f0 * 32, pc, l31, hi);
    if (ch + 1 < nch) wave_lds_fence();  // the next chunk overwrites the image
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) U[r] = RsRows<float>::live(lw[r]) ? U[r] + lw[r] : -INFINITY;
  return U;
}

// bit j of the result: row i0 + j starts a segment (row 0 always does); wave-uniform
__device__ __forceinline__ unsigned rs_starts(const RsRows<float> &rd, int i0, int l31) {
  const unsigned long long b = __ballot(RsRows<float>::start(rd.seg[i0 + l31]));
  return (unsigned)b | (i0 == 0 ? 1u : 0u);
}

// The forward scan of one block: c[r] = the inclusive segmented prefix log-sum-exp at row nf_row(r, hi), given the carry cin into the
// block; returns the carry out of it.  FULL = false leaves c as the in-group prefixes (only the carry is wanted).
template <bool FULL>
__device__ __forceinline__ float rs_scan(const f32x16 &a, unsigned sm, float cin, int hi, float (&c)[16]) {
  float tot[4], oth[4], pin[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {  // inside the lane's groups of four rows
    const int sh = 8 * g + 4 * hi;
    float run = a[4 * g];
    c[4 * g] = run;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
      run = ((sm >> (sh + e)) & 1u) ? a[4 * g + e] : rs_lae(run, a[4 * g + e]);
      c[4 * g + e] = run;
    }
    tot[g] = run;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) oth[g] = __shfl_xor(tot[g], 32, 64);
  float P = cin;
#pragma unroll
  for (int gg = 0; gg < 8; ++gg) {  // over the eight groups, in row order: even groups belong to half 0, odd ones to half 1
    const bool mine = (gg & 1) == hi;
    const float T = mine ? tot[gg >> 1] : oth[gg >> 1];
    if ((gg & 1) == 0) pin[gg >> 1] = P;
    else pin[gg >> 1] = mine ? P : pin[gg >> 1];
    P = ((sm >> (4 * gg)) & 0xFu) ? T : rs_lae(P, T);
  }
  if (FULL) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int sh = 8 * (r >> 2) + 4 * hi;
      const bool started = ((sm >> sh) & ((2u << (r & 3)) - 1u)) != 0u;  // a start at or before the row, inside its group
      c[r] = started ? c[r] : rs_lae(pin[r >> 2], c[r]);
    }
  }
  return P;
}

// The backward scan of one block: V at row nf_row(r, hi) = A[r] + F[r] V_in, V_in what enters the block's LAST row from behind it
// (V_31 = m_31 + V_in).  A0 / F0: the pair of the block's first row.
__device__ __forceinline__ void rs_back(const float (&c)[16], const float (&m)[16], unsigned sm, int hi, float (&A)[16], float (&F)[16],
                                        float &A0, float &F0) {
  float xc[4], fl[4], Ag[4], Hg[4], oA[4], oH[4], vinA[4], vinF[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xc[g] = __shfl_xor(c[4 * g], 32, 64);  // c of the other half's group firsts
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int sh = 8 * g + 4 * hi;
    A[4 * g + 3] = m[4 * g + 3];
    F[4 * g + 3] = 1.f;
#pragma unroll
    for (int e = 2; e >= 0; --e) {
      const int r = 4 * g + e;
      const float f = rs_link(((sm >> (sh + e + 1)) & 1u) != 0u, c[r], c[r + 1]);
      A[r] = m[r] + f * A[r + 1];
      F[r] = f * F[r + 1];
    }
    // from the group's last row to the next group's first one (the other half's); the block's last row takes V_in itself
    const bool last = g == 3 && hi == 1;
    const float cn = hi ? xc[g < 3 ? g + 1 : 3] : xc[g];  // (unused at the block's last row)
    const int nr = sh + 4;
    const bool st = nr < 32 ? ((sm >> (nr & 31)) & 1u) != 0u : false;
    fl[g] = last ? 1.f : rs_link(st, c[4 * g + 3], cn);
    Ag[g] = A[4 * g];
    Hg[g] = F[4 * g] * fl[g];
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    oA[g] = __shfl_xor(Ag[g], 32, 64);
    oH[g] = __shfl_xor(Hg[g], 32, 64);
  }
  float AA = 0.f, FF = 1.f;  // V of the next group's first row = AA + FF V_in
#pragma unroll
  for (int gg = 7; gg >= 0; --gg) {
    const bool mine = (gg & 1) == hi;
    const int g = gg >> 1;
    if ((gg & 1) == 1) {
      vinA[g] = fl[g] * AA;  // (kept by half 1; half 0 overwrites it at its own group below)
      vinF[g] = fl[g] * FF;
    } else {
      vinA[g] = mine ? fl[g] * AA : vinA[g];
      vinF[g] = mine ? fl[g] * FF : vinF[g];
    }
    const float a_ = mine ? Ag[g] : oA[g], h_ = mine ? Hg[g] : oH[g];
    AA = a_ + h_ * AA;
    FF = h_ * FF;
  }
  A0 = AA;
  F0 = FF;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    A[r] = A[r] + F[r] * vinA[r >> 2];
    F[r] = F[r] * vinF[r >> 2];
  }
}

template <int DB>
__global__ __launch_bounds__(RS_BLOCK, DB <= 2 ? 2 : 1) void k_target_riskset_tiled(int d, int R, long N, const float *__restrict__ yt,
                                                                                   const float *__restrict__ p0, const float *__restrict__ X,
                                                                                   const float *__restrict__ logq, const float *__restrict__ ladj,
                                                                                   float *__restrict__ gt, float gscale, float *__restrict__ elbos_out,
                                                                                   double *__restrict__ partial, double pscale) {
  using G = RsGeo<DB>;
  const RsRows<float> rd(p0, R, d);
  const int p = d;
  const int S = G::stride(p);
  const int nch = DB == 8 ? (p + RS_CW - 1) / RS_CW : 1;  // (p <= 128 below DB = 8)
  extern __shared__ float rs_lds[];
  float *sY = rs_lds;
  float *sA = rs_lds + G::YTP;
  float *sCar = sA + RS_WAVES * 32 * S;          // [block][sample]: the carry into the block
  __shared__ float sAgg[2][RS_WAVES][32];        // [parity][wave][sample]: the block's c aggregate
  __shared__ int sAggF[2][RS_WAVES];             //                         ... a segment starts inside it
  __shared__ float sBk[2][RS_WAVES][4][32];      // [parity][wave][A0, F0, c_first, c_last][sample]
  __shared__ int sBkF[2][RS_WAVES];              //                         ... its first row starts a segment
  __shared__ float sL[RS_WAVES][64];             // [wave][lane] log-p partial sums
  __shared__ float red[RS_BLOCK / 32][32], red2[RS_BLOCK / 32][32];
  __shared__ double sm[RS_WAVES];
  const long tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float *yb = yt + tile * d * 32;

  {  // every load of the tile is issued before the first LDS store
    constexpr int PER = G::YTP / RS_BLOCK;
    float yv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int idx = threadIdx.x + k * RS_BLOCK, f = idx >> 5, s = idx & 31;
      yv[k] = (f < d && tile * 32 + s < N) ? yb[idx] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) sY[threadIdx.x + k * RS_BLOCK] = yv[k];
  }
  __syncthreads();

  float *img = sA + wave * 32 * S;
  const int nrb = R >> 5, nsb = (nrb + RS_WAVES - 1) / RS_WAVES;

  // ---- sweep 1: the carry into every block -----------------------------------------------------------------------------------------
  {
    float run = -INFINITY;  // c at the end of the previous super-block (every wave keeps it)
    for (int k = 0; k < nsb; ++k) {
      const int rb = RS_WAVES * k + wave, par = k & 1;
      const bool valid = rb < nrb;
      float Cb = -INFINITY;
      unsigned smk = 0u;
      if (valid) {
        const f32x16 a = rs_block_a(img, S, X, sY, rd, rb * 32, p, nch, lane, l31, hi);
        smk = rs_starts(rd, rb * 32, l31);
        float c[16];
        Cb = rs_scan<false>(a, smk, -INFINITY, hi, c);
      }
      if (hi == 0) sAgg[par][wave][l31] = Cb;
      if (lane == 0) sAggF[par][wave] = smk != 0u;
      __syncthreads();  // (also: the image is free again)
      float cin = run, mine = run;
#pragma unroll
      for (int b = 0; b < RS_WAVES; ++b) {
        mine = b == wave ? cin : mine;
        const float cb = sAgg[par][b][l31];
        cin = sAggF[par][b] ? cb : rs_lae(cin, cb);
      }
      run = cin;
      if (valid && hi == 0) sCar[rb * 32 + l31] = mine;
    }
  }

  // ---- sweep 2: c and V of every row, r, GEMM 2 ------------------------------------------------------------------------------------
  f32x16 Gacc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) Gacc[b][r] = 0.f;
  float lp = 0.f;
  {
    float Vn = 0.f, cn = 0.f;  // V and c of the first row behind the super-block, and whether it starts a segment (the end does)
    int sn = 1;
    for (int k = nsb - 1; k >= 0; --k) {
      const int rb = RS_WAVES * k + wave, par = k & 1;
      const bool valid = rb < nrb;
      const int i0 = rb * 32;
      f32x16 U;
      float A[16], F[16];
      float A0 = 0.f, F0 = 0.f, cf = 0.f, cl = 0.f;
      int s0 = 1;  // a block behind the last one: nothing enters through it
      if (valid) {
        float m[16], c[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = RsRows<float>::mass(rd.m[i0 + nf_row(r, hi)]);
        U = rs_block_a(img, S, X, sY, rd, i0, p, nch, lane, l31, hi);
        const unsigned smk = rs_starts(rd, i0, l31);
        cl = rs_scan<true>(U, smk, sCar[i0 + l31], hi, c);
        cf = __shfl(c[0], l31, 64);  // row 0 is register 0 of half 0
        s0 = (int)(smk & 1u);
        rs_back(c, m, smk, hi, A, F, A0, F0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          lp -= m[r] > 0.f ? m[r] * c[r] : 0.f;
          U[r] = U[r] > -INFINITY ? lp_exp(U[r] - c[r]) : 0.f;  // exp(a - c), 0 for a dropped row by select
        }
      }
      if (hi == 0) {
        sBk[par][wave][0][l31] = A0;
        sBk[par][wave][1][l31] = F0;
        sBk[par][wave][2][l31] = cf;
        sBk[par][wave][3][l31] = cl;
      }
      if (lane == 0) sBkF[par][wave] = s0;
      __syncthreads();
      float vin = 0.f;
#pragma unroll
      for (int b = RS_WAVES - 1; b >= 0; --b) {
        const float v = rs_link(sn != 0, sBk[par][b][3][l31], cn) * Vn;  // what enters block b's last row
        vin = b == wave ? v : vin;
        Vn = sBk[par][b][0][l31] + sBk[par][b][1][l31] * v;
        cn = sBk[par][b][2][l31];
        sn = sBkF[par][b];
      }
      if (valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) U[r] = -U[r] * (A[r] + F[r] * vin);
        for (int ch = nch - 1; ch >= 0; --ch) {
          const int f0 = ch * RS_CW, pc = p - f0 < RS_CW ? p - f0 : RS_CW;
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
    }
  }

  // the four waves' gradients, combined in wave order into the feature rows of the tile
  sL[wave][lane] = lp;
  for (int w = 0; w < RS_WAVES; ++w) {
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

  // epilogue in k_target_tiled's thread layout: thread (q, s) owns features q, q + 8, ... of sample s
  const float pw = rd.par[0];
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  const long j = tile * 32 + s;
  const bool valid = j < N;
  float yy = 0.f, ly = 0.f;
  {
    constexpr int PER = 4 * DB;  // features per thread: q, q + 8, ...
    float yv[PER], lv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (RS_BLOCK / 32);
      yv[k] = (valid && i < d) ? yb[i * 32 + s] : 0.f;
      lv[k] = i < d ? rd.lin[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = q + k * (RS_BLOCK / 32);
      yy += yv[k] * yv[k];
      ly += lv[k] * yv[k];
      if (gt && i < d) gt[tile * d * 32 + i * 32 + s] = valid ? gscale * (sY[i * 32 + s] + lv[k] - pw * yv[k]) : 0.f;
    }
  }
  red[q][s] = yy;
  red2[q][s] = ly;
  __syncthreads();
  double contrib = 0.0;
  if (q == 0 && valid) {
    float tb = 0.f, tl = 0.f, l = 0.f;
#pragma unroll
    for (int k = 0; k < RS_BLOCK / 32; ++k) {
      tb += red[k][s];
      tl += red2[k][s];
    }
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) l += sL[w][s] + sL[w][32 + s];
    float e = rd.par[1] + tl + l - 0.5f * pw * tb;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  if (partial) {  // (tgt_block_partial, in place: as a call it reorders the kernel's last instructions, and the DB = 8 kernel then measured 0.08 % outside the parent's spread)
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
// k_target's thread layout: 16 lanes per sample, 16 samples per block, one partial per block.  X passes through LDS in blocks of
// 16 rows: lane q of a sample takes row q -- eta, a --, a goes through LDS as [sample][row], and every lane of the sample runs the two
// recurrences over the block's 16 rows in row order (the plain sequential form: c = logaddexp(c, a), V = m + V exp(c - c_next)) and
// keeps what belongs to its own row.  Sweep 1 leaves the carry into every block in LDS, [block][sample]; sweep 2 runs the blocks in
// reverse, r goes through LDS as [sample][row], and lane q then owns the features q, q + 16, ... of d y.
#define RSF_LANES 16
#define RSF_SPB (RS_BLOCK / RSF_LANES)
#define RSF_RB 16

template <class T>
__global__ __launch_bounds__(RS_BLOCK) void k_target_riskset(int d, int R, long N, const T *__restrict__ y, const T *__restrict__ p0,
                                                             const T *__restrict__ X, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                             T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale,
                                                             T *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  const RsRows<T> rd(p0, R, d);
  const T pw = rd.par[0];
  const int p = d;
  extern __shared__ double rsf_lds[];
  const int S = d + 1, SD = RSF_RB + 1;
  T *sY = (T *)rsf_lds;          // [sample][d + 1]
  T *sA = sY + RSF_SPB * S;      // [row][d + 1]
  T *sD = sA + RSF_RB * S;       // [sample][row]: a, then r
  T *sCar = sD + RSF_SPB * SD;   // [block][sample]: the carry into the block
  __shared__ double sm[RS_BLOCK / 64];
  const int q = threadIdx.x & (RSF_LANES - 1), sl = threadIdx.x / RSF_LANES;
  const long j = (long)blockIdx.x * RSF_SPB + sl;
  const bool valid = j < N;
  for (int idx = threadIdx.x; idx < RSF_SPB * d; idx += RS_BLOCK) {
    const int si = idx / d, f = idx - si * d;
    const long jj = (long)blockIdx.x * RSF_SPB + si;
    sY[si * S + f] = jj < N ? y[jj * d + f] : (T)0;
  }
  const T *py = sY + sl * S;
  const int nb = R / RSF_RB;

  // a of row i0 + q of the lane's sample -> sD[sample][q]; ends behind a barrier
  auto block_a = [&](int i0) -> T {
    const T of = rd.off[i0 + q], lw = rd.logw[i0 + q];  // (requested with the block of X)
    __syncthreads();  // the tile (first pass); the previous block's readers
    for (int idx = threadIdx.x; idx < RSF_RB * p; idx += RS_BLOCK) {
      const int row = idx / p, f = idx - row * p;
      sA[row * S + f] = X[(long)(i0 + row) * p + f];
    }
    __syncthreads();
    T eta = of;
    for (int f = 0; f < p; ++f) eta += sA[q * S + f] * py[f];
    const T a = RsRows<T>::live(lw) ? eta + lw : -(T)INFINITY;
    sD[sl * SD + q] = a;
    __syncthreads();
    return a;
  };

  // ---- sweep 1 ----
  {
    T run = -(T)INFINITY;
    for (int b = 0; b < nb; ++b) {
      const int i0 = b * RSF_RB;
      block_a(i0);
      if (q == 0) sCar[b * RSF_SPB + sl] = run;
#pragma unroll
      for (int r = 0; r < RSF_RB; ++r) {
        const bool st = (i0 + r == 0) || RsRows<T>::start(rd.seg[i0 + r]);
        const T a = sD[sl * SD + r];
        run = st ? a : rs_lae(run, a);
      }
    }
  }

  // ---- sweep 2 ----
  T g[RS_MAXD / RSF_LANES];
#pragma unroll
  for (int k = 0; k < RS_MAXD / RSF_LANES; ++k) g[k] = (T)0;
  T lp = 0;
  {
    T Vn = 0, cn = 0;  // V and c of the first row behind the block, and whether it starts a segment (the end does)
    bool sn = true;
    for (int b = nb - 1; b >= 0; --b) {
      const int i0 = b * RSF_RB;
      const T a = block_a(i0);
      T cc[RSF_RB];
      T run = sCar[b * RSF_SPB + sl], myc = 0, myV = 0;
#pragma unroll
      for (int r = 0; r < RSF_RB; ++r) {
        const bool st = (i0 + r == 0) || RsRows<T>::start(rd.seg[i0 + r]);
        const T ar = sD[sl * SD + r];
        run = st ? ar : rs_lae(run, ar);
        cc[r] = run;
        myc = r == q ? run : myc;
      }
      T V = Vn, cnext = cn;
      bool snext = sn;
#pragma unroll
      for (int r = RSF_RB - 1; r >= 0; --r) {
        V = RsRows<T>::mass(rd.m[i0 + r]) + rs_link(snext, cc[r], cnext) * V;
        myV = r == q ? V : myV;
        cnext = cc[r];
        snext = (i0 + r == 0) || RsRows<T>::start(rd.seg[i0 + r]);
      }
      Vn = V;
      cn = cnext;
      sn = snext;
      const T mq = RsRows<T>::mass(rd.m[i0 + q]);
      lp -= mq > (T)0 ? mq * myc : (T)0;
      __syncthreads();  // every lane has read a
      sD[sl * SD + q] = a > -(T)INFINITY ? -lp_exp(a - myc) * myV : (T)0;
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < RS_MAXD / RSF_LANES; ++kk) {
        const int f = kk * RSF_LANES + q;
        if (f < p) {
          T acc = g[kk];
          const T *pd = sD + sl * SD;
          const T *px = sA + f;
#pragma unroll
          for (int r = 0; r < RSF_RB; ++r) acc += px[r * S] * pd[r];
          g[kk] = acc;
        }
      }
    }
  }
  lp = group16_sum(lp);
  T yy = 0, ly = 0;
#pragma unroll
  for (int kk = 0; kk < RS_MAXD / RSF_LANES; ++kk) {
    const int f = kk * RSF_LANES + q;
    if (f < d && valid) {
      const T yv = y[j * d + f], lv = rd.lin[f];
      yy += yv * yv;
      ly += lv * yv;
      if (grad_out) grad_out[j * d + f] = gscale * (g[kk] + lv - pw * yv);
    }
  }
  yy = group16_sum(yy);
  ly = group16_sum(ly);
  double contrib = 0.0;
  if (valid && q == 0) {
    T e = rd.par[1] + ly + lp - (T)0.5 * pw * yy;
    if (logp_out) logp_out[j] = e;
    contrib = tgt_elbo_term(e, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = R, a multiple of 32, R <= NF_RISKSET_MAXR)
// ---------------------------------------------------------------------------------------------------------------------
template <int DB>
static int launch_riskset_tiled(const TgtTiledArgs &a) {
  using G = RsGeo<DB>;
  const int R = (int)a.t->s0;
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_riskset_tiled<DB>>(ctx, G::floats(G::PMAX, NF_RISKSET_MAXR) * sizeof(float)));
  ProfScope ps(ctx, "target_riskset");
  return tgt_launch_tiled<k_target_riskset_tiled<DB>>(a, (size_t)G::floats(a.d, R) * sizeof(float), a.d, R, a.N, a.yt, (const float *)a.t->p0,
                                                      (const float *)a.t->p1);
}

int nf_launch_target_riskset_tiled(const TgtTiledArgs &a) {
  if (a.d > RS_MAXD || a.t->s0 > (double)NF_RISKSET_MAXR) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_db(a.d, [&](auto db) { return launch_riskset_tiled<db()>(a); });
}

// elements of LDS the flat kernel takes at (d, R)
static size_t riskset_flat_lds(int d, int R) {
  return (size_t)(RSF_SPB * (d + 1) + RSF_RB * (d + 1) + RSF_SPB * (RSF_RB + 1) + (R / RSF_RB) * RSF_SPB);
}

template <class T>
static int launch_riskset_flat(const TgtFlatArgs &a) {
  const int R = (int)a.t->s0;
  nf_ctx *ctx = a.ctx;
  NF_TRY(nf_lds_once<k_target_riskset<T>>(ctx, riskset_flat_lds(RS_MAXD, NF_RISKSET_MAXR) * sizeof(T)));  // the most any served target takes
  ProfScope ps(ctx, "target_riskset");
  return tgt_launch_flat<k_target_riskset<T>, T>(a, riskset_flat_lds(a.d, R) * sizeof(T), a.d, R, a.N, (const T *)a.y, (const T *)a.t->p0,
                                                 (const T *)a.t->p1);
}

int nf_launch_target_riskset(const TgtFlatArgs &a) {
  if (a.d > RS_MAXD || a.t->s0 > (double)NF_RISKSET_MAXR) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_riskset_flat<decltype(e)>(a); });
}
