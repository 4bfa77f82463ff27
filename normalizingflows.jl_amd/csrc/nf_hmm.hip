// nf_hmm.hip -- the hidden-Markov-model targets (NF_TARGET_HMM_NORMAL / _POISSON / _BERNOULLI; gfx950): the states summed out by the
// forward algorithm, the score by the scaled backward recursion, both on chip.
//     y = [iota (K) ; Lambda (K x K, row-major) ; emission block (E x K, parameter-major)],   d = K + K^2 + E K,   2 <= K <= 8,
//     pi0 = softmax(iota),   P_i. = softmax(Lambda_i.),
//     log p(y) = par[1] + sum_sequences log L(y) - sum_j ((y_j - pm_j) pis_j)^2 / 2.
// Row t carries x_t, off_t, wt_t >= 0 and seg_t (non-zero: the first row of a sequence; row 0 is read as one).  Row log-emissions
// l_t(k) = wt_t logf(x_t; k), exactly 0 for wt_t == 0 by select (a missing observation: the transition still happens):
//     normal      z = (x - off - mu_k) exp(-ls_k) formed before it is squared:  -z^2 / 2 - ls_k
//     poisson     eta = omega_k + off:  x eta - exp(eta)
//     bernoulli   eta = omega_k + off:  x eta - softplus(eta)            (the exp(-|eta|) forms)
// Data: p0 = x[R] | off[R] | wt[R] | seg[R];  p1 = pm[d] | pis[d] | par[2]  (two buffers, the flow's element type).
//
// The recursion (nothing is clamped): m_t = max_k l_t(k), b_t(k) = exp(l_t(k) - m_t) <= 1 with one b exactly 1;
//     a = alpha_{t-1} P (pi0 at a sequence start),  c_t = sum_k a_k b_t(k) > 0,  alpha_t = a b_t / c_t,  log L += m_t + log c_t;
// backwards with the same c_t: beta_T = 1, r_t(j) = b_t(j) beta_t(j) / c_t, beta_{t-1}(i) = sum_j P_ij r_t(j),
//     gamma_t = alpha_t beta_t,  xi_t(i, j) = alpha_{t-1}(i) P_ij r_t(j);  at a sequence start gamma_t goes to d iota and beta restarts at 1.
//     d Lambda_ij = sum_t xi_t(i, j) - P_ij sum_t gamma_{t-1}(i),   d iota_k = sum_starts gamma_t(k) - (number of sequences) pi0_k,
//     d emission_k = sum_t wt_t gamma_t(k) dlogf / d parameter.
//
// A LANE PER (SAMPLE, STATE).  A sample's G lanes (G = 2, 4, 8: the power of two >= K) sit side by side in one wave.  Lane k keeps
// row k of P as Pr[m] = P[k][k ^ m] and column k as Pc[m] = P[k ^ m][k] (one cross-lane move of Pr[m]), its state's emission
// parameters, alpha(k) or beta(k), and its accumulators: acc[m] = sum_t xi_t(k ^ m, k), the gamma sums and the emission sums.  Every
// register array is indexed by the unrolled m.  K is a kernel argument below G: a state k >= K has a zero row and column, pi0 = 0
// and l = -inf, so nothing can enter it (three instantiations per family instead of seven).
// THE K-WAY EXCHANGE is DPP, not LDS: lane k ^ m is quad_perm for m = 1, 2, 3, row_half_mirror for m = 7 and the two composed for
// m = 4, 5, 6 -- a modifier on the v_fma that consumes it, no LDS traffic and no wait.  Group sums and maxima are the fixed order
// xor 1, xor 2, xor 7: every lane of the group holds the same bits.  There is no barrier and no LDS wait inside the forward row.
// ROW DATA are the same for every lane: they are read eight rows at a time through a pointer that is uniform over the wave.
// LDS IS THE TAPE (there is no workspace).  The forward sweep stores alpha before every L-th row (L = NF_HMM_SEGMENT = 64) as a
// checkpoint; the reverse sweep re-runs one L-row segment from its checkpoint into the segment buffer -- alpha_t(k), c_t, m_t --
// and walks it backwards; the last segment is recorded by the forward sweep itself.  Both are [row][wave][state][sample of the
// wave]: a wave's lanes address consecutive words.  A lane reads back its own alpha; c_t and m_t are written by the sample's lane 0
// and read by its G lanes after a wave-level fence.  Bytes: 128 (nseg K + min(R, L) (K + 2)) in either kernel (32 floats or 16
// doubles per row and state): 144 KB at K = 8, R = NF_HMM_MAXR = 4096; 57 KB at K = 4, R = 1024; the launch asks for what its R and
// K need.
// Two kernels per (G, family):
//   k_target_hmm_tiled  Float32, tiled layout, drop-in for k_target_tiled: 32 samples x G lanes = the first G / 2 waves; the
//                       others take no part in the sweeps (a wave-uniform skip of a region without barriers)
//   k_target_hmm        flat layout, float / double, drop-in for k_target: 16 lanes per sample, the first G of them at work
// No atomics; every sum runs in a fixed order: two launches give the same bits.
#include "nf_common.h"
#include "nf_linpred.h"
#include "nf_target_stages.h"

#define HMM_BLOCK 256
#define HMM_L NF_HMM_SEGMENT
#define HMM_RB 8  // rows whose data are requested together

// ---- the exchange: v of lane (lane ^ M) within aligned groups of eight lanes --------------------------------------------------
template <int M>
__device__ __forceinline__ int hmm_dpp(int v) {
  static_assert(M >= 1 && M <= 7, "a group is at most eight lanes");
  if constexpr (M == 1)
    return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
  else if constexpr (M == 2)
    return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
  else if constexpr (M == 3)
    return __builtin_amdgcn_update_dpp(0, v, 0x1B, 0xF, 0xF, false);  // quad_perm [3,2,1,0]
  else if constexpr (M == 7)
    return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else
    return hmm_dpp<7 - M>(hmm_dpp<7>(v));  // k ^ M = (k ^ 7) ^ (7 - M) for M = 4, 5, 6
}
template <int M>
__device__ __forceinline__ float hmm_xor(float v) {
  if constexpr (M == 0)
    return v;
  else
    return __builtin_bit_cast(float, hmm_dpp<M>(__builtin_bit_cast(int, v)));
}
template <int M>
__device__ __forceinline__ double hmm_xor(double v) {
  if constexpr (M == 0) {
    return v;
  } else {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)hmm_dpp<M>((int)(unsigned)b), hi = (unsigned)hmm_dpp<M>((int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
  }
}
// the group's sum and maximum in every lane of it: xor 1, xor 2, xor 7 (each step adds two values that both lanes hold: the same bits)
template <int G, class T>
__device__ __forceinline__ T hmm_gsum(T v) {
  v += hmm_xor<1>(v);
  if constexpr (G >= 4) v += hmm_xor<2>(v);
  if constexpr (G >= 8) v += hmm_xor<7>(v);
  return v;
}
template <class T>
__device__ __forceinline__ T hmm_max(T a, T b) {
  return a > b ? a : b;
}
template <int G, class T>
__device__ __forceinline__ T hmm_gmax(T v) {
  v = hmm_max(v, hmm_xor<1>(v));
  if constexpr (G >= 4) v = hmm_max(v, hmm_xor<2>(v));
  if constexpr (G >= 8) v = hmm_max(v, hmm_xor<7>(v));
  return v;
}

// ---- a lane's emission: l = wt logf(x; k) and wt dlogf / d(parameter 0, parameter 1), all exactly 0 at wt == 0 by select ------
template <class T, int FAM>
struct HmmEmis {
  T a, b, einv;  // normal: mu, log sigma, exp(-log sigma); poisson, bernoulli: omega
  bool live;     // a real state (k < K): the others have l = -inf
  __device__ __forceinline__ void eval(T x, T off, T wt, T &l, T &d0, T &d1) const {
    T lf;
    if constexpr (FAM == 0) {
      const T z = (x - off - a) * einv;
      lf = (T)-0.5 * z * z - b;
      d0 = z * einv;
      d1 = z * z - (T)1;
    } else if constexpr (FAM == 1) {
      const T eta = a + off, ex = lp_exp(eta);
      lf = x * eta - ex;
      d0 = x - ex;
      d1 = (T)0;
    } else {
      const T eta = a + off, e = lp_exp(eta < (T)0 ? eta : -eta), den = (T)1 + e;
      lf = x * eta - ((eta > (T)0 ? eta : (T)0) + lp_log1p(e));
      d0 = x - (eta >= (T)0 ? (T)1 / den : e / den);
      d1 = (T)0;
    }
    const bool miss = wt == (T)0;
    l = live ? (miss ? (T)0 : wt * lf) : -(T)INFINITY;
    d0 = miss ? (T)0 : wt * d0;
    d1 = miss ? (T)0 : wt * d1;
  }
};

// ---- the body: both sweeps of the caller's sample; returns log p(y) (in the G lanes of the sample) -----------------------------
// LPS lanes per sample slot (G tiled, 16 flat), SPB samples per block.  y(f): coordinate f of the lane's sample (0 for a padding
// sample); put(f, g): the score's coordinate f.  `lds`: SPB (nseg K + min(R, L) (K + 2)) elements.
template <class T, int G, int FAM, int LPS, int SPB, class YF, class PF>
__device__ __forceinline__ T hmm_body(int K, int R, const T *__restrict__ rows, const T *__restrict__ prior, T *__restrict__ lds, bool grad, YF y, PF put) {
  constexpr int SPW = 64 / LPS, E = FAM == 0 ? 2 : 1;
  const int d = K + K * K + E * K;
  const int smp = threadIdx.x / LPS, k = threadIdx.x % LPS;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sw = (threadIdx.x & 63) / LPS;
  if (wave * SPW >= SPB) return (T)0;  // (wave-uniform) a wave a small K leaves over
  const bool live = k < K;             // (K <= G <= LPS)
  const int nseg = (R + HMM_L - 1) / HMM_L;
  const int RS = (K + 2) * SPB;                                       // a segment row: alpha [wave][state][sample] | c [sample] | m [sample]
  T *ck = lds, *sb = lds + nseg * K * SPB;
  const int own = live ? wave * K * SPW + k * SPW + sw : 0;           // the lane's word of a row (read and written under `live` only)

  // softmax of iota, of row k of Lambda (the row maximum subtracted), the column by one exchange per entry
  T pi0, Pr[G], Pc[G];
  {
    const T v = live ? y(k) : -(T)INFINITY, mx = hmm_gmax<G>(v), e = live ? lp_exp(v - mx) : (T)0;
    pi0 = e / hmm_gsum<G>(e);
    T lam[G], rmx = -(T)INFINITY, s = (T)0;
#pragma unroll
    for (int m = 0; m < G; ++m) {
      const int j = k ^ m;
      lam[m] = (live && j < K) ? y(K + k * K + j) : -(T)INFINITY;
      rmx = hmm_max(rmx, lam[m]);
    }
#pragma unroll
    for (int m = 0; m < G; ++m) {
      Pr[m] = (live && (k ^ m) < K) ? lp_exp(lam[m] - rmx) : (T)0;
      s += Pr[m];
    }
#pragma unroll
    for (int m = 0; m < G; ++m) Pr[m] = live ? Pr[m] / s : (T)0;
    Pc[0] = Pr[0];
    if constexpr (G >= 2) Pc[1] = hmm_xor<1>(Pr[1]);
    if constexpr (G >= 4) Pc[2] = hmm_xor<2>(Pr[2]), Pc[3] = hmm_xor<3>(Pr[3]);
    if constexpr (G >= 8) Pc[4] = hmm_xor<4>(Pr[4]), Pc[5] = hmm_xor<5>(Pr[5]), Pc[6] = hmm_xor<6>(Pr[6]), Pc[7] = hmm_xor<7>(Pr[7]);
  }
  HmmEmis<T, FAM> em;
  em.live = live;
  em.a = live ? y(K + K * K + k) : (T)0;
  em.b = (FAM == 0 && live) ? y(K + K * K + K + k) : (T)0;
  em.einv = FAM == 0 ? lp_exp(-em.b) : (T)1;

  // sum_m w[m] v(lane ^ m), m ascending
  auto mix = [&](const T(&w)[G], T v) -> T {
    T a = w[0] * v;
    if constexpr (G >= 2) a += w[1] * hmm_xor<1>(v);
    if constexpr (G >= 4) a += w[2] * hmm_xor<2>(v), a += w[3] * hmm_xor<3>(v);
    if constexpr (G >= 8) {
      const T h = hmm_xor<7>(v);
      a += w[4] * hmm_xor<3>(h), a += w[5] * hmm_xor<2>(h), a += w[6] * hmm_xor<1>(h), a += w[7] * h;
    }
    return a;
  };

  T alpha = (T)0, beta = (T)1, logl = (T)0, nseq = (T)0;
  T acc[G], gi = (T)0, gs = (T)0, g0 = (T)0, g1 = (T)0;
#pragma unroll
  for (int m = 0; m < G; ++m) acc[m] = (T)0;

  // one loop holds both sweeps, so that there is one copy of each row body: forward over the segments ascending (checkpoints; the
  // last one recorded when a score is wanted), then per segment descending: re-run (all but the last), walk backwards
  int seg = 0;
  bool rev = false;
  for (;;) {
    const int ts = seg * HMM_L, te = ts + HMM_L < R ? ts + HMM_L : R;
    const bool rec = rev || (grad && seg == nseg - 1);
    const bool replay = rev && seg != nseg - 1;  // (the last segment's record is the forward sweep's)
    if (!rev || replay) {
      if (!rev) {
        if (live) ck[seg * K * SPB + own] = alpha;
      } else {
        alpha = live ? ck[seg * K * SPB + own] : (T)0;
      }
      for (int t0 = ts; t0 < te; t0 += HMM_RB) {
        T xv[HMM_RB], ov[HMM_RB], wv[HMM_RB], sv[HMM_RB];
#pragma unroll
        for (int u = 0; u < HMM_RB; ++u) {
          const int t = t0 + u < R ? t0 + u : R - 1;
          xv[u] = rows[t], ov[u] = rows[R + t], wv[u] = rows[2 * R + t], sv[u] = rows[3 * R + t];
        }
#pragma unroll
        for (int u = 0; u < HMM_RB; ++u) {
          const int t = t0 + u;
          if (t < te) {  // (uniform)
            const bool start = t == 0 || sv[u] != (T)0;
            T l, d0, d1;
            em.eval(xv[u], ov[u], wv[u], l, d0, d1);
            const T mt = hmm_gmax<G>(l), b = lp_exp(l - mt);
            const T a = start ? pi0 : mix(Pc, alpha);
            const T ab = a * b, c = hmm_gsum<G>(ab);
            alpha = ab / c;
            if (!rev) {
              logl += mt + lp_log(c);
              nseq += start ? (T)1 : (T)0;
            }
            if (rec) {
              T *row = sb + (t - ts) * RS;
              if (live) row[own] = alpha;
              if (k == 0) row[K * SPB + smp] = c, row[(K + 1) * SPB + smp] = mt;
            }
          }
        }
      }
      if (!rev) {
        if (seg < nseg - 1) {
          ++seg;
          continue;
        }
        if (!grad) break;
        rev = true;
      }
    }
    wave_lds_fence();  // c_t and m_t are another lane's writes
    for (int t0 = (te - 1) & ~(HMM_RB - 1); t0 >= ts; t0 -= HMM_RB) {
      T xv[HMM_RB], ov[HMM_RB], wv[HMM_RB], sv[HMM_RB];
#pragma unroll
      for (int u = 0; u < HMM_RB; ++u) {
        const int t = t0 + u < R ? t0 + u : R - 1;
        xv[u] = rows[t], ov[u] = rows[R + t], wv[u] = rows[2 * R + t], sv[u] = rows[3 * R + t];
      }
#pragma unroll
      for (int u = HMM_RB - 1; u >= 0; --u) {
        const int t = t0 + u;
        if (t < te) {  // (uniform)
          const bool start = t == 0 || sv[u] != (T)0;
          const T *row = sb + (t - ts) * RS;
          const T c = row[K * SPB + smp], mt = row[(K + 1) * SPB + smp], at = live ? row[own] : (T)0;
          const T *prow = t > ts ? row - RS : ck + seg * K * SPB;  // alpha before row t: the row above, or the segment's checkpoint
          const T ap = (live && !start) ? prow[own] : (T)0;
          T l, d0, d1;
          em.eval(xv[u], ov[u], wv[u], l, d0, d1);
          const T b = lp_exp(l - mt), gam = at * beta, r = b * beta / c;
          g0 += gam * d0;
          if constexpr (FAM == 0) g1 += gam * d1;
          gi += start ? gam : (T)0;
          // xi_t(k ^ m, k) = alpha_{t-1}(k ^ m) P[k ^ m][k] r_t(k)
          acc[0] += ap * Pc[0] * r;
          if constexpr (G >= 2) acc[1] += hmm_xor<1>(ap) * Pc[1] * r;
          if constexpr (G >= 4) acc[2] += hmm_xor<2>(ap) * Pc[2] * r, acc[3] += hmm_xor<3>(ap) * Pc[3] * r;
          if constexpr (G >= 8) {
            const T h = hmm_xor<7>(ap);
            acc[4] += hmm_xor<3>(h) * Pc[4] * r, acc[5] += hmm_xor<2>(h) * Pc[5] * r, acc[6] += hmm_xor<1>(h) * Pc[6] * r, acc[7] += h * Pc[7] * r;
          }
          const T bp = mix(Pr, r);  // beta_{t-1}(k)
          gs += ap * bp;            // gamma_{t-1}(k) (alpha_{t-1} read as 0 at a start)
          beta = start ? (T)1 : bp;
        }
      }
    }
    if (seg == 0) break;
    --seg;
    wave_lds_fence();  // the replay overwrites the segment buffer
  }

  // the prior on the lane's coordinates and the score: iota_k, column k of Lambda, the state's emission parameters
  const T *pm = prior, *pis = prior + d;
  T q = (T)0;
  auto coord = [&](int f, T g) {
    const T s = pis[f], dv = (y(f) - pm[f]) * s;
    q += dv * dv;
    if (grad) put(f, g - dv * s);
  };
  T gx[G];  // sum_t gamma_{t-1}(k ^ m) (exchanged by every lane of the wave, before the lanes part)
  gx[0] = gs;
  if constexpr (G >= 2) gx[1] = hmm_xor<1>(gs);
  if constexpr (G >= 4) gx[2] = hmm_xor<2>(gs), gx[3] = hmm_xor<3>(gs);
  if constexpr (G >= 8) gx[4] = hmm_xor<4>(gs), gx[5] = hmm_xor<5>(gs), gx[6] = hmm_xor<6>(gs), gx[7] = hmm_xor<7>(gs);
  if (live) {
    coord(k, gi - nseq * pi0);
    // d Lambda[k ^ m][k] = acc[m] - P[k ^ m][k] sum_t gamma_{t-1}(k ^ m)
#pragma unroll
    for (int m = 0; m < G; ++m)
      if ((k ^ m) < K) coord(K + (k ^ m) * K + k, acc[m] - Pc[m] * gx[m]);
    coord(K + K * K + k, g0);
    if constexpr (FAM == 0) coord(K + K * K + K + k, g1);
  }
  q = hmm_gsum<G>(q);
  return prior[2 * d + 1] + logl - (T)0.5 * q;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------
template <int G, int FAM>
__global__ __launch_bounds__(HMM_BLOCK) void k_target_hmm_tiled(int d, int R, int K, long N, const float *__restrict__ yt, const float *__restrict__ rows,
                                                                const float *__restrict__ prior, const float *__restrict__ logq,
                                                                const float *__restrict__ ladj, float *__restrict__ gt, float gscale,
                                                                float *__restrict__ elbos_out, double *__restrict__ partial, double pscale) {
  extern __shared__ float hmm_lds[];
  __shared__ double sm[HMM_BLOCK / 64];
  const int smp = threadIdx.x / G;  // (samples 32 .. : the waves that take no part)
  const long tile = blockIdx.x, j = tile * 32 + smp;
  const bool valid = smp < 32 && j < N;
  const float *yb = yt + tile * d * 32;
  float *gb = gt ? gt + tile * d * 32 : nullptr;
  const float lp = hmm_body<float, G, FAM, G, 32>(
      K, R, rows, prior, hmm_lds, gt != nullptr, [&](int f) { return valid ? yb[f * 32 + smp] : 0.f; },
      [&](int f, float g) { gb[f * 32 + smp] = valid ? gscale * g : 0.f; });
  double contrib = 0.0;
  if (valid && threadIdx.x % G == 0) contrib = tgt_elbo_term(lp, j, logq, ladj, elbos_out, pscale);
  tgt_block_partial(contrib, sm, partial);
}

template <class T, int G, int FAM>
__global__ __launch_bounds__(HMM_BLOCK) void k_target_hmm(int d, int R, int K, long N, const T *__restrict__ y, const T *__restrict__ rows,
                                                          const T *__restrict__ prior, const T *__restrict__ logq, const T *__restrict__ ladj,
                                                          T *__restrict__ logp_out, T *__restrict__ grad_out, T gscale, T *__restrict__ elbos_out,
                                                          double *__restrict__ partial, double pscale) {
  extern __shared__ double hmmf_lds[];
  __shared__ double sm[HMM_BLOCK / 64];
  const long j = (long)blockIdx.x * 16 + threadIdx.x / 16;
  const bool valid = j < N;
  const T lp = hmm_body<T, G, FAM, 16, 16>(
      K, R, rows, prior, (T *)hmmf_lds, grad_out != nullptr, [&](int f) { return valid ? y[j * d + f] : (T)0; },
      [&](int f, T g) {
        if (valid) grad_out[j * d + f] = gscale * g;
      });
  double contrib = 0.0;
  if (valid && threadIdx.x % 16 == 0) {
    if (logp_out) logp_out[j] = lp;
    contrib = tgt_elbo_term(lp, j, logq, ladj, elbos_out, pscale);
  }
  tgt_block_partial(contrib, sm, partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers (called by nf_launch_target / nf_launch_target_tiled after nf_target_check: s0 = R in 1 .. NF_HMM_MAXR, s1 = K in 2 .. 8,
// d = K + K^2 + E K)
// ---------------------------------------------------------------------------------------------------------------------
// elements of LDS a launch takes: the checkpoints and the segment buffer, 32 floats or 16 doubles per row and state
static size_t hmm_lds_elems(int spb, int R, int K) {
  const int nseg = (R + HMM_L - 1) / HMM_L, lrows = R < HMM_L ? R : HMM_L;
  return (size_t)spb * ((size_t)nseg * K + (size_t)lrows * (K + 2));
}

// f(G, FAM as integral constants) for the kind and the group that holds K
template <class F>
static int hmm_dispatch(int kind, int K, F &&f) {
  auto fam = [&](auto g) {
    if (kind == NF_TARGET_HMM_NORMAL) return f(g, std::integral_constant<int, 0>());
    if (kind == NF_TARGET_HMM_POISSON) return f(g, std::integral_constant<int, 1>());
    return f(g, std::integral_constant<int, 2>());
  };
  if (K <= 2) return fam(std::integral_constant<int, 2>());
  if (K <= 4) return fam(std::integral_constant<int, 4>());
  return fam(std::integral_constant<int, 8>());
}

int nf_launch_target_hmm_tiled(const TgtTiledArgs &a) {
  const int R = (int)a.t->s0, K = (int)a.t->s1;
  if (K < 2 || K > 8 || R < 1 || R > NF_HMM_MAXR) return NF_ERR_UNSUPPORTED;
  return hmm_dispatch(a.t->kind, K, [&](auto g, auto fam) {
    nf_ctx *ctx = a.ctx;
    NF_TRY((nf_lds_once<k_target_hmm_tiled<g(), fam()>>(ctx, hmm_lds_elems(32, NF_HMM_MAXR, 8) * sizeof(float))));
    ProfScope ps(ctx, "target_hmm");
    return tgt_launch_tiled<k_target_hmm_tiled<g(), fam()>>(a, hmm_lds_elems(32, R, K) * sizeof(float), a.d, R, K, a.N, a.yt, (const float *)a.t->p0,
                                                            (const float *)a.t->p1);
  });
}

template <class T>
static int launch_hmm_flat(const TgtFlatArgs &a) {
  const int R = (int)a.t->s0, K = (int)a.t->s1;
  return hmm_dispatch(a.t->kind, K, [&](auto g, auto fam) {
    nf_ctx *ctx = a.ctx;
    NF_TRY((nf_lds_once<k_target_hmm<T, g(), fam()>>(ctx, hmm_lds_elems(16, NF_HMM_MAXR, 8) * sizeof(T))));
    ProfScope ps(ctx, "target_hmm");
    return tgt_launch_flat<k_target_hmm<T, g(), fam()>, T>(a, hmm_lds_elems(16, R, K) * sizeof(T), a.d, R, K, a.N, (const T *)a.y, (const T *)a.t->p0,
                                                           (const T *)a.t->p1);
  });
}

int nf_launch_target_hmm(const TgtFlatArgs &a) {
  const int R = (int)a.t->s0, K = (int)a.t->s1;
  if (K < 2 || K > 8 || R < 1 || R > NF_HMM_MAXR) return NF_ERR_UNSUPPORTED;
  return tgt_dispatch_dtype(a.dtype, [&](auto e) { return launch_hmm_flat<decltype(e)>(a); });
}
