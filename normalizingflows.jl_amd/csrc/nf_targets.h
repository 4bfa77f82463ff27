// nf_targets.h -- the built-in target log-densities, one feature at a time (shared by the stand-alone
// target kernels of nf_elementwise.hip, the fused ELBO forwards and steps of nf_simple.hip and, through
// nf_target_epilogue.h, the chain kernels), the NF_TGT_* sets of kinds a kernel instantiation serves, and
// nf_with_target_kind, the one place a run-time kind becomes a compile-time one.
#pragma once
#include <type_traits>

#include "nf_common.h"

// Built-in targets.  target_term returns feature i's additive share of log p(y) (their sum over
// i = 0..d-1 is log p) and g = d log p / d y_i.  y0, y1 are the sample's first two coordinates and
// s2 = sum_{i>=1} y_i^2 (Funnel only).  s0, s1 are the two scalar parameters of the target:
//   DIAGGAUSS  MvNormal(mu, Diagonal(var))                   test/flow.jl:43-46
//   BANANA     (b, var)       example/targets/banana.jl:58-63,77-83
//   FUNNEL     (mu, sigma)    example/targets/neal_funnel.jl:53-72 (`score` is the gradient)
//   WARPED     (sigma1, sigma2), d = 2   example/targets/warped_gaussian.jl:51-87 (with its + log r term)
//   CROSS      (mu, sigma), d = 2        example/targets/cross.jl:30-37 (components as the code builds them)
template <int kind, class T>
__device__ __forceinline__ T target_term(int d, int i, T v, T y0, T y1, T s2, const T *__restrict__ mu,
                                         const T *__restrict__ var, T s0, T s1, T &g) {
  const T L2PI = (T)1.8378770664093453;
  if (kind == NF_TARGET_DIAGGAUSS) {
    const T vv = var[i];
    const T r = v - mu[i];
    g = -r / vv;
    return (T)-0.5 * (L2PI + log(vv) + r * r / vv);
  }
  if (kind == NF_TARGET_BANANA) {
    const T y2 = y1 + s0 * y0 * y0 - s1 * s0;
    if (i == 0) {
      g = -v / s1 - (T)2 * s0 * v * y2;
      return (T)-0.5 * v * v / s1 - (log(s1) / (T)d + L2PI) * (T)d / (T)2;
    }
    if (i == 1) {
      g = -y2;
      return (T)-0.5 * y2 * y2;
    }
    g = -v;
    return (T)-0.5 * v * v;
  }
  if (kind == NF_TARGET_FUNNEL) {
    const T a = exp(-y0);
    if (i == 0) {
      const T z = (y0 - s0) / s1;
      g = -z / s1 - (T)(d - 1) / (T)2 + a * s2 / (T)2;
      return (T)-0.5 * L2PI - log(s1) - (T)0.5 * z * z - (T)0.5 * (T)(d - 1) * (L2PI + y0);
    }
    g = -a * v;
    return (T)-0.5 * a * v * v;
  }
  if (kind == NF_TARGET_WARPED) {
    const T r = sqrt(y0 * y0 + y1 * y1);
    const T th = atan2(y1, y0) + r / (T)2;
    const T c = cos(th), sn = sin(th);
    const T zx = r * c, zy = r * sn;
    const T dr = (i == 0 ? y0 : y1) / r;
    const T dth = i == 0 ? -y1 / (r * r) + y0 / ((T)2 * r) : y0 / (r * r) + y1 / ((T)2 * r);
    g = -zx / (s0 * s0) * (dr * c - r * sn * dth) - zy / (s1 * s1) * (dr * sn + r * c * dth) + dr / r;
    if (i != 0) return (T)0;
    return (T)-0.5 * (zx * zx / (s0 * s0) + zy * zy / (s1 * s1)) - L2PI - log(s0) - log(s1) + log(r);
  }
  // CROSS: equal-weight mixture of 4 diagonal Gaussians
  const T mx[4] = {(T)0, -s0, s0, (T)0}, my[4] = {s0, (T)1, (T)1, -s0};
  const T sx[4] = {s1, (T)1, (T)1, s1}, sy[4] = {(T)1, s1, s1, (T)1};
  T lg[4], m = (T)-1e300;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const T a = (y0 - mx[k]) / sx[k], b = (y1 - my[k]) / sy[k];
    lg[k] = -L2PI - log(sx[k]) - log(sy[k]) - (T)0.5 * (a * a + b * b);
    m = lg[k] > m ? lg[k] : m;
  }
  T sw = 0, gw = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const T w = exp(lg[k] - m);
    sw += w;
    gw += w * (i == 0 ? -(y0 - mx[k]) / (sx[k] * sx[k]) : -(y1 - my[k]) / (sy[k] * sy[k]));
  }
  g = gw / sw;
  if (i != 0) return (T)0;
  return log((T)0.25) + m + log(sw);
}

// Sets of kinds one kernel instantiation serves.  Two users: the chain bodies' template argument TGT (nf_target_epilogue.h,
// nf_coupling.hip, nf_rqs.hip) holds the four non-Gaussian bits only, and TGT == 0 there means the diagonal-Gaussian kernel;
// nf_with_target_kind's KSET may hold NF_TGT_DIAG as well (NF_TGT_ALL5: every kind behind one dispatch).
#define NF_TGT_BANANA 1
#define NF_TGT_FUNNEL 2
#define NF_TGT_WARPED 4
#define NF_TGT_CROSS 8
#define NF_TGT_ALL4 15
#define NF_TGT_DIAG 16
#define NF_TGT_ALL5 31
constexpr int nf_tgt_bit(int kind) {
  return kind == NF_TARGET_DIAGGAUSS ? NF_TGT_DIAG : kind == NF_TARGET_BANANA ? NF_TGT_BANANA : kind == NF_TARGET_FUNNEL ? NF_TGT_FUNNEL
         : kind == NF_TARGET_WARPED ? NF_TGT_WARPED : NF_TGT_CROSS;
}
constexpr int nf_tgt_last(int kset) {  // the set's last member in the order DiagGauss, Banana, Funnel, WarpedGauss, Cross
  return kset & NF_TGT_CROSS ? NF_TARGET_CROSS : kset & NF_TGT_WARPED ? NF_TARGET_WARPED : kset & NF_TGT_FUNNEL ? NF_TARGET_FUNNEL
         : kset & NF_TGT_BANANA ? NF_TARGET_BANANA : NF_TARGET_DIAGGAUSS;
}

// Calls f(std::integral_constant<int, KIND>{}) for the run-time `kind` (wave-uniform), so that f's body is compiled once per
// kind with the kind a constant.  KSET leaves arms out: `kind` must be a member -- the host launches nothing else -- and every
// value without an arm of its own takes the set's last member's (with all five: Cross, the `default:` this replaces).
template <int KSET = NF_TGT_ALL5, class F>
__device__ __forceinline__ void nf_with_target_kind(int kind, F &&f) {
  constexpr int LAST = nf_tgt_last(KSET);
#define NF_TGT_ARM(K) \
  case K:             \
    if constexpr ((KSET & nf_tgt_bit(K)) && K != LAST) return f(std::integral_constant<int, K>{}); \
    break;
  switch (kind) {
    NF_TGT_ARM(NF_TARGET_DIAGGAUSS)
    NF_TGT_ARM(NF_TARGET_BANANA)
    NF_TGT_ARM(NF_TARGET_FUNNEL)
    NF_TGT_ARM(NF_TARGET_WARPED)
    default: break;
  }
#undef NF_TGT_ARM
  f(std::integral_constant<int, LAST>{});
}
__host__ __device__ inline bool target_needs_d2(int kind) { return kind == NF_TARGET_WARPED || kind == NF_TARGET_CROSS; }
// The linear-predictor kinds (NF_TARGET_DENSEGAUSS, NF_TARGET_LOGREG) couple every feature with every other through a
// matrix: target_term cannot express them.  They have kernels of their own (nf_linpred.hip), reached through
// nf_launch_target / nf_launch_target_tiled; every path that evaluates target_term inside a fused kernel refuses them.
// The generalised kinds (NF_TARGET_GLM_LOGIT .. NF_TARGET_GLM_NORMAL: row offsets, row weights, a linear term and a family
// parameter) are linear-predictor kinds served by the same two kernels.
__host__ __device__ inline bool target_is_glm(int kind) { return kind >= NF_TARGET_GLM_LOGIT && kind <= NF_TARGET_GLM_NORMAL; }
// The hierarchical kinds (NF_TARGET_HGLM_LOGIT .. NF_TARGET_HGLM_NORMAL = the GLM kind + 7: the generalised form under a
// structured prior with learned group scales) are linear-predictor kinds too, served by a third form of the same two bodies.
__host__ __device__ inline bool target_is_hglm(int kind) { return kind >= NF_TARGET_HGLM_LOGIT && kind <= NF_TARGET_HGLM_NORMAL; }
// The dispersion kinds (NF_TARGET_DGLM_NORMAL / STUDENT / NEGBIN: the hierarchical form with one more coordinate, the
// log-dispersion lambda = y[d - 1], inside the row function) are linear-predictor kinds too: the fourth form of the two bodies.
__host__ __device__ inline bool target_is_dglm(int kind) { return kind >= NF_TARGET_DGLM_NORMAL && kind <= NF_TARGET_DGLM_NEGBIN; }
__host__ __device__ inline bool target_is_linpred(int kind) {
  return kind == NF_TARGET_DENSEGAUSS || kind == NF_TARGET_LOGREG || target_is_glm(kind) || target_is_hglm(kind) || target_is_dglm(kind);
}
// The Gaussian mixture (NF_TARGET_GAUSSMIX, nf_mixture.hip) is routed like them: a kernel of its own behind
// nf_launch_target / nf_launch_target_tiled, refused wherever target_term would have to evaluate it.
// So is the softmax regression target (NF_TARGET_SOFTMAX, nf_softmax.hip): C predictors per data row, coupled through a
// log-sum-exp, which the one-function-per-row form of the linear-predictor kernels cannot express.
// So are the one-hidden-layer Bayesian neural-network kinds (NF_TARGET_BNN_LOGIT .. NF_TARGET_BNN_NORMAL = the GLM kind + 13,
// nf_bnn.hip): some coordinates of y are per-sample scalars (the output weights and bias), not rows of a matrix product.
__host__ __device__ inline bool target_is_bnn(int kind) { return kind >= NF_TARGET_BNN_LOGIT && kind <= NF_TARGET_BNN_NORMAL; }
// So is the ordinal (cumulative-logit) kind (NF_TARGET_ORDINAL_LOGIT, nf_ordinal.hip): the cutpoints are coordinates of y, and a
// row's term depends on two of them, chosen by the label of its 32-row block.
__host__ __device__ inline bool target_is_ordinal(int kind) { return kind == NF_TARGET_ORDINAL_LOGIT; }
// So is the risk-set kind (NF_TARGET_RISKSET, nf_riskset.hip): the first target whose rows interact -- a row's term is a log-sum-exp
// over the rows before it in its segment, so a scan over the rows sits between the two matrix products.
__host__ __device__ inline bool target_is_riskset(int kind) { return kind == NF_TARGET_RISKSET; }
__host__ __device__ inline bool target_has_own_kernel(int kind) {
  return target_is_linpred(kind) || kind == NF_TARGET_GAUSSMIX || kind == NF_TARGET_SOFTMAX || target_is_bnn(kind) || target_is_ordinal(kind) ||
         target_is_riskset(kind);
}
// widest flow the mixture's tiled kernel serves (two U and two G blocks in registers); the flat kernel goes to 256
#define NF_MIXTURE_TILED_MAXD 64
