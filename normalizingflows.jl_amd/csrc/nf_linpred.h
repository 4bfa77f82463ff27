// nf_linpred.h -- the row functions of the linear-predictor targets (nf_linpred.hip).
//
// A linear-predictor target is  log p(y) = c + sum_i phi(u_i) - pw |y|^2 / 2,  u = A (y - mu),  with gradient
// A' phi'(u) - pw y.  The two built-in kinds differ in phi, in the constant c and in the prior weight pw only:
//   DENSEGAUSS  phi(u) = -u^2 / 2        c = -d/2 log(2 pi) + log|det W|     pw = 0           (A = W = inv(L))
//   LOGREG      phi(u) = log sigmoid(u)  c = -d/2 log(2 pi sigma^2)          pw = 1 / sigma^2 (A_i = t_i x_i)
// A row function returns phi(u) and phi'(u) of ONE element; both target kernels are templated on it.
#pragma once
#include "nf_common.h"
#include "nf_mfma.h"
#include "nf_targets.h"

struct PhiHalfSquare {  // -u^2 / 2 ; -u
  template <class T>
  static __device__ __forceinline__ void eval(T u, T &phi, T &dphi) {
    phi = (T)-0.5 * u * u;
    dphi = -u;
  }
};

// log sigmoid(u) = min(u, 0) - log1p(exp(-|u|)) ; sigmoid(-u).  e = exp(-|u|) is in (0, 1]: nothing overflows for any finite u.
struct PhiLogSigmoid {
  static __device__ __forceinline__ void eval(double u, double &phi, double &dphi) {
    const double e = exp(-fabs(u));
    phi = fmin(u, 0.0) - log1p(e);
    dphi = (u >= 0.0 ? e : 1.0) / (1.0 + e);
  }
  // float: the hardware exponential and logarithm (1 ulp each).  1 + e is in (1, 2], so log(1 + e) has an ABSOLUTE error of
  // at most one float ulp of 1 -- of the size of the rounding of the sum the term is added to.
  static __device__ __forceinline__ void eval(float u, float &phi, float &dphi) {
    const float e = nf_exp(-fabsf(u));
    const float s = 1.f + e;
    phi = fminf(u, 0.f) - nf_log(s);
    dphi = nf_fdiv(u >= 0.f ? e : 1.f, s);
  }
};

// the constant and the prior weight of a checked target (host side, in double)
struct LinpredConsts {
  double c, pw;
  long rows;
};
inline LinpredConsts linpred_consts(const nf_target *t, int d) {
  const double L2PI = 1.8378770664093453;
  if (t->kind == NF_TARGET_DENSEGAUSS) return {-0.5 * d * L2PI + t->s0, 0.0, (long)d};
  return {-0.5 * d * (L2PI + 2.0 * std::log(t->s1)), 1.0 / (t->s1 * t->s1), (long)t->s0};
}
