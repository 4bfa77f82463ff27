// nf_linpred.h -- the row functions and the row data of the linear-predictor targets (nf_linpred.hip).
//
// A linear-predictor target is a sum of ONE scalar function over the rows of a matrix product plus a prior.  Four
// forms share the kernels:
//   centred (kinds 5, 6)   log p(y) = c + sum_i phi(u_i) - pw |y|^2 / 2,   u = A (y - mu),   grad = A' phi'(u) - pw y
//     DENSEGAUSS  phi(u) = -u^2 / 2        c = -d/2 log(2 pi) + log|det W|     pw = 0           (A = W = inv(L))
//     LOGREG      phi(u) = log sigmoid(u)  c = -d/2 log(2 pi sigma^2)          pw = 1 / sigma^2 (A_i = t_i x_i)
//   generalised (kinds 9..13, NF_TARGET_GLM_*)
//                          log p(y) = par[1] + c + sum_i wt_i phi(u_i; par[0]) + lin . y - pw |y|^2 / 2,   u = A y + off,
//                          grad = A' (wt o phi'(u)) + lin - pw y,   c = -d/2 log(2 pi sigma^2), pw = 1 / sigma^2 (both 0
//                          for the flat prior sigma = +inf), with the row data in ONE device buffer
//                          p0 = lin[d] | off[rows] | wt[rows] | par[2]   (GlmRows below).
//     LOGIT log sigmoid(u) | PROBIT log Phi(u) | POISSON -exp(u) | STUDENT -(nu + 1)/2 log1p(u^2 / nu) | NORMAL -u^2 / 2
//   hierarchical (kinds 16..20, NF_TARGET_HGLM_* = the GLM kind + 7)
//                          the generalised form over y = [beta (p) ; tau (G)] with the structured prior of HierRows below in
//                          place of the isotropic one (c = pw = 0; s1 = G), its data behind par[2] in the same buffer.
//   dispersion (kinds 29..31, NF_TARGET_DGLM_*)
//                          the hierarchical form over y = [beta (p) ; tau (G) ; lambda] with a learned log-dispersion lambda =
//                          y[d - 1] INSIDE the row function (DispScale / DispNegBin below): phi_i(u_i, lambda), a hyper-prior
//                          h_G on exp(lambda) and, for the negative binomial, the table term T(lambda) (DispRows below).
// A row function returns phi(u; par) and phi'(u; par) of ONE element; both target kernels are templated on it and on the
// form (LP_CENTRED / LP_GLM / LP_HIER / LP_DISP: the centred instantiations compile the row data away).  par is the family parameter par[0], read once per
// launch (nu for STUDENT; the other families ignore it).  A row of weight 0 contributes exactly 0 by SELECT, whatever phi
// returns there (a subsampling mask may sit over a row whose phi overflows); nothing is clamped.
#pragma once
#include "nf_common.h"
#include "nf_mfma.h"
#include "nf_targets.h"

struct PhiHalfSquare {  // -u^2 / 2 ; -u
  template <class T>
  static __device__ __forceinline__ void eval(T u, T, T &phi, T &dphi) {
    phi = (T)-0.5 * u * u;
    dphi = -u;
  }
};

// log sigmoid(u) = min(u, 0) - log1p(exp(-|u|)) ; sigmoid(-u).  e = exp(-|u|) is in (0, 1]: nothing overflows for any finite u.
struct PhiLogSigmoid {
  static __device__ __forceinline__ void eval(double u, double, double &phi, double &dphi) {
    const double e = exp(-fabs(u));
    phi = fmin(u, 0.0) - log1p(e);
    dphi = (u >= 0.0 ? e : 1.0) / (1.0 + e);
  }
  // float: the hardware exponential and logarithm (1 ulp each).  1 + e is in (1, 2], so log(1 + e) has an ABSOLUTE error of
  // at most one float ulp of 1 -- of the size of the rounding of the sum the term is added to.
  static __device__ __forceinline__ void eval(float u, float, float &phi, float &dphi) {
    const float e = nf_exp(-fabsf(u));
    const float s = 1.f + e;
    phi = fminf(u, 0.f) - nf_log(s);
    dphi = nf_fdiv(u >= 0.f ? e : 1.f, s);
  }
};

// the library's own transcendentals by element type (erfcx has no float overload to resolve to: it would promote to double)
__device__ __forceinline__ float lp_exp(float x) { return expf(x); }
__device__ __forceinline__ double lp_exp(double x) { return exp(x); }
__device__ __forceinline__ float lp_log(float x) { return logf(x); }
__device__ __forceinline__ double lp_log(double x) { return log(x); }
__device__ __forceinline__ float lp_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double lp_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float lp_erfc(float x) { return erfcf(x); }
__device__ __forceinline__ double lp_erfc(double x) { return erfc(x); }
__device__ __forceinline__ float lp_erfcx(float x) { return erfcxf(x); }
__device__ __forceinline__ double lp_erfcx(double x) { return erfcx(x); }

// log Phi(u) ; phi_N(u) / Phi(u)  (probit).  The left tail goes through the scaled complementary error function,
// Phi(u) = exp(-u^2 / 2) erfcx(-u / sqrt 2) / 2, so neither the value nor the ratio meets 0 / 0 or log 0:
//   u <  0   log Phi = -u^2 / 2 + log(erfcx(-u / sqrt 2) / 2),   phi' = sqrt(2 / pi) / erfcx(-u / sqrt 2)
//   u >= 0   c = erfc(u / sqrt 2) / 2 in (0, 1/2],   log Phi = log1p(-c),   phi' = phi_N(u) / (1 - c)
// The library's own exp / log / erfc / erfcx (no hardware approximations: the tails are the point of this form).
struct PhiLogNormCdf {
  template <class T>
  static __device__ __forceinline__ void eval(T u, T, T &phi, T &dphi) {
    const T RSQRT2 = (T)0.70710678118654752440, SQRT_2_PI = (T)0.79788456080286535588, RSQRT_2PI = (T)0.39894228040143267794;
    if (u < (T)0) {
      const T t = lp_erfcx(-u * RSQRT2);
      phi = (T)-0.5 * u * u + lp_log((T)0.5 * t);
      dphi = SQRT_2_PI / t;
    } else {
      const T c = (T)0.5 * lp_erfc(u * RSQRT2);
      phi = lp_log1p(-c);
      dphi = RSQRT_2PI * lp_exp((T)-0.5 * u * u) / ((T)1 - c);
    }
  }
};

// -exp(u) ; -exp(u)  (Poisson with the log link; the k u term is linear in y and sits in `lin` / par[1]).  The library's
// expf: the hardware exponential's error grows with |u| (the rounding of u log2 e), and u reaches tens here.  Not clamped:
// a predictor beyond exp's range gives -inf, and the step reports NF_ERR_NONFINITE.
struct PhiNegExp {
  template <class T>
  static __device__ __forceinline__ void eval(T u, T, T &phi, T &dphi) {
    phi = dphi = -lp_exp(u);
  }
};

// -(nu + 1)/2 log1p(u^2 / nu) ; -(nu + 1) u / (nu + u^2)  (Student-t residual u, nu = par > 0)
struct PhiStudent {
  template <class T>
  static __device__ __forceinline__ void eval(T u, T nu, T &phi, T &dphi) {
    const T u2 = u * u;
    phi = (T)-0.5 * (nu + (T)1) * lp_log1p(u2 / nu);
    dphi = -(nu + (T)1) * u / (nu + u2);
  }
};

// The row data of the generalised form, addressed inside the one buffer p0 = lin[d] | off[rows] | wt[rows] | par[2].
template <class T>
struct GlmRows {
  const T *lin, *off, *wt, *par;
  __device__ __forceinline__ GlmRows(const T *p0, int d, int rows) : lin(p0), off(p0 + d), wt(p0 + d + rows), par(p0 + d + 2 * (long)rows) {}
};
// one row's phi and phi' under its weight: exactly 0 for weight 0, by select
template <class T>
__device__ __forceinline__ void glm_weigh(T w, T &phi, T &dphi) {
  phi = w == (T)0 ? (T)0 : w * phi;
  dphi = w == (T)0 ? (T)0 : w * dphi;
}

// The four forms of the two kernel bodies (their template argument FORM).
#define LP_CENTRED 0
#define LP_GLM 1
#define LP_HIER 2
#define LP_DISP 3

// The structured prior of the hierarchical form (NF_TARGET_HGLM_*): y = [beta (p) ; tau (G)], the prior data behind the row
// data in the same buffer,   ... par[2] | grp[p] | isd[p] | hm[G] | his[G] | hk[G] | gptr[G + 1] | gidx[p].
// The host cannot validate device memory, so every index read from the buffer is bounded by SELECT before it addresses
// anything: a garbage buffer gives wrong numbers, never an access outside y's d features or the buffer's own arrays.
template <class T>
struct HierRows {
  const T *grp, *isd, *hm, *his, *hk, *gptr, *gidx;
  int p, G;
  __device__ __forceinline__ HierRows(const T *p0, int d, int rows, int ng) : p(d - ng), G(ng) {
    grp = p0 + d + 2 * (long)rows + 2;
    isd = grp + p;
    hm = isd + p;
    his = hm + G;
    hk = his + G;
    gptr = hk + G;
    gidx = gptr + G + 1;
  }
  // The dispersion form's layout: y = [beta (p) ; tau (G) ; lambda], par[4], and hm / his / hk hold G + 1 entries (entry G is
  // lambda's hyper-prior; it has no member list, so gptr keeps its G + 1 entries).
  struct Disp {};
  __device__ __forceinline__ HierRows(Disp, const T *p0, int d, int rows, int ng) : p(d - ng - 1), G(ng) {
    grp = p0 + d + 2 * (long)rows + 4;
    isd = grp + p;
    hm = isd + p;
    his = hm + G + 1;
    hk = his + G + 1;
    gptr = hk + G + 1;
    gidx = gptr + G + 1;
  }
  template <int FORM>
  static __device__ __forceinline__ HierRows of_form(const T *p0, int d, int rows, int ng) {
    if constexpr (FORM == LP_DISP)
      return HierRows(Disp{}, p0, d, rows, ng);
    else
      return HierRows(p0, d, rows, FORM == LP_HIER ? ng : 0);
  }
  // an integer-valued element as an index of [0, n), or -1 (NaN fails both comparisons)
  static __device__ __forceinline__ int index_in(T v, int n) { return (v >= (T)0 && v < (T)n) ? (int)v : -1; }
  // Coefficient i < p of a sample whose feature f is y(f): the prior's share of log p and of d log p / d beta_i.
  template <class Y>
  __device__ __forceinline__ void coef(int i, T beta, Y &&y, T &val, T &grad) const {
    const int g = index_in(grp[i], G);
    const T sd = isd[i];
    const T om = g < 0 ? sd * sd : lp_exp((T)-2 * y(p + g));
    grad = -beta * om;
    val = (T)-0.5 * (beta * beta) * om;
  }
  // Log-scale g < G, tau = y(p + g): the hyper-prior h_g and the members' beta^2 exp(-2 tau), summed in list order.
  template <class Y>
  __device__ __forceinline__ void scale(int g, T tau, Y &&y, T &val, T &grad) const {
    const T a = gptr[g], b = gptr[g + 1];
    const int lo = a >= (T)0 ? (a <= (T)p ? (int)a : p) : 0, hi = b >= (T)0 ? (b <= (T)p ? (int)b : p) : 0;  // clamped to [0, p]; NaN -> 0
    T ss = 0;
    for (int k = lo; k < hi; ++k) {
      const int j = index_in(gidx[k], p);
      const T bj = y(j < 0 ? 0 : j);
      ss += j < 0 ? (T)0 : bj * bj;
    }
    const T x = tau - hm[g], kind = hk[g];
    T hv, hd;
    if (kind == (T)0) {
      const T s = his[g], z = x * s;
      hv = (T)-0.5 * z * z;
      hd = -z * s;
    } else if (kind == (T)1) {
      const T e = lp_exp((T)2 * x);
      hv = (T)-0.5 * e;
      hd = -e;
    } else {  // -softplus(2 x) = log sigmoid(-2 x) ; -2 sigmoid(2 x): the exp(-|.|) forms of the logit row function
      T dp;
      PhiLogSigmoid::eval((T)-2 * x, (T)0, hv, dp);
      hd = (T)-2 * dp;
    }
    val = hv;
    grad = ss * lp_exp((T)-2 * tau) + hd;
  }
  // Hyper-prior entry g alone at the log-scale t: h_g(t - hm_g) and its derivative, the three forms of `scale` (the dispersion
  // form's lambda, entry G, which has no member list).  `scale` keeps its own copy: routing it through this function changes
  // the shipped hierarchical kernels' register allocation, and they keep their instruction streams.
  __device__ __forceinline__ void hyper(int g, T t, T &hv, T &hd) const {
    const T x = t - hm[g], kind = hk[g];
    if (kind == (T)0) {
      const T s = his[g], z = x * s;
      hv = (T)-0.5 * z * z;
      hd = -z * s;
    } else if (kind == (T)1) {
      const T e = lp_exp((T)2 * x);
      hv = (T)-0.5 * e;
      hd = -e;
    } else {  // -softplus(2 x) = log sigmoid(-2 x) ; -2 sigmoid(2 x): the exp(-|.|) forms of the logit row function
      T dp;
      PhiLogSigmoid::eval((T)-2 * x, (T)0, hv, dp);
      hd = (T)-2 * dp;
    }
  }
};

// The row functions of the dispersion form (NF_TARGET_DGLM_*).  lambda = y[d - 1] is a per-sample scalar: `Lane` holds what a
// lane derives from it ONCE per tile (every row a lane evaluates belongs to one sample).  eval returns phi, d phi / d u and
// d phi / d lambda of one row; k is the row's count (read only where COUNTS).
//   DispScale<PHI>  z = u exp(-lambda):  phi_fam(z; par) ;  exp(-lambda) phi'(z) ;  -phi'(z) z      (NORMAL, STUDENT)
//   DispNegBin      x = u - lambda, r = exp(lambda):  -(k + r) softplus(x) ;  -(k + r) sigmoid(x) ;  -r softplus(x) + (k + r) sigmoid(x)
// softplus and sigmoid are the exp(-|x|) forms of PhiLogSigmoid (log sigmoid(-x) = -softplus(x)); exp(+-lambda) is the library's
// exponential (once per lane per tile: its cost does not show, and the hardware one's error grows with |lambda|).  Nothing is clamped.
template <class T>
struct DispLane {
  T lam, einv, el;  // lambda, exp(-lambda), exp(lambda)
};
template <class PHI>
struct DispScale {
  static constexpr bool COUNTS = false;
  template <class T>
  static __device__ __forceinline__ DispLane<T> lane(T lam) {
    return {lam, lp_exp(-lam), (T)0};
  }
  template <class T>
  static __device__ __forceinline__ void eval(T u, T, T par, const DispLane<T> &L, T &phi, T &du, T &dl) {
    const T z = u * L.einv;
    T dz;
    PHI::eval(z, par, phi, dz);
    du = L.einv * dz;
    dl = -dz * z;
  }
};
struct DispNegBin {
  static constexpr bool COUNTS = true;
  template <class T>
  static __device__ __forceinline__ DispLane<T> lane(T lam) {
    return {lam, lp_exp(-lam), lp_exp(lam)};
  }
  template <class T>
  static __device__ __forceinline__ void eval(T u, T k, T, const DispLane<T> &L, T &phi, T &du, T &dl) {
    T nsp, sg;  // -softplus(x), sigmoid(x)
    PhiLogSigmoid::eval(L.lam - u, (T)0, nsp, sg);
    const T kr = k + L.el;
    phi = kr * nsp;
    du = -kr * sg;
    dl = L.el * nsp + kr * sg;
  }
};
// phi, d phi / d u and d phi / d lambda of one row under its weight: exactly 0 for weight 0, by select
template <class T>
__device__ __forceinline__ void disp_weigh(T w, T &phi, T &du, T &dl) {
  glm_weigh(w, phi, du);
  dl = w == (T)0 ? (T)0 : w * dl;
}

// The data of the dispersion form behind the structured prior's, in the same buffer:  ... gidx[p] | cnt[rows] | ctab[Mt]
// (NEGBIN only), Mt = par[2] clamped to [0, 4096] by select (NaN -> 0), ctab[j] = c_{j + 1}.  The table term
//   T(lambda) = sum_j ctab[j] log1p((j + 1) exp(-lambda)),   T'(lambda) = -sum_j ctab[j] (j + 1) / (exp(lambda) + j + 1)
// is summed by `nth` threads of a sample: thread `th` takes j = th, th + nth, ... ascending.
#define LP_DISP_MAXTAB 4096
template <class T>
struct DispRows {
  const T *cnt, *ctab;
  int Mt;
  __device__ __forceinline__ DispRows(const HierRows<T> &hr, const T *par, int rows, bool counts) {
    cnt = hr.gidx + hr.p;
    ctab = cnt + rows;
    const T m = counts ? par[2] : (T)0;
    Mt = m >= (T)0 ? (m <= (T)LP_DISP_MAXTAB ? (int)m : LP_DISP_MAXTAB) : 0;
  }
  __device__ __forceinline__ void table(int th, int nth, const DispLane<T> &L, T &tv, T &td) const {
    tv = (T)0, td = (T)0;
    for (int j = th; j < Mt; j += nth) {
      const T m = (T)(j + 1), c = ctab[j];
      tv += c * lp_log1p(m * L.einv);
      td -= c * m / (L.el + m);
    }
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
  if (target_is_glm(t->kind) && std::isinf(t->s1)) return {0.0, 0.0, (long)t->s0};  // flat prior: both prior terms vanish
  if (target_is_hglm(t->kind) || target_is_dglm(t->kind)) return {0.0, 0.0, (long)t->s0};  // s1 = G: the prior is evaluated from the buffer, its constants sit in par[1]
  return {-0.5 * d * (L2PI + 2.0 * std::log(t->s1)), 1.0 / (t->s1 * t->s1), (long)t->s0};
}
