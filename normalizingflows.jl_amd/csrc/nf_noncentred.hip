// nf_noncentred.hip -- the layer S of NF_KIND_NONCENTRED (gfx950): over z = [beta (p) ; tau (G) (; lambda)], the layout of the
// hierarchical (NF_TARGET_HGLM_*) and dispersion (NF_TARGET_DGLM_*) targets,
//   y_j = z_j exp(lam_j tau_g(j))  for j < p with g(j) = grp[j] >= 0,   y_j = z_j  for every other coordinate,
//   ladj = sum_{j: g(j) >= 0} lam_j tau_g(j)  in increasing j;   inverse: z_j = y_j exp(-lam_j tau_g(j)), ladj_inv = -ladj
// (tau passes through, so both directions read it from their own input).  lam (p, trainable) is the layer's theta: 0 = centred,
// 1 = non-centred.  grp comes from the target's device buffer p0 through HierRows (nf_linpred.h): the layouts of both forms, and
// every index bounded by select before it addresses anything -- a garbage buffer gives wrong numbers, never an access outside the
// d features.  The lam_j of a coefficient with g(j) < 0 belongs to theta and is never used: masked by select, so NaN there
// changes no output bit and its gradient is exactly 0.0 (nf_fullrank.hip's upper-triangle rule).
// Pullback for cotangents ybar, lbar, with a_j = ybar_j y_j + lbar:
//   zbar_j = ybar_j exp(lam_j tau_g(j)),   taubar_g = ybar_{p+g} + lam_j a_j over the members j of g in increasing j,
//   lambar_j = sum_samples tau_g(j) a_j.
// The exponential is the library's (lp_exp), not the hardware approximation: |lam tau| reaches tens on a funnel.
//
// Float32, tiled layout ([feature][32 samples] per tile, nf_elementwise.hip), four samples per lane and access:
//   k_nc_fwd_tiled   one workgroup per tile, out of place: the input tile stays intact as the tape of the inner flow's reverse
//                    pass.  The terms lam_j tau_g(j) go through LDS so that one lane per sample adds them in increasing j.
//   k_nc_bwd_tiled   grid-stride over tiles on at most one workgroup per compute unit (nf_fr_bwd_grid): zbar in place over ybar
//                    (a thread's whole share of the tile is staged in registers before anything is written), the taubar rows,
//                    lambar in registers across the workgroup's tiles, one slab per workgroup reduced in block order by
//                    nf_launch_reduce_slabs.  y is the forward's own output, read back, never re-derived.  No atomics.
// Both element types, standard layout (the general path): one thread per sample for forward / inverse (k_nc_apply_flat) and
// for the cotangent (k_nc_pull_flat), one thread per parameter and sample chunk for lambar (k_nc_grad_flat); their y is the
// forward's arithmetic run again from z in the element type, hence the same bits.
#include "nf_common.h"
#include "nf_launchers.h"
#include "nf_linpred.h"

#define NC_BLOCK 256
#define NC_MAXD 256  // widest tiled batch (the tiled inner flows stop there too)

// group of coefficient j, or -1; lam_j where it is used, 0 where it is not (by select: whatever theta holds there)
template <class T>
struct NcCoef {
  int g;
  T lam;
};
template <class T>
__device__ __forceinline__ NcCoef<T> nc_coef(const HierRows<T> &hr, const T *__restrict__ lam, int j) {
  const int g = HierRows<T>::index_in(hr.grp[j], hr.G);
  const T l = lam[j];
  return {g, g < 0 ? (T)0 : l};
}

// the feature that holds tau_g; feature 0 for a coefficient without a group (its value is read and dropped by select), so that
// the address stays inside the d features whatever G is (G = 0: there is no feature p)
__device__ __forceinline__ int nc_tau_row(int p, int g) { return g < 0 ? 0 : p + g; }

__device__ __forceinline__ float4 nc_ld4(const float *p, long n0, int s0, long N) {
  float4 v = *reinterpret_cast<const float4 *>(p);
  v.x = n0 + s0 + 0 < N ? v.x : 0.f;
  v.y = n0 + s0 + 1 < N ? v.y : 0.f;
  v.z = n0 + s0 + 2 < N ? v.z : 0.f;
  v.w = n0 + s0 + 3 < N ? v.w : 0.f;
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Float32, tiled
// ---------------------------------------------------------------------------------------------------------------------
template <int FORM>
__global__ __launch_bounds__(NC_BLOCK) void k_nc_fwd_tiled(int d, long N, int rows, int G, const float *__restrict__ p0,
                                                           const float *__restrict__ lam, float sign, const float *__restrict__ in,
                                                           float *__restrict__ out, float *__restrict__ ladj) {
  extern __shared__ float sC[];  // [p][32]: lam_j tau_g(j), 0 for a coefficient without a group
  const HierRows<float> hr = HierRows<float>::template of_form<FORM>(p0, d, rows, G);
  const int p = hr.p;
  const long tile = blockIdx.x, n0 = tile * 32;
  const float *src = in + tile * d * 32;
  float *dst = out + tile * d * 32;
  for (int q = threadIdx.x; q < d * 8; q += NC_BLOCK) {
    const int f = q >> 3, s0 = (q & 7) * 4;
    float4 v = nc_ld4(src + f * 32 + s0, n0, s0, N);
    if (f < p) {
      const NcCoef<float> c = nc_coef(hr, lam, f);
      const float4 t = nc_ld4(src + nc_tau_row(p, c.g) * 32 + s0, n0, s0, N);
      const float4 a = {c.lam * t.x, c.lam * t.y, c.lam * t.z, c.lam * t.w};
      if (c.g >= 0) {
        v.x *= lp_exp(sign * a.x);
        v.y *= lp_exp(sign * a.y);
        v.z *= lp_exp(sign * a.z);
        v.w *= lp_exp(sign * a.w);
      }
      *reinterpret_cast<float4 *>(sC + f * 32 + s0) = c.g < 0 ? float4{0.f, 0.f, 0.f, 0.f} : a;
    }
    *reinterpret_cast<float4 *>(dst + f * 32 + s0) = v;
  }
  __syncthreads();
  if (threadIdx.x < 32 && n0 + threadIdx.x < N) {
    float a = 0.f;
    for (int j = 0; j < p; ++j) a += sC[j * 32 + threadIdx.x];
    ladj[n0 + threadIdx.x] = sign * a;
  }
}

// DB = feature blocks of 32: a thread owns the float4 at position threadIdx.x + k NC_BLOCK of the tile, k < DB, i.e. four
// samples of feature (threadIdx.x >> 3) + 32 k in every tile it visits.
template <int FORM, int DB>
__global__ __launch_bounds__(NC_BLOCK) void k_nc_bwd_tiled(int d, long N, long ntiles, int rows, int G, const float *__restrict__ p0,
                                                           const float *__restrict__ lam, const float *__restrict__ y, float *gt,
                                                           const float *__restrict__ lbar, float lbar_const,
                                                           float *__restrict__ slab) {
  extern __shared__ float sU[];  // [p][32]: lam_j a_j (0 without a group), then the p group indices
  const HierRows<float> hr = HierRows<float>::template of_form<FORM>(p0, d, rows, G);
  const int p = hr.p;
  int *sG = reinterpret_cast<int *>(sU + p * 32);
  for (int j = threadIdx.x; j < p; j += NC_BLOCK) sG[j] = HierRows<float>::index_in(hr.grp[j], G);
  const int s0 = (threadIdx.x & 7) * 4;
  float glam[DB];
#pragma unroll
  for (int k = 0; k < DB; ++k) glam[k] = 0.f;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long n0 = tile * 32;
    const float *yt = y + tile * d * 32;
    float *g = gt + tile * d * 32;
    float4 lb;
    if (lbar) {
      lb = {n0 + s0 + 0 < N ? lbar[n0 + s0 + 0] : 0.f, n0 + s0 + 1 < N ? lbar[n0 + s0 + 1] : 0.f,
            n0 + s0 + 2 < N ? lbar[n0 + s0 + 2] : 0.f, n0 + s0 + 3 < N ? lbar[n0 + s0 + 3] : 0.f};
    } else {
      lb = {n0 + s0 + 0 < N ? lbar_const : 0.f, n0 + s0 + 1 < N ? lbar_const : 0.f, n0 + s0 + 2 < N ? lbar_const : 0.f,
            n0 + s0 + 3 < N ? lbar_const : 0.f};
    }
    float4 zb[DB];
#pragma unroll
    for (int k = 0; k < DB; ++k) {
      const int f = (threadIdx.x >> 3) + 32 * k;
      if (f < p) {
        const NcCoef<float> c = nc_coef(hr, lam, f);
        const float4 gb = nc_ld4(g + f * 32 + s0, n0, s0, N), yv = nc_ld4(yt + f * 32 + s0, n0, s0, N);
        const float4 t = nc_ld4(yt + nc_tau_row(p, c.g) * 32 + s0, n0, s0, N);
        const float4 a = {gb.x * yv.x + lb.x, gb.y * yv.y + lb.y, gb.z * yv.z + lb.z, gb.w * yv.w + lb.w};
        const bool mem = c.g >= 0;
        zb[k] = mem ? float4{gb.x * lp_exp(c.lam * t.x), gb.y * lp_exp(c.lam * t.y), gb.z * lp_exp(c.lam * t.z),
                            gb.w * lp_exp(c.lam * t.w)}
                   : gb;
        *reinterpret_cast<float4 *>(sU + f * 32 + s0) =
            mem ? float4{c.lam * a.x, c.lam * a.y, c.lam * a.z, c.lam * a.w} : float4{0.f, 0.f, 0.f, 0.f};
        // samples beyond N: tau and a are 0 there (the loads' select), so they add exactly 0
        glam[k] += mem ? ((t.x * a.x + t.y * a.y) + (t.z * a.z + t.w * a.w)) : 0.f;
      }
    }
    __syncthreads();  // every thread has read its share of the coefficient rows, and sU is complete
#pragma unroll
    for (int k = 0; k < DB; ++k) {
      const int f = (threadIdx.x >> 3) + 32 * k;
      if (f < p) *reinterpret_cast<float4 *>(g + f * 32 + s0) = zb[k];
    }
    // the taubar rows: lane s of lane group w takes the groups w, w + 8, ... (one reader and one writer per element)
    const int s = threadIdx.x & 31;
    for (int gi = threadIdx.x >> 5; gi < G; gi += NC_BLOCK / 32) {
      float a = n0 + s < N ? g[(p + gi) * 32 + s] : 0.f;
      for (int j = 0; j < p; ++j) a += sG[j] == gi ? sU[j * 32 + s] : 0.f;
      g[(p + gi) * 32 + s] = a;
    }
    __syncthreads();  // sU is rewritten by the next tile
  }
  if (!slab) return;
#pragma unroll
  for (int k = 0; k < DB; ++k) {
    float a = glam[k];
    a += __shfl_xor(a, 1, 8);
    a += __shfl_xor(a, 2, 8);
    a += __shfl_xor(a, 4, 8);
    const int f = (threadIdx.x >> 3) + 32 * k;
    if ((threadIdx.x & 7) == 0 && f < p) slab[(long)blockIdx.x * p + f] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// standard layout, either element type
// ---------------------------------------------------------------------------------------------------------------------
// out may alias in: the tau coordinates are copied onto themselves
template <class T, int FORM>
__global__ __launch_bounds__(NC_BLOCK) void k_nc_apply_flat(int d, long N, int rows, int G, const T *__restrict__ p0,
                                                            const T *__restrict__ lam, T sign, const T *in, T *out,
                                                            T *__restrict__ ladj) {
  const HierRows<T> hr = HierRows<T>::template of_form<FORM>(p0, d, rows, G);
  const int p = hr.p;
  const long n = (long)blockIdx.x * NC_BLOCK + threadIdx.x;
  if (n >= N) return;
  const T *x = in + n * d;
  T *yo = out + n * d;
  T a = 0;
  for (int j = 0; j < p; ++j) {
    const NcCoef<T> c = nc_coef(hr, lam, j);
    const T t = x[nc_tau_row(p, c.g)], v = x[j];
    const T lt = c.lam * t;
    a += c.g < 0 ? (T)0 : lt;
    yo[j] = c.g < 0 ? v : v * lp_exp(sign * lt);
  }
  for (int j = p; j < d; ++j) yo[j] = x[j];
  ladj[n] = sign * a;
}

// xbar from the layer's input x and ybar; xbar may alias ybar (a thread reads each element of its sample before it writes it)
template <class T, int FORM>
__global__ __launch_bounds__(NC_BLOCK) void k_nc_pull_flat(int d, long N, int rows, int G, const T *__restrict__ p0,
                                                           const T *__restrict__ lam, const T *__restrict__ xin, const T *ybar,
                                                           const T *__restrict__ lbar, T lbar_const, T *xbar) {
  const HierRows<T> hr = HierRows<T>::template of_form<FORM>(p0, d, rows, G);
  const int p = hr.p;
  const long n = (long)blockIdx.x * NC_BLOCK + threadIdx.x;
  if (n >= N) return;
  const T *x = xin + n * d, *yb = ybar + n * d;
  T *xb = xbar + n * d;
  const T lb = lbar ? lbar[n] : lbar_const;
  for (int j = p; j < d; ++j) xb[j] = yb[j];
  for (int j = 0; j < p; ++j) {
    const NcCoef<T> c = nc_coef(hr, lam, j);
    const T t = x[nc_tau_row(p, c.g)], gb = yb[j];
    const T e = lp_exp(c.lam * t);
    const T yv = c.g < 0 ? x[j] : x[j] * e;
    const T a = gb * yv + lb;
    xb[j] = c.g < 0 ? gb : gb * e;
    if (c.g >= 0) xb[p + c.g] += c.lam * a;
  }
}

// slab[blockIdx.y][j]: lambar_j over the samples of chunk blockIdx.y
template <class T, int FORM>
__global__ __launch_bounds__(NC_BLOCK) void k_nc_grad_flat(int d, long N, long chunk, int rows, int G, const T *__restrict__ p0,
                                                           const T *__restrict__ lam, const T *__restrict__ x,
                                                           const T *__restrict__ ybar, const T *__restrict__ lbar, T lbar_const,
                                                           T *__restrict__ slabs) {
  const HierRows<T> hr = HierRows<T>::template of_form<FORM>(p0, d, rows, G);
  const int p = hr.p;
  const int j = blockIdx.x * NC_BLOCK + threadIdx.x;
  if (j >= p) return;
  const NcCoef<T> c = nc_coef(hr, lam, j);
  const long n0 = (long)blockIdx.y * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
  T acc = 0;
  if (c.g >= 0) {
    for (long n = n0; n < n1; ++n) {
      const T t = x[n * d + p + c.g];
      const T yv = x[n * d + j] * lp_exp(c.lam * t);
      acc += t * (ybar[n * d + j] * yv + (lbar ? lbar[n] : lbar_const));
    }
  }
  slabs[(long)blockIdx.y * p + j] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers.  `desc` is the layer's own descriptor: kind NF_KIND_NONCENTRED without segments, d, dtype, K and score.
// ---------------------------------------------------------------------------------------------------------------------
struct NcShape {
  int p, G, rows;
  bool disp;
  const void *p0;
};
static inline NcShape nc_shape(const nf_flow_desc *desc) {
  const nf_target *t = (const nf_target *)desc->score;
  const bool disp = target_is_dglm(t->kind);
  const int G = (int)t->s1;
  return {desc->d - G - (disp ? 1 : 0), G, (int)t->s0, disp, t->p0};
}

// the layer's parameter count p, or NF_ERR_ARG for a score that is no hierarchical / dispersion target of this dimension
long nf_nc_params(const nf_flow_desc *desc) {
  const nf_target *t = (const nf_target *)desc->score;
  if (!t || !(target_is_hglm(t->kind) || target_is_dglm(t->kind))) return NF_ERR_ARG;
  if (!(t->s1 >= 0 && t->s1 <= (double)desc->d)) return NF_ERR_ARG;
  const long p = nc_shape(desc).p;
  return p >= 1 ? p : NF_ERR_ARG;
}

bool nf_nc_tiled_supported(const nf_flow_desc *desc) { return desc->dtype == NF_DTYPE_F32 && desc->d <= NC_MAXD; }

static inline int nc_flat_slabs(long N) {
  const long n = (N + 63) / 64;
  return (int)(n < 1 ? 1 : n > 64 ? 64 : n);
}

template <class T>
static int nc_apply_flat(nf_ctx *ctx, const nf_flow_desc *desc, bool inverse, const void *theta, const void *x, long N, void *y,
                         void *ladj) {
  const NcShape s = nc_shape(desc);
  const dim3 grid((unsigned)((N + NC_BLOCK - 1) / NC_BLOCK));
  ProfScope ps(ctx, "nc_apply_flat");
  if (s.disp)
    hipLaunchKernelGGL((k_nc_apply_flat<T, LP_DISP>), grid, dim3(NC_BLOCK), 0, ctx->stream, desc->d, N, s.rows, s.G, (const T *)s.p0,
                       (const T *)theta, inverse ? (T)-1 : (T)1, (const T *)x, (T *)y, (T *)ladj);
  else
    hipLaunchKernelGGL((k_nc_apply_flat<T, LP_HIER>), grid, dim3(NC_BLOCK), 0, ctx->stream, desc->d, N, s.rows, s.G, (const T *)s.p0,
                       (const T *)theta, inverse ? (T)-1 : (T)1, (const T *)x, (T *)y, (T *)ladj);
  return (int)hipGetLastError();
}

// forward / inverse in the standard layout; y may alias x; ladj is overwritten
int nf_nc_apply(nf_ctx *ctx, const nf_flow_desc *desc, bool inverse, const void *theta, const void *x, long N, void *y, void *ladj) {
  if (N <= 0) return NF_OK;
  if (desc->dtype == NF_DTYPE_F32) return nc_apply_flat<float>(ctx, desc, inverse, theta, x, N, y, ladj);
  return nc_apply_flat<double>(ctx, desc, inverse, theta, x, N, y, ladj);
}

// the pullback's workspace: the gradient slabs
size_t nf_nc_bwd_ws_bytes(const nf_flow_desc *desc, long N) {
  return carve_bytes((size_t)nc_flat_slabs(N) * (size_t)nc_shape(desc).p * (desc->dtype == NF_DTYPE_F64 ? 8 : 4));
}

template <class T>
static int nc_bwd_flat(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *x, const void *ybar, const void *lbar,
                       double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws) {
  const NcShape s = nc_shape(desc);
  const int d = desc->d;
  if (desc->K == 1) {  // lam frozen
    NF_TRY(nf_launch_fill(ctx, desc->dtype, gtheta_out, s.p, 0.0));
  } else {
    const int ns = nc_flat_slabs(N);
    const long chunk = (N + ns - 1) / ns;
    const dim3 grid((unsigned)((s.p + NC_BLOCK - 1) / NC_BLOCK), (unsigned)ns);
    {
      ProfScope ps(ctx, "nc_grad_flat");
      if (s.disp)
        hipLaunchKernelGGL((k_nc_grad_flat<T, LP_DISP>), grid, dim3(NC_BLOCK), 0, ctx->stream, d, N, chunk, s.rows, s.G, (const T *)s.p0,
                           (const T *)theta, (const T *)x, (const T *)ybar, (const T *)lbar, (T)lbar_const, (T *)ws);
      else
        hipLaunchKernelGGL((k_nc_grad_flat<T, LP_HIER>), grid, dim3(NC_BLOCK), 0, ctx->stream, d, N, chunk, s.rows, s.G, (const T *)s.p0,
                           (const T *)theta, (const T *)x, (const T *)ybar, (const T *)lbar, (T)lbar_const, (T *)ws);
      NF_HIP(hipGetLastError());
    }
    NF_TRY(nf_launch_reduce_slabs(ctx, desc->dtype, ws, ns, s.p, gtheta_out));
  }
  if (!xbar_out) return NF_OK;
  const dim3 grid((unsigned)((N + NC_BLOCK - 1) / NC_BLOCK));
  ProfScope ps(ctx, "nc_pull_flat");
  if (s.disp)
    hipLaunchKernelGGL((k_nc_pull_flat<T, LP_DISP>), grid, dim3(NC_BLOCK), 0, ctx->stream, d, N, s.rows, s.G, (const T *)s.p0,
                       (const T *)theta, (const T *)x, (const T *)ybar, (const T *)lbar, (T)lbar_const, (T *)xbar_out);
  else
    hipLaunchKernelGGL((k_nc_pull_flat<T, LP_HIER>), grid, dim3(NC_BLOCK), 0, ctx->stream, d, N, s.rows, s.G, (const T *)s.p0,
                       (const T *)theta, (const T *)x, (const T *)ybar, (const T *)lbar, (T)lbar_const, (T *)xbar_out);
  return (int)hipGetLastError();
}

// pullback in the standard layout from the layer's input x: gtheta_out[p] (overwritten; exactly 0.0 with K = 1), and xbar_out
// unless NULL (xbar_out may alias ybar: the parameter gradient reads ybar first).  lbar == NULL: every sample's log-det
// cotangent is lbar_const.
int nf_nc_bwd(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *x, const void *ybar, const void *lbar,
              double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws) {
  if (desc->dtype == NF_DTYPE_F32) return nc_bwd_flat<float>(ctx, desc, theta, x, ybar, lbar, lbar_const, N, xbar_out, gtheta_out, ws);
  return nc_bwd_flat<double>(ctx, desc, theta, x, ybar, lbar, lbar_const, N, xbar_out, gtheta_out, ws);
}

// Float32 forward on tiled buffers (the training step): yt = S(xt), ladj = the layer's log-det; yt must not alias xt
int nf_nc_fwd_tiled(nf_ctx *ctx, const nf_flow_desc *desc, const float *lam, const float *xt, long N, float *yt, float *ladj) {
  const NcShape s = nc_shape(desc);
  const dim3 grid((unsigned)((N + 31) / 32));
  const size_t lds = (size_t)s.p * 32 * sizeof(float);
  ProfScope ps(ctx, "nc_fwd");
  if (s.disp)
    hipLaunchKernelGGL(k_nc_fwd_tiled<LP_DISP>, grid, dim3(NC_BLOCK), lds, ctx->stream, desc->d, N, s.rows, s.G, (const float *)s.p0, lam,
                       1.f, xt, yt, ladj);
  else
    hipLaunchKernelGGL(k_nc_fwd_tiled<LP_HIER>, grid, dim3(NC_BLOCK), lds, ctx->stream, desc->d, N, s.rows, s.G, (const float *)s.p0, lam,
                       1.f, xt, yt, ladj);
  return (int)hipGetLastError();
}

template <int FORM>
static int nc_bwd_tiled_form(nf_ctx *ctx, int d, long N, int grid, const NcShape &s, const float *lam, const float *yt, float *gt,
                             const float *lbar, float lbar_const, float *slab) {
  const size_t lds = (size_t)s.p * 33 * sizeof(float);
  const long nt = (N + 31) / 32;
#define NC_BWD(DB)                                                                                                                \
  hipLaunchKernelGGL((k_nc_bwd_tiled<FORM, DB>), dim3((unsigned)grid), dim3(NC_BLOCK), lds, ctx->stream, d, N, nt, s.rows, s.G, \
                     (const float *)s.p0, lam, yt, gt, lbar, lbar_const, slab)
  if (d <= 32) NC_BWD(1);
  else if (d <= 64) NC_BWD(2);
  else if (d <= 128) NC_BWD(4);
  else NC_BWD(8);
#undef NC_BWD
  return (int)hipGetLastError();
}

// floats of gradient slabs of the tiled reverse launch
size_t nf_nc_slab_floats(nf_ctx *ctx, const nf_flow_desc *desc, long N) { return (size_t)nf_fr_bwd_grid(ctx, N) * (size_t)nc_shape(desc).p; }

// The layer's whole reverse pass on tiled buffers in one launch: gt holds ybar on entry and the cotangent of the layer's input
// on exit, yt is the forward's output, glam_out[p] the parameter gradient (exactly 0.0 with K = 1: lam frozen).
int nf_nc_bwd_tiled(nf_ctx *ctx, const nf_flow_desc *desc, const float *lam, const float *yt, float *gt, const float *lbar,
                    float lbar_const, long N, float *slab, float *glam_out) {
  const NcShape s = nc_shape(desc);
  const int grid = nf_fr_bwd_grid(ctx, N);
  const bool frozen = desc->K == 1;
  {
    ProfScope ps(ctx, "nc_bwd");
    if (s.disp) NF_TRY(nc_bwd_tiled_form<LP_DISP>(ctx, desc->d, N, grid, s, lam, yt, gt, lbar, lbar_const, frozen ? nullptr : slab));
    else NF_TRY(nc_bwd_tiled_form<LP_HIER>(ctx, desc->d, N, grid, s, lam, yt, gt, lbar, lbar_const, frozen ? nullptr : slab));
  }
  if (frozen) return nf_launch_fill(ctx, NF_DTYPE_F32, glam_out, s.p, 0.0);
  return nf_launch_reduce_slabs(ctx, NF_DTYPE_F32, slab, grid, s.p, glam_out);
}
