// nf_launchers.h -- every host function that one translation unit of libnfhip.so defines and another calls, declared once,
// grouped by the defining file.  nf_api.hip and every defining file include it, so the compiler checks each definition
// against the declaration its callers see; a default argument stands here and nowhere else.  Host only: no kernel, no
// device function.  (nf_common.h declares the context helpers of nf_api.hip and nf_comm.hip, nf_target_stages.h the twelve
// launchers of the matrix-pipe target files.)
#pragma once
#include "nf_common.h"

// ---- nf_elementwise.hip: base distribution, targets, sums, optimisers, layout ---------------------------------------
int nf_launch_base_sample(nf_ctx *, int, int, long, uint64_t, uint64_t, uint32_t, void *, void *);
int nf_launch_base_logpdf(nf_ctx *, int, int, long, const void *, void *);
int nf_launch_base_unwhiten(nf_ctx *, int dtype, int kind, int d, long N, const void *mu, const void *scale, void *x);
int nf_launch_base_general_logpdf(nf_ctx *, int dtype, int kind, int d, long N, const void *mu, const void *scale, double logdet,
                                  const void *x, void *logq_out, void *corr_out, void *zbuf);
int nf_launch_base_general_score(nf_ctx *, int dtype, int kind, int d, long N, const void *mu, const void *scale, double logdet,
                                 const void *x, void *logq_out, void *score_out, double gscale, void *zbuf);
long nf_target_nblocks(long N);
int nf_launch_target(nf_ctx *, int, const nf_target *, int, long, const void *, const void *, const void *, void *,
                     void *, double, void *, double *, double, int joint_d);
long nf_sum2_nblocks(long N);
int nf_launch_sum2(nf_ctx *, int, long, const void *, const void *, void *, double *, double);
int nf_launch_finish_sum(nf_ctx *, const double *, long, int, double *, float *, double *, unsigned *bump = nullptr);
int nf_launch_reduce_slabs(nf_ctx *, int, const void *, int, long, void *);
long nf_adam_nblocks(long P);
int nf_launch_adam(nf_ctx *, int, void *, const void *, void *, void *, long, double, double, double, double, long,
                   double *);
int nf_launch_sgd(nf_ctx *, int, void *, const void *, void *, long, double, double, double *);
int nf_launch_fill(nf_ctx *, int, void *, long, double);
int nf_launch_base_sample_tiled(nf_ctx *, int d, long N, uint64_t seed, uint64_t off, uint32_t stream, float *xt, float *logq);
int nf_launch_base_logpdf_tiled(nf_ctx *, int d, long N, const float *xt, float *logq);
long nf_target_tiled_nblocks(long N);
int nf_launch_target_tiled(nf_ctx *, const nf_target *, int d, long N, const float *yt, const float *logq,
                           const float *ladj, float *gt, double gscale, float *elbos_out, double *partial, double pscale);
int nf_launch_layout_convert(nf_ctx *, int d, long N, const float *src, float *dst, int to_tiled);
int nf_target_check(const nf_target *t, int d);

// ---- nf_coupling.hip: RealNVP with LDS-resident conditioner nets --------------------------------------------------
bool nf_affine_supported(const nf_flow_desc *desc);
int nf_affine_apply(nf_ctx *, const nf_flow_desc *, int k, bool inverse, const float *theta, const float *x, long N,
                    float *y, float *ladj, int accumulate);
int nf_affine_bwd_grid(nf_ctx *, long N);
int nf_affine_pack(nf_ctx *, const nf_flow_desc *, const float *theta);
int nf_affine_chain(nf_ctx *, const nf_flow_desc *, bool inverse, float *xt, long N, float *ladj, float *stash = nullptr);
long nf_affine_chain_grid(nf_ctx *, long N);
int nf_affine_chain_elbo(nf_ctx *, const nf_flow_desc *, long N, uint64_t seed, uint64_t off, uint32_t stream,
                         const nf_target *target, float *yt, float *gt, double gscale, double *partial,
                         double pscale, float *stash = nullptr, const uint32_t *stream_ptr = nullptr);
long nf_affine_epilogue_blocks(const nf_flow_desc *desc);
bool nf_affine_chain_fkl_ok(const nf_flow_desc *desc);
int nf_affine_chain_fkl(nf_ctx *, const nf_flow_desc *, const float *ys, long N, float *gt, double gscale, double *partial,
                        double pscale, float *stash);
int nf_affine_epilogue(nf_ctx *, const nf_flow_desc *, int mode, const float *slab, int nslab, float *g, const double *lpart,
                       int nlpart, float *theta, float *m, float *v, double lr, double b1, double b2, double eps, unsigned t_val,
                       unsigned *t_ptr, double *gpart);
size_t nf_affine_stash_floats(const nf_flow_desc *desc, long N);
bool nf_affine_stash_pays(const nf_flow_desc *desc);
bool nf_affine_fused_ok(const nf_flow_desc *desc);
int nf_affine_bwd_stashed(nf_ctx *, const nf_flow_desc *, float *stash, float *ybar, const float *lbar, float lbar_const, long N,
                          float *slab, long slab_stride, int grid, bool inv_dir = false, bool no_xbar = false);
long nf_affine_slab_floats(const nf_flow_desc *desc);
int nf_affine_reduce_slabs(nf_ctx *, const nf_flow_desc *, const float *slab, int nslab, float *g,
                           const double *lpart = nullptr, int nlpart = 0, float *lout = nullptr);
int nf_affine_bwd(nf_ctx *, const nf_flow_desc *, int k, const float *theta, float *y, float *ybar, const float *lbar,
                  float lbar_const, long N, float *slab, long slab_stride, int grid);
int nf_affine_bwd_all(nf_ctx *, const nf_flow_desc *, float *y, float *ybar, const float *lbar, float lbar_const, long N,
                      float *slab, long slab_stride, int grid, bool inv_dir = false);
size_t nf_affine_wimg_bytes(const nf_flow_desc *desc);

// ---- nf_deep.hip: resident nets with 1, 3 or 4 hidden layers; to nf_api.hip they are "resident RealNVP flows without a
// stash", so every nf_affine_* entry point hands them over first --------------------------------------------------------
int nf_deep_geo_id(const nf_flow_desc *desc);
int nf_deep_image_floats(const nf_flow_desc *desc);
size_t nf_deep_wimg_bytes(const nf_flow_desc *desc);
long nf_deep_slab_floats(const nf_flow_desc *desc);
int nf_deep_pack(nf_ctx *ctx, const nf_flow_desc *desc, const float *theta);
int nf_deep_reduce_slabs(nf_ctx *ctx, const nf_flow_desc *desc, const float *slab, int nslab, float *g, const double *lpart, int nlpart,
                         float *lout);
int nf_deep_chain(nf_ctx *ctx, const nf_flow_desc *desc, bool inverse, float *xt, long N, float *ladj, int k_only, int accumulate);
int nf_deep_bwd(nf_ctx *ctx, const nf_flow_desc *desc, int k_lo, int k_hi, float *y, float *ybar, const float *lbar, float lbar_const,
                long N, float *slab, long slab_stride, int grid, bool inv_dir);

// ---- nf_wide.hip: RealNVP with conditioner nets streamed from L2, d <= 256, hidden <= 256 ------------------------------
bool nf_wide_supported(const nf_flow_desc *desc);
int nf_wide_pack(nf_ctx *, const nf_flow_desc *, const float *theta);
int nf_wide_apply(nf_ctx *, const nf_flow_desc *, int k, bool inverse, float *xt, long N, float *ladj, int accumulate);
size_t nf_wide_bwd_ws_floats(nf_ctx *, const nf_flow_desc *, long N);
int nf_wide_bwd(nf_ctx *, const nf_flow_desc *, float *state, float *gbar, const float *lbar, float lbar_const, long N,
                float *ws, float *g_out, bool inv_dir = false);
size_t nf_wide_train_ws_floats(nf_ctx *, const nf_flow_desc *, long N);
int nf_wide_train_forward(nf_ctx *, const nf_flow_desc *, float *xt, long N, float *ladj, float *ws);
int nf_wide_train_backward(nf_ctx *, const nf_flow_desc *, float *state, float *gbar, const float *lbar,
                           float lbar_const, long N, float *ws, float *g_out, float *scratch = nullptr);
size_t nf_wide_fwd_stash_floats(nf_ctx *, const nf_flow_desc *, long N);
size_t nf_wide_train_scratch_floats(nf_ctx *, const nf_flow_desc *, long N);
size_t nf_wide_wimg_bytes(nf_ctx *, const nf_flow_desc *desc);

// ---- nf_rqs.hip: neural spline couplings ----------------------------------------------------------------------------
bool nf_rqs_supported(const nf_flow_desc *desc);
int nf_rqs_pack(nf_ctx *, const nf_flow_desc *, const float *theta);
int nf_rqs_chain(nf_ctx *, const nf_flow_desc *, bool inverse, float *xt, long N, float *ladj, int k_only, void *tape = nullptr);
size_t nf_rqs_tape_bytes(const nf_flow_desc *desc, long N);
int nf_rqs_bwd_grid(nf_ctx *, long N);
int nf_rqs_bwd(nf_ctx *, const nf_flow_desc *, int k, float *y, float *ybar, const float *lbar, float lbar_const, long N,
               float *slab, long slab_stride, int grid, bool inv_dir = false, void *tape = nullptr);
long nf_rqs_slab_floats(const nf_flow_desc *desc);
long nf_rqs_chain_grid(nf_ctx *, long N);
int nf_rqs_chain_elbo(nf_ctx *, const nf_flow_desc *, long N, uint64_t seed, uint64_t off, uint32_t stream,
                      const nf_target *target, float *yt, float *gt, double gscale, double *partial,
                      double pscale, void *tape = nullptr, const uint32_t *stream_ptr = nullptr);
int nf_rqs_reduce_slabs(nf_ctx *, const nf_flow_desc *, const float *slab, int nslab, float *g);
long nf_rqs_epilogue_blocks(const nf_flow_desc *desc);
int nf_rqs_epilogue(nf_ctx *, const nf_flow_desc *, const float *slab, int nslab, float *g, const double *lpart, int nlpart, float *theta,
                    float *m, float *v, double lr, double b1, double b2, double eps, unsigned t_val, double *gpart,
                    const unsigned *t_ptr = nullptr);
bool nf_rqs_chain_fkl_ok(const nf_flow_desc *desc);
int nf_rqs_chain_fkl(nf_ctx *, const nf_flow_desc *, const float *ys, long N, float *zt, float *gt, double gscale, double *partial,
                     double pscale, void *tape);
size_t nf_rqs_wimg_bytes(const nf_flow_desc *desc);

// ---- nf_simple.hip: planar / radial / mean-field flows ---------------------------------------------------------------
bool nf_simple_supported(const nf_flow_desc *desc);
int nf_simple_apply(nf_ctx *, const nf_flow_desc *, int layer_lo, int layer_hi, bool inverse, const void *theta,
                    const void *x, long N, void *y, void *ladj);
size_t nf_simple_bwd_ws_bytes(nf_ctx *, const nf_flow_desc *, long N);
int nf_simple_bwd(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, const void *ybar, const void *lbar,
                  double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws, bool have_stash, bool inv = false);
int nf_simple_apply_stash(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, long N, void *y, void *ladj,
                          void *ws, bool inverse = false);
long nf_simple_elbo_max_partials(nf_ctx *);
int nf_simple_elbo_forward(nf_ctx *, const nf_flow_desc *, const nf_target *, const void *theta, const void *xs, long N,
                           uint64_t seed, uint64_t off, uint32_t stream_id, void *gbar, double gscale, double *partial,
                           double pscale, void *ws, long *npartial);
bool nf_simple_step_supported(const nf_flow_desc *desc);
size_t nf_simple_step_ws_bytes(nf_ctx *, const nf_flow_desc *, long N);
int nf_simple_elbo_step(nf_ctx *, const nf_flow_desc *, const nf_target *, const void *theta, const void *xs, long N,
                        uint64_t seed, uint64_t off, uint32_t stream_id, double gscale, double lbar_const, double *partial,
                        double pscale, void *ws, void *gtheta_out, long *npartial, const uint32_t *step_device);
int nf_simple_epilogue_blocks(const nf_flow_desc *desc);
int nf_simple_epilogue(nf_ctx *, const nf_flow_desc *, const void *slabs, int nblk, void *g, const double *lpart, void *theta, void *m,
                       void *v, double lr, double b1, double b2, double eps, unsigned t_val, const unsigned *t_ptr, double *gpart);
int nf_simple_rand(nf_ctx *, const nf_flow_desc *, const void *theta, long N, uint64_t seed, uint64_t off, uint32_t stream_id,
                   void *y);

// ---- nf_generic64.hip: general coupling kernels, Float64 and the Float32 shapes the MFMA paths do not build; one thread
// per sample, standard layout -------------------------------------------------------------------------------------------
bool nf_g64_supported(const nf_flow_desc *desc);
int nf_g64_apply(nf_ctx *, const nf_flow_desc *, int layer_lo, int layer_hi, bool inverse, const void *theta,
                 const void *x, long N, void *y, void *ladj);
size_t nf_g64_bwd_ws_bytes(const nf_flow_desc *desc, long N);
int nf_g64_apply_keep(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, long N, void *y, void *ladj, void *ws);
int nf_g64_bwd(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, const void *ybar, const void *lbar,
               double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws);
size_t nf_g64_bwd_inv_ws_bytes(const nf_flow_desc *desc, long N);
int nf_g64_bwd_inv(nf_ctx *, const nf_flow_desc *, const void *theta, void *z, void *gbar, double lbar_const, long N,
                   void *gtheta_out, void *ws);
size_t nf_l64_scratch_bytes(const nf_flow_desc *desc, long N);

// ---- nf_hamiltonian.hip: Hamiltonian flow of the demos ---------------------------------------------------------------
bool nf_hf_supported(const nf_flow_desc *desc);
int nf_hf_apply(nf_ctx *, const nf_flow_desc *, int lo, int hi, bool inverse, const void *theta, const void *x, long N,
                void *y, void *ladj);
size_t nf_hf_bwd_ws_bytes(const nf_flow_desc *desc, long N);
int nf_hf_bwd(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, const void *ybar, const void *lbar,
              double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws);
int nf_hf_bwd_inv(nf_ctx *, const nf_flow_desc *, const void *theta, const void *u, const void *gbar, double lbar_const,
                  long N, void *gtheta_out, void *ws);

// ---- nf_fullrank.hip: full-rank Gaussian family, Shift o Scale(LowerTriangular) --------------------------------------
bool nf_fr_supported(const nf_flow_desc *desc);
size_t nf_fr_apply_ws_bytes(const nf_flow_desc *desc, bool inverse);
int nf_fr_apply(nf_ctx *, const nf_flow_desc *, int lo, int hi, bool inverse, const void *theta, const void *x, long N, void *y,
                void *ladj);
size_t nf_fr_bwd_ws_bytes(nf_ctx *, const nf_flow_desc *, long N);
int nf_fr_bwd(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, const void *ybar, const void *lbar,
              double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws);
int nf_fr_bwd_grid(nf_ctx *, long N);
int nf_fr_fwd_tiled(nf_ctx *, const nf_flow_desc *, const float *theta, const float *xt, long N, float *yt, float *ladj);
int nf_fr_grad(nf_ctx *, const nf_flow_desc *, const float *theta, const float *x, int x_tiled, const float *ybar, int y_tiled,
               const float *lbar, float lbar_const, long N, float *slabs, float *gtheta_out);
int nf_fr_bwd_x_tiled(nf_ctx *, const nf_flow_desc *, const float *theta, const float *xt, const float *ybar, const float *lbar,
                      float lbar_const, long N, float *slabs, float *gtheta_out, float *xbar);
int nf_fr_pull_tiled(nf_ctx *, const nf_flow_desc *, const float *theta, const float *ybar, long N, float *xbar);

// ---- nf_noncentred.hip: the non-centring layer of NF_KIND_NONCENTRED; `desc` is the layer's own descriptor ---------------
long nf_nc_params(const nf_flow_desc *desc);
bool nf_nc_tiled_supported(const nf_flow_desc *desc);
int nf_nc_apply(nf_ctx *, const nf_flow_desc *, bool inverse, const void *theta, const void *x, long N, void *y, void *ladj);
size_t nf_nc_bwd_ws_bytes(const nf_flow_desc *desc, long N);
int nf_nc_bwd(nf_ctx *, const nf_flow_desc *, const void *theta, const void *x, const void *ybar, const void *lbar,
              double lbar_const, long N, void *xbar_out, void *gtheta_out, void *ws);
int nf_nc_fwd_tiled(nf_ctx *, const nf_flow_desc *, const float *lam, const float *xt, long N, float *yt, float *ladj);
size_t nf_nc_slab_floats(nf_ctx *, const nf_flow_desc *, long N);
int nf_nc_bwd_tiled(nf_ctx *, const nf_flow_desc *, const float *lam, const float *yt, float *gt, const float *lbar,
                    float lbar_const, long N, float *slab, float *glam_out);
