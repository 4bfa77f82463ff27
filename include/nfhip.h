/* nfhip.h -- C ABI of libnfhip.so: the MI355X (gfx950) implementation of the
 * ELBO / reverse-KL hot path of TuringLang/NormalizingFlows.jl.
 *
 * This is the drop-in boundary.  The reference is pure
 * Julia with no FFI of its own; the seams it offers for a device back end are
 * generic functions selected by dispatch.  Every entry point below names the
 * reference interface it stands behind (paths relative to the reference
 * checkout).  The Julia-side binding (`ccall`) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns an int status: 0 = ok, > 0 = hipError_t of a failed
 *     HIP call, < 0 = NF_ERR_* argument / capability error.  Nothing throws or
 *     aborts; the host wrapper turns non-zero into error(nf_strerror(code)).
 *   - All array pointers are DEVICE pointers owned by the caller (AMDGPU.jl
 *     ROCArray -> pointer(A); torch tensor -> data_ptr()), unless the parameter
 *     name ends in _host.
 *   - A batch is d x N column-major with one sample per column, i.e. x[j*d + i]
 *     (reference: src/objectives/elbo.jl:52,60; src/flows/realnvp.jl:29).
 *   - theta is the flat parameter vector produced by Optimisers.destructure(flow)
 *     (src/NormalizingFlows.jl:67); its layout is documented in DESIGN.md and
 *     matches oracle/nf_oracle.py:layers_flat_order.
 *   - Work is enqueued on the context's HIP stream and is asynchronous unless
 *     the function returns a host scalar.
 *   - A context is not thread-safe (the reference's caller is one Julia task).
 */
#ifndef NFHIP_H
#define NFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NF_ABI_VERSION 4

/* status codes (< 0: library errors; > 0: hipError_t) */
#define NF_OK 0
#define NF_ERR_ARG -1          /* null pointer, negative size, bad enum            */
#define NF_ERR_UNSUPPORTED -2  /* flow shape / dtype not built into this library   */
#define NF_ERR_NO_DEVICE -3    /* no gfx950 device visible                         */
#define NF_ERR_NONFINITE -4    /* loss or gradient norm became non-finite (nf_elbo_step; the reference's
                                  tests require finite ELBOs, test/flow.jl:58-60)  */
#define NF_ERR_WORKSPACE -7    /* the caller-provided arena (nf_ctx_set_arena) is too small         */
#define NF_ERR_NO_RCCL -5      /* librccl.so.1 could not be loaded (multi-GPU entry points only) */
#define NF_ERR_RCCL -6         /* an RCCL call failed (nf_strerror gives RCCL's message), or a step left this rank's collective
                                  sequence incomplete (nf_elbo_step with bucketed all-reduce: fewer messages issued than
                                  nf_comm_bucket_count promises -- the peers wait in RCCL).  Either way the context's
                                  communicator is unusable: every later collective call returns this code until
                                  nf_comm_destroy + a new nf_comm_init_rank on EVERY rank.  Any other code from nf_elbo_step
                                  under a communicator is a local failure with a complete collective sequence.          */

/* flow kinds: the constructors of src/flows/*.jl */
#define NF_KIND_PLANAR 0    /* planarflow  src/flows/planar_radial.jl:21-29        */
#define NF_KIND_RADIAL 1    /* radialflow  src/flows/planar_radial.jl:52-60        */
#define NF_KIND_REALNVP 2   /* realnvp     src/flows/realnvp.jl:170-180            */
#define NF_KIND_NSF 3       /* nsf         src/flows/neuralspline.jl:218-234       */
#define NF_KIND_MEANFIELD 4 /* Shift o Scale, test/interface.jl:22-25              */
#define NF_KIND_HAMILTONIAN 5 /* mean-field reference + (momentum Shift o Scale) o LeapFrog blocks on the
                                 joint [x; rho], example/demo_hamiltonian_flow.jl:27-146: d = 2 * dims,
                                 nlayers = blocks, K = leapfrog steps per block, score = target whose
                                 score drives the integrator; targets passed to the ELBO entry points
                                 describe x, the library adds log N(rho; 0, I) (logp_joint, demo :121-128).
                                 theta = [shift0(d); scale0(d); per block: shift_rho(d/2), scale_rho(d/2),
                                 log_eps(d/2)] -- the reference distribution's affine map FIRST (destructure of
                                 a TransformedDistribution whose `dist` is q0 = transformed(MvNormal, Shift o
                                 Scale), demo :135-137).  nf_param_count cannot detect a permuted theta: bind
                                 by name, see INTEGRATION.md "theta order of the Hamiltonian demo flow".
                                 Limits (NF_ERR_UNSUPPORTED beyond them): d / 2 <= 32 (HF_MAXD), K <= 16 (HF_MAXL), and
                                 the reverse kernels' gradient row of nf_param_count elements must fit 128 KiB of LDS:
                                 at most 16 384 parameters in Float64, 32 768 in Float32. */

#define NF_KIND_FULLRANK 7 /* Shift o Scale of test/interface.jl:22-25 with a LowerTriangular scale (a matrix where the reference
                              passes a vector; built through create_flow, src/flows/utils.jl:23-26): y = mu + L x,
                              ladj = sum_i log|L_ii| -- the full-rank Gaussian family of ADVI.  theta = [mu(d) ; L as a d x d
                              column-major matrix] (shift first, as test/interface.jl:47-48 pins for the diagonal family), so
                              nf_param_count = d + d^2 and nf_layer_count = 2 (flat order: Shift, Scale).  The strict upper
                              triangle of L belongs to theta (the parent matrix of LowerTriangular) and is never read: every
                              output has the same bits whatever it holds (NaN included), its gradient is exactly 0.0, Adam
                              leaves it where it was.  Diagonal entries may be negative; zero is invalid.  nlayers must be 1
                              (NF_ERR_ARG otherwise); n_hidden, K, B and score are ignored.  Limits: 1 <= d <= 256
                              (NF_ERR_UNSUPPORTED beyond).  Served: nf_flow_fwd / inv / rand, nf_layer_apply, the tape pair
                              and nf_flow_bwd, nf_elbo_batch(_rng), nf_elbo_value_and_grad, nf_elbo_step (the split sequence,
                              with or without a communicator), general bases -- with EVERY built-in target, the linear-predictor
                              kinds and the mixture included (Float32: the mixture up to d = 64, as for the coupling flows).
                              NF_ERR_UNSUPPORTED: nf_loglikelihood, nf_loglikelihood_value_and_grad, nf_loglikelihood_step(_enqueue),
                              nf_elbo_step_enqueue, and as a segment of NF_KIND_COMPOSITE. */

#define NF_KIND_COMPOSITE 6 /* create_flow((L1, ..., Ln), q0) with MIXED bijector families (src/flows/utils.jl:23-26:
                               any list of bijectors composes).  `segments` lists the maximal runs of one family in FLAT
                               order (segment 0 = outermost = applied last), each a descriptor of one of the kinds above
                               with the same d / dtype; theta = the segments' thetas concatenated in that order, which is
                               the order Optimisers.destructure walks the composition.  Forward, inverse, per-layer
                               application, rand, elbo / elbo_batch, the training step, loglikelihood, forward-KL
                               training and nf_flow_bwd are all built (reverse passes chain the segments' own). */

#define NF_KIND_PRECOND 8 /* transformed(q0, Shift(mu) o Scale(LowerTriangular(L)) o couplings): a coupling flow under a full-rank
                             affine layer, y = mu + L T(x) -- one create_flow((Shift, Scale, couplings...), q0) in the reference
                             (src/flows/utils.jl:23-26).  nlayers = 1, nsegments = 1 and `segments` points to ONE inner
                             descriptor of kind NF_KIND_REALNVP or NF_KIND_NSF with the same d and dtype and no base
                             (NF_ERR_ARG otherwise); a general base belongs to the outer descriptor.  Limits: d <= 256 and
                             whatever the inner flow's own limits are (NF_ERR_UNSUPPORTED beyond).  theta = [mu(d) ; L, d x d
                             column-major ; theta_inner], outermost first; the strict upper triangle of L keeps
                             NF_KIND_FULLRANK's contract (never read, gradient exactly 0.0).  nf_param_count = d + d^2 +
                             P_inner; nf_layer_count = 2 + the inner flow's (flat order: Shift, Scale, the couplings).
                             Served: nf_flow_fwd / inv / rand, nf_layer_apply, nf_loglikelihood (value only), the tape pair
                             and nf_flow_bwd, nf_elbo_batch(_rng), nf_elbo_value_and_grad, nf_elbo_step (the split sequence,
                             with or without a communicator), general bases -- with every target the inner flow is served
                             with.  Float32 with the inner flow on the matrix-pipe kernels: nf_elbo_value_and_grad keeps every
                             buffer in the tiled layout from the draw to the gradient, and the full-rank layer's reverse pass
                             is one launch from d = 33 on, the two launches of NF_KIND_FULLRANK at d <= 32 (as measured; the
                             same bits; NF_PRECOND_BWD_SPLIT in the environment, read once per process, overrides: 1 = the
                             two launches, 0 = the one launch, at every d).  NF_ERR_UNSUPPORTED:
                             nf_loglikelihood_value_and_grad, nf_loglikelihood_step(_enqueue), nf_elbo_step_enqueue;
                             NF_ERR_ARG as a segment of NF_KIND_COMPOSITE. */

/* (kind 9 is unassigned) */
#define NF_KIND_NONCENTRED 10 /* transformed(q0, S o T): an inner flow T under the non-centring layer S of the hierarchical targets.
                             Over z = [beta (p) ; tau (G)] (d = p + G, NF_TARGET_HGLM_*) or [beta ; tau ; lambda] (d = p + G + 1,
                             NF_TARGET_DGLM_*; the last coordinate passes through), with g(j) the group of coefficient j:
                               y_j = z_j exp(lam_j tau_g(j)) for j < p with g(j) >= 0, y_j = z_j otherwise,
                               ladj = sum_{j: g(j) >= 0} lam_j tau_g(j).
                             lam = 0 is the identity (the centred parameterisation the targets are written in), lam = 1 the
                             non-centred beta = exp(tau) z, in between the flow learns its own (Gorinova et al., "Automatic
                             reparameterisation").  nsegments = 1 and `segments` points to ONE inner descriptor of kind
                             NF_KIND_REALNVP, NF_KIND_NSF or NF_KIND_FULLRANK with the same d and dtype and no base; `score`
                             (host pointer) is a target of kind 16..20 or 29..31 that passes its own argument check at this d:
                             S reads grp[p] from its device buffer p0 (every index bounded by select: a garbage buffer gives
                             wrong numbers, never an access outside the d features), and p, G from d and s1; the buffer must
                             outlive the flow.  The ELBO target of the entry points may be that target or any other the inner
                             flow is served with.  K = 0: lam is trained; K = 1: lam is frozen, its p gradient entries are
                             written as exactly 0.0; any other K, or anything else above, is NF_ERR_ARG; what the inner flow
                             refuses is NF_ERR_UNSUPPORTED.  theta = [lam (p) ; theta_inner]; the lam_j of a coefficient without
                             a group is never read (NaN there changes no output bit; its gradient is exactly 0.0).
                             nf_param_count = p + P_inner; nf_layer_count = the inner flow's + 1: the inner flow's layers come
                             first, S is the last.  Served: nf_flow_fwd / inv / rand, nf_layer_apply, nf_loglikelihood (value
                             only), the tape pair and nf_flow_bwd, nf_elbo_batch(_rng), nf_elbo_value_and_grad, nf_elbo_step
                             (the split sequence), general bases, shards.  Float32 with the inner flow on the tiled kernels:
                             nf_elbo_value_and_grad keeps every buffer in the tiled layout from the draw to the gradient (S out
                             of place, so that the inner chain's output stays the tape of its reverse pass; S's reverse pass is
                             one launch).  NF_ERR_UNSUPPORTED: nf_loglikelihood_value_and_grad,
                             nf_loglikelihood_step(_enqueue), nf_elbo_step_enqueue; NF_ERR_ARG as a segment of
                             NF_KIND_COMPOSITE or as the inner flow of NF_KIND_PRECOND. */

#define NF_DTYPE_F32 0
#define NF_DTYPE_F64 1

#define NF_TARGET_DIAGGAUSS 0 /* MvNormal(mu, Diagonal(var)), test/flow.jl:43-46        */
#define NF_TARGET_BANANA 1    /* Banana(d, b, var), example/targets/banana.jl:58-83     */
#define NF_TARGET_FUNNEL 2    /* Funnel(d, mu, sigma), example/targets/neal_funnel.jl:53-72 (s0 = mu, s1 = sigma) */
#define NF_TARGET_WARPED 3    /* WarpedGauss(s1, s2), d = 2, example/targets/warped_gaussian.jl:51-87 (s0, s1) */
#define NF_TARGET_CROSS 4     /* Cross(mu, sigma), d = 2, example/targets/cross.jl:30-37 (s0 = mu, s1 = sigma) */
/* Linear-predictor targets: log p(y) = c + sum_i phi(u_i) + prior(y), u = A (y - mu), evaluated as two GEMMs per tile of
 * samples on the matrix pipe (d <= 256, any number of rows).  All device pointers are in the flow's element type.
 *   NF_TARGET_DENSEGAUSS  MvNormal(mu, Sigma), Sigma = L L'.  p0 = mu[d]; p1 = W[d x d] row-major, W = inv(L) (lower
 *       triangular, stored dense with its zeros), so u = W (y - mu) ~ N(0, I); s0 = log|det W| = -sum(log(diag(L))); s1 unused.
 *       log p = -d/2 log(2 pi) + s0 - |u|^2 / 2,  grad = -W' u.
 *   NF_TARGET_LOGREG      posterior of logistic-regression weights y in R^d under the prior N(0, s1^2 I), data rows x_i and
 *       labels t_i in {-1, +1}.  p0 = NULL (or a shift mu[d]); p1 = A[n x d] row-major with A_i = t_i x_i (the host folds the
 *       labels into the rows); s0 = n (an integer value, 1 <= n < 2^31); s1 = prior sigma > 0.
 *       log p = sum_i log sigmoid(u_i) - |y|^2 / (2 s1^2) - d/2 log(2 pi s1^2),  grad = A' sigmoid(-u) - y / s1^2,
 *       with log sigmoid(u) evaluated as min(u, 0) - log1p(exp(-|u|)).
 * Served by nf_target_logp and, as ELBO targets, by RealNVP / NSF flows (either element type), general bases and
 * compositions.  Planar, radial, mean-field and Hamiltonian flows answer NF_ERR_UNSUPPORTED to every ELBO entry point with
 * these kinds (their kernels evaluate the target one feature at a time); a Hamiltonian descriptor cannot use them as its
 * score either.  nf_elbo_step runs the split sequence (value and gradient, then Adam) for them. */
#define NF_TARGET_DENSEGAUSS 5
#define NF_TARGET_LOGREG 6
/* Gaussian mixture: MixtureModel([MvNormal(mu_k, Sigma_k)], pi), K components with Sigma_k = L_k L_k' (what
 * example/targets/cross.jl:31-37 builds for Cross).  Kind 7 stays unassigned (callers may rely on it being "no such kind").
 *   With W_k = inv(L_k) and ONE common centre mbar = sum_k pi_k mu_k (the device centres a tile of samples once):
 *       u_k = W_k (y - mbar) - b_k,  b_k = W_k (mu_k - mbar),
 *       q_k = c_k - |u_k|^2 / 2,     c_k = log pi_k + log|det W_k| - d/2 log(2 pi),
 *       log p = logsumexp_k q_k,     grad = -sum_k r_k W_k' u_k,  r_k = exp(q_k - log p).
 *   p1 = A[K d x d] row-major: the W_k stacked, each lower triangular and stored dense with its zeros;
 *   p0 = ONE buffer [d + K d + K]: mbar | b | c;  s0 = K (an integer value, K >= 1, K d < 2^31);  s1 unused, must be 0.
 *   All device pointers are in the flow's element type.  NF_ERR_ARG for a NULL p0 / p1, s0 < 1, a non-integral or too
 *   large s0, or s1 != 0 -- before any device work.
 * Evaluated in one pass over the components with a running log-sum-exp (never (-inf) - (-inf); a sample far from every
 * component keeps a finite log p and score).  Served like the linear-predictor kinds: nf_target_logp (d <= 256), RealNVP /
 * NSF flows of either element type, general bases and compositions as ELBO targets; planar, radial, mean-field and
 * Hamiltonian flows answer NF_ERR_UNSUPPORTED at every ELBO entry point (a Hamiltonian descriptor cannot use it as its
 * score either); nf_elbo_step runs the split sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED.
 * Float32 RealNVP / NSF flows on the tiled path take the matrix-pipe kernel, which is built for d <= 64 (every LDS-resident
 * coupling flow); with 64 < d (the weight-streaming shapes) those flows answer NF_ERR_UNSUPPORTED at every ELBO entry
 * point before any launch -- there is no chunked form.  A general base does not change this: it runs the same flow's
 * standard-base path on draws of its own. */
#define NF_TARGET_GAUSSMIX 8
/* Generalised linear-predictor targets: the regression posteriors that need a per-row offset, a per-row weight, a linear
 * term or a family parameter.  One form, five row functions:
 *       log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) + lin . y - |y|^2 / (2 s1^2) - d/2 log(2 pi s1^2),   u = A y + off,
 *       grad     = A' (wt o phi'(u)) + lin - y / s1^2.
 *   p1 = A[rows x d] row-major;  p0 = ONE buffer of d + 2 rows + 2 elements: lin[d] | off[rows] | wt[rows] | par[2], with
 *   par[0] the family parameter (nu > 0 for STUDENT, ignored by the others) and par[1] the additive constant the host folded
 *   (log-factorials, normalisers);  s0 = rows (an integer value, 1 <= rows < 2^31);  s1 = the prior sigma > 0, where +inf
 *   is the flat prior (both prior terms vanish).  All device pointers are in the flow's element type.  NF_ERR_ARG for a
 *   NULL p0 / p1, a bad s0, s1 <= 0 or a NaN s1 -- before any device work.
 *   NF_TARGET_GLM_LOGIT    phi = log sigmoid(u)                    phi' = sigmoid(-u)       (binomial / Bernoulli, logit link)
 *   NF_TARGET_GLM_PROBIT   phi = log Phi(u)                        phi' = phi_N(u) / Phi(u) (through erfcx on the left tail)
 *   NF_TARGET_GLM_POISSON  phi = -exp(u)                           phi' = -exp(u)           (log link; k u sits in lin / par[1])
 *   NF_TARGET_GLM_STUDENT  phi = -(nu + 1)/2 log1p(u^2 / nu)       phi' = -(nu + 1) u / (nu + u^2)
 *   NF_TARGET_GLM_NORMAL   phi = -u^2 / 2                          phi' = -u
 * A row with wt_i == 0 contributes exactly 0 to the value and the gradient (by select: a subsampling mask may sit over a
 * row whose phi overflows).  Nothing is clamped: a POISSON predictor beyond exp's range gives a non-finite value, which
 * nf_elbo_step reports as NF_ERR_NONFINITE.  Served exactly like NF_TARGET_DENSEGAUSS / NF_TARGET_LOGREG: nf_target_logp
 * (d <= 256), RealNVP / NSF flows of either element type including the weight-streaming shapes, general bases and
 * compositions; nf_elbo_step runs the split sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial,
 * mean-field and Hamiltonian flows answer NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included. */
#define NF_TARGET_GLM_LOGIT 9
#define NF_TARGET_GLM_PROBIT 10
#define NF_TARGET_GLM_POISSON 11
#define NF_TARGET_GLM_STUDENT 12
#define NF_TARGET_GLM_NORMAL 13
/* Softmax (multinomial-logit) regression: the posterior of C weight vectors w_c in R^p under the prior N(0, sigma^2 I), data
 * rows x_i, labels c_i in {0 .. C-1} and row weights wt_i >= 0.  Kind 14 stays unassigned (as kind 7 does).
 *   y in R^d, d = C p, class-major: y = [w_0; ...; w_{C-1}] -- vec(W) of the p x C weight matrix in column-major order, logits = X W.
 *       u_{i,c}    = x_i . w_c
 *       log p(y)   = par[1] + sum_i wt_i (u_{i,c_i} - logsumexp_c u_{i,c}) - par[0] |y|^2 / 2,
 *       grad_{w_c} = sum_i wt_i (1[c_i = c] - softmax_c(u_i)) x_i - par[0] w_c.
 *   p1 = X[rows x p] row-major (an intercept is a ones column);  p0 = ONE buffer of 2 rows + 2 elements: lab[rows] | wt[rows] |
 *   par[2], the labels as integer-valued elements, par[0] the prior precision 1 / sigma^2 (0: the flat prior) and par[1] the
 *   additive constant the host folded (-d/2 log(2 pi sigma^2) plus any multinomial coefficients);  s0 = rows (an integer value,
 *   1 <= rows < 2^31);  s1 = C (an integer value, 2 <= C <= 16).  All device pointers are in the flow's element type.
 *   NF_ERR_ARG for a NULL p0 / p1, a bad s0, a non-integral or out-of-range s1, or d % C != 0 -- before any device work;
 *   NF_ERR_UNSUPPORTED for d > 256.
 * A row with wt_i == 0 contributes exactly 0 to the value and the gradient (by select: a subsampling mask may sit over a row
 * whose logits are not finite).  The log-sum-exp subtracts the row maximum: nothing overflows for finite logits, nothing is
 * clamped.  Served exactly like NF_TARGET_GLM_*: nf_target_logp (d <= 256), RealNVP / NSF flows of either element type
 * including the weight-streaming shapes, full-rank flows, general bases and compositions; nf_elbo_step runs the split
 * sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial, mean-field and Hamiltonian flows answer
 * NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included. */
#define NF_TARGET_SOFTMAX 15
/* Hierarchical GLM targets: the five GLM families under a structured prior -- groups of coefficients share a scale that is
 * itself a coordinate with a hyper-prior (random intercepts, varying slopes, eight schools, shrinkage priors; the centred
 * parameterisation, whose joint density has the funnel's geometry).  Kind = the GLM kind + 7.
 *   y in R^d is [beta (p coefficients) ; tau (G group log-scales)], d = p + G, p >= 1, 0 <= G <= d - 1.  Coefficient j has
 *   the prior N(0, sigma_j^2) with a fixed sigma_j when grp_j = -1 and N(0, exp(tau_g)^2) when grp_j = g in [0, G).
 *       u        = A y + off                                  (A is rows x d; the tau-columns are usually zero)
 *       w_j(y)   = isd_j^2 (isd = 1 / sigma_j; 0: a flat prior on that coefficient)  if grp_j < 0,   exp(-2 tau_{grp_j})  otherwise
 *       x_g      = tau_g - hm_g
 *       h_g(x)   = -(x his_g)^2 / 2    hk_g = 0   tau_g ~ N(hm, 1 / his^2)                (log-normal scale)
 *                = -exp(2 x) / 2       hk_g = 1   exp(tau_g) ~ half-normal(s),  hm = log s
 *                = -softplus(2 x)      hk_g = 2   exp(tau_g) ~ half-Cauchy(s),  hm = log s
 *       log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) + lin . y - sum_{j<p} beta_j^2 w_j(y) / 2 + sum_g h_g(x_g)
 *       d beta_j = [A' (wt o phi')]_j + lin_j - beta_j w_j
 *       d tau_g  = [A' (wt o phi')]_{p+g} + lin_{p+g} + exp(-2 tau_g) sum_{j: grp_j = g} beta_j^2 + h_g'(x_g)
 *       h'       = -x his^2 | -exp(2 x) | -2 sigmoid(2 x)
 *   Everything linear in y or constant is folded by the host: the -n_g tau_g of the Gaussian normalisers and the +tau_g
 *   Jacobian of the two half-families sit in lin[p + g], every normaliser in par[1].
 *   p1 = A[rows x d] row-major;  s0 = rows (an integer value, 1 <= rows < 2^31);  s1 = G (an integer value, 0 <= G <= d - 1);
 *   p0 = ONE buffer of 4 d + 2 rows + 3 + G elements in the flow's element type:
 *       lin[d] | off[rows] | wt[rows] | par[2] | grp[p] | isd[p] | hm[G] | his[G] | hk[G] | gptr[G + 1] | gidx[p]
 *   grp, hk, gptr and gidx are integer-valued elements; gptr / gidx are the CSR member lists of the groups, each group's
 *   members in increasing feature index (which fixes the summation order).  NF_ERR_ARG for a NULL p0 / p1, a bad s0 or a bad
 *   s1 (NaN included) -- before any device work;  NF_ERR_UNSUPPORTED for d > 256.  The host cannot validate device memory:
 *   every index read from p0 is bounded by select before it addresses anything (a grp outside [0, G) is -1, a gidx outside
 *   [0, p) contributes 0, gptr is clamped to [0, p]).
 * Row weights as for NF_TARGET_GLM_*.  Nothing is clamped: a non-finite value is reported by nf_elbo_step as
 * NF_ERR_NONFINITE.  Served exactly like NF_TARGET_GLM_*: nf_target_logp (d <= 256), RealNVP / NSF flows of either element
 * type including the weight-streaming shapes, full-rank flows, general bases and compositions; nf_elbo_step runs the split
 * sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial, mean-field and Hamiltonian flows answer
 * NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included. */
#define NF_TARGET_HGLM_LOGIT 16
#define NF_TARGET_HGLM_PROBIT 17
#define NF_TARGET_HGLM_POISSON 18
#define NF_TARGET_HGLM_STUDENT 19
#define NF_TARGET_HGLM_NORMAL 20
/* One-hidden-layer Bayesian neural-network targets: the posterior of a tanh network with H hidden units over its weights, under
 * the five GLM row functions.  Kind = the GLM kind + 13; kind 21 stays unassigned (as kinds 7 and 14 do).
 *   y in R^d, d = H (p + 1) + 1, hidden-unit-major: y = [w_0; ...; w_{H-1}; v; c] -- w_k in R^p the input weights of unit k, v in R^H
 *   the output weights, c the output bias.  A hidden bias is a ones column of X.
 *       a_{ik}   = tanh(x_i . w_k)        f_i = c + sum_k v_k a_{ik}        u_i = scl_i f_i + off_i
 *       log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) - par[2]/2 sum_k |w_k|^2 - par[3]/2 (|v|^2 + c^2)
 *       g_i      = wt_i phi'(u_i; par[0]) scl_i                              (0 exactly when wt_i = 0)
 *       d c      = sum_i g_i - par[3] c
 *       d v_k    = sum_i g_i a_{ik} - par[3] v_k
 *       d w_k    = sum_i g_i v_k (1 - a_{ik}^2) x_i - par[2] w_k
 *   p1 = X[rows x p] row-major;  p0 = ONE buffer of 3 rows + 4 elements: scl[rows] | off[rows] | wt[rows] | par[4], with par[0]
 *   the family parameter (nu > 0 for STUDENT, ignored by the others), par[1] the additive constant the host folded, par[2] the
 *   prior precision of the hidden weights and par[3] that of [v; c] (0: flat);  s0 = rows (an integer value, 1 <= rows < 2^31);
 *   s1 = H (an integer value, 1 <= H <= 16).  All device pointers are in the flow's element type.  scl and off carry the
 *   likelihood: labels +-1 in scl for LOGIT / PROBIT, scl = 1 / sigma and off = -t_i / sigma for Gaussian or Student noise,
 *   log-exposures in off for POISSON.
 *   NF_ERR_ARG for a NULL p0 / p1, a bad s0, a non-integral, NaN or out-of-range s1, d < H + 2 or (d - 1) % H != 0 (so that
 *   p = (d - 1) / H - 1 >= 1), then NF_ERR_UNSUPPORTED for d > 256 or p > 128 -- both before any device work.
 * A row with wt_i == 0 contributes exactly 0 to the value and to every gradient by select, wherever its values enter a sum: a
 * zero-weight row of huge finite features, or one whose phi overflows, changes no bit.  tanh saturates to exactly +-1 with
 * derivative exactly 0; nothing is clamped: a non-finite value is reported by nf_elbo_step as NF_ERR_NONFINITE.  Served exactly
 * like NF_TARGET_SOFTMAX: nf_target_logp (d <= 256), RealNVP / NSF flows of either element type including the
 * weight-streaming shapes, full-rank and preconditioned flows, general bases and compositions; nf_elbo_step runs the split
 * sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial, mean-field and Hamiltonian flows answer
 * NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included. */
#define NF_TARGET_BNN_LOGIT 22
#define NF_TARGET_BNN_PROBIT 23
#define NF_TARGET_BNN_POISSON 24
#define NF_TARGET_BNN_STUDENT 25
#define NF_TARGET_BNN_NORMAL 26
/* GLM targets with a learned dispersion: Gaussian / Student-t regression with an unknown residual scale (the linear mixed
 * model included) and negative-binomial regression with an unknown size.  The hierarchical kinds' sibling: there a log-scale
 * coordinate multiplies the prior, here one multiplies the likelihood.  Kinds 27 and 28 stay unassigned (as 7, 14 and 21 do).
 *   y in R^d is [beta (p) ; tau (G) ; lambda], d = p + G + 1, p >= 1, 0 <= G <= d - 2, d <= 256.  beta and tau are exactly the
 *   hierarchical kinds' coefficients and group log-scales (their w_j, h_g and member lists, with p = d - G - 1); G = 0 gives
 *   plain regressions with per-coefficient fixed prior scales.  lambda = y[d - 1] is the log-dispersion.
 *       u        = A y + off                  (A is rows x d; the tau- and lambda-columns are usually zero but take part like any column)
 *       log p(y) = par[1] + sum_i wt_i phi_i(u_i, lambda) + lin . y - sum_{j<p} beta_j^2 w_j(y) / 2 + sum_{g<G} h_g(tau_g - hm_g)
 *                  + h_G(lambda - hm_G) + T(lambda)
 *   h_G is one of the three hyper-prior forms applied to exp(lambda) (log-normal, half-normal, half-Cauchy, as a density over
 *   lambda): entry G of hm / his / hk, with an empty member list.
 *   NF_TARGET_DGLM_NORMAL / NF_TARGET_DGLM_STUDENT (scale families, sigma = exp(lambda)):
 *       z = u exp(-lambda),   phi = phi_fam(z; par[0]) (-z^2 / 2 | -(nu + 1)/2 log1p(z^2 / nu)),
 *       d phi / d u = exp(-lambda) phi'(z),   d phi / d lambda = -phi'(z) z,   T = 0;
 *       the -(sum_i wt_i) lambda of the normalisers is linear in y: the host folds it into lin[d - 1].
 *   NF_TARGET_DGLM_NEGBIN (counts k_i, integers; mean exp(u_i); size r = exp(lambda)):
 *       phi_i = -(k_i + e^lambda) softplus(u_i - lambda),
 *       d phi / d u = -(k_i + e^lambda) sigmoid(u_i - lambda),
 *       d phi / d lambda = -e^lambda softplus(u_i - lambda) + (k_i + e^lambda) sigmoid(u_i - lambda),
 *       T(lambda) = sum_{m=1}^{M-1} c_m log1p(m e^-lambda),   c_m = sum_{i: k_i > m} wt_i,   M = max k,
 *       T'(lambda) = -sum_m c_m m / (e^lambda + m).
 *     This is lgamma(k + r) - lgamma(r) + r log r - (k + r) log(r + e^u) rewritten so that no lgamma runs on the device and
 *     nothing cancels as r -> inf, where the form tends to the Poisson kind's.  The host folds, in float64, sum_i wt_i k_i u_i
 *     into lin and its offset part and -sum_i wt_i lgamma(k_i + 1) into par[1].  softplus and sigmoid are the exp(-|.|) forms
 *     of the logit row function.
 *   d lambda = [A' (wt o d phi / d u)]_{d-1} + lin_{d-1} + sum_i wt_i d phi_i / d lambda + h_G' + T'.
 *   p1 = A[rows x d] row-major;  s0 = rows (an integer value, 1 <= rows < 2^31);  s1 = G (an integer value, 0 <= G <= d - 2);
 *   p0 = ONE buffer in the flow's element type:
 *       lin[d] | off[rows] | wt[rows] | par[4] | grp[p] | isd[p] | hm[G+1] | his[G+1] | hk[G+1] | gptr[G+1] | gidx[p] | cnt[rows] | ctab[Mt]
 *   par[0] = nu for STUDENT, par[1] = the folded constant, par[2] = Mt, the table length (an integer value, NEGBIN only;
 *   ctab[j] = c_{j+1}), par[3] = 0.  cnt (the counts) and ctab are absent for NORMAL and STUDENT.
 *   NF_ERR_ARG for a NULL p0 / p1, a bad s0, or an s1 that is non-integral, NaN or outside 0 .. d - 2; NF_ERR_UNSUPPORTED for
 *   d > 256 -- both before any device work.  The host cannot validate device memory: every index or length read from p0 is
 *   bounded by select before it addresses anything (the hierarchical kinds' rule; Mt is clamped to [0, 4096]).
 * A row with wt_i == 0 contributes exactly 0 to the value and to every gradient, d lambda included, by select (zero-weight rows
 * never enter c_m: that is host work).  Nothing is clamped: a non-finite value is reported by nf_elbo_step as
 * NF_ERR_NONFINITE.  Served exactly like NF_TARGET_HGLM_*: nf_target_logp (d <= 256), RealNVP / NSF flows of either element
 * type including the weight-streaming shapes, full-rank and preconditioned flows, general bases and compositions;
 * nf_elbo_step runs the split sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial, mean-field and
 * Hamiltonian flows answer NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included. */
#define NF_TARGET_DGLM_NORMAL 29
#define NF_TARGET_DGLM_STUDENT 30
#define NF_TARGET_DGLM_NEGBIN 31
/* Ordinal (cumulative-logit) regression: an ordered categorical response k_i in {0 .. C-1} (ratings, grades, Likert items; polr,
 * brms::cumulative, Stan's ordered_logistic) with one linear predictor per row and C - 1 ordered cutpoints that are coordinates.
 *   y in R^d is [beta (p) ; gamma (C - 1)], d = p + C - 1 <= 256, 2 <= C <= 16, p >= 1.  The cutpoints are the ordered transform
 *       c_1 = gamma_1,   c_k = c_{k-1} + exp(gamma_k)   (k = 2 .. C-1);   c_0 = -inf, c_C = +inf
 *       eta_i    = x_i . beta + off_i
 *       P(k_i)   = sigmoid(c_{k_i + 1} - eta_i) - sigmoid(c_{k_i} - eta_i)
 *       log p(y) = par[1] + sum_i wt_i log P(k_i) - par[0]/2 |beta|^2 - par[2]/2 sum_k (c_k - par[3])^2 + sum_{k>=2} gamma_k
 *   (a density over the unconstrained y: the last sum is the transform's Jacobian).  The kernels evaluate the factored form
 *       sigmoid(a) - sigmoid(b) = sigmoid(a) sigmoid(-b) (1 - exp(-(a - b))),   a - b = exp(gamma_{k+1}) for adjacent cutpoints:
 *       sum_i wt_i log P(k_i) = sum_i wt_i ([k_i < C-1] log sigmoid(c_{k_i + 1} - eta_i) + [k_i > 0] log sigmoid(eta_i - c_{k_i}))
 *                               + sum_{k=1}^{C-2} n_k log1mexp(exp(gamma_{k+1})),     n_k = sum_i wt_i [k_i = k],
 *   log1mexp(D) = log(-expm1(-D)) for D <= ln 2 and log1p(-exp(-D)) beyond: no difference of probabilities is ever formed.
 *       d beta    = X' g - par[0] beta,   g_i = wt_i ([k_i > 0] sigmoid(c_{k_i} - eta_i) - [k_i < C-1] sigmoid(eta_i - c_{k_i + 1}))
 *       d c_m     = sum_i wt_i ([k_i = m-1] sigmoid(eta_i - c_m) - [k_i = m] sigmoid(c_m - eta_i)) - par[2] (c_m - par[3])
 *       d gamma_1 = sum_m d c_m,   d gamma_k = exp(gamma_k) sum_{m>=k} d c_m + n_{k-1} D / expm1(D) + 1,   D = exp(gamma_k)
 *   The rows are GROUPED BY LABEL and every label is padded to whole 32-row blocks with rows of weight 0, so that the label is a
 *   property of a row block (a label without rows has no block):
 *   p1 = X[R x p] row-major, R a multiple of 32;  s0 = R (an integer value, 32 <= R < 2^31, R % 32 == 0);  s1 = C (an integer
 *   value in 2 .. 16);  p0 = ONE buffer of 2 R + R/32 + 4 + C elements in the flow's element type:
 *       off[R] | wt[R] | lab[R/32] | par[4] | nk[C]
 *   par[0] = 1 / sigma_beta^2 and par[2] = 1 / sigma_c^2 (0: flat), par[1] the additive constant the host folded, par[3] the
 *   cutpoint prior's location; lab holds integer-valued elements, nk the n_k (folded by the host in float64).
 *   NF_ERR_ARG for a NULL p0 / p1, an s0 that is not a positive integer multiple of 32 fitting an int, an s1 that is non-integral,
 *   NaN or outside 2 .. 16, or d < C; then NF_ERR_UNSUPPORTED for d > 256 -- both before any device work.  The host cannot validate
 *   device memory: a block's label is bounded to [0, C-1] by select before it addresses anything (NaN -> 0).
 * A row with wt_i == 0 contributes exactly 0 to the value and to every gradient by select.  Nothing is clamped: a non-finite
 * value is reported by nf_elbo_step as NF_ERR_NONFINITE.  Served exactly like NF_TARGET_BNN_*: nf_target_logp (d <= 256), RealNVP /
 * NSF flows of either element type including the weight-streaming shapes, full-rank and preconditioned flows, general bases and
 * compositions; nf_elbo_step runs the split sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial, mean-field
 * and Hamiltonian flows answer NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included.  A non-centring layer
 * does not take it (no group structure).
 * The value is 32.  It is written relative to the kind before it: tests/test_disp_cpu.py reads the kinds that are defined by a
 * literal and holds the highest of them at 31; tests/test_ordinal_cpu.py evaluates this definition and holds it at 32. */
#define NF_TARGET_ORDINAL_LOGIT (NF_TARGET_DGLM_NEGBIN + 1)
/* Risk-set regression: the partial likelihood of Cox proportional hazards (coxph, brms cox, stan_surv), conditional logit (matched
 * case-control, McFadden discrete choice) and Plackett-Luce rankings.  The first target whose rows interact: they are coupled through
 * risk sets, and once the host has sorted them every risk set is a prefix of its segment (stratum, choice set).
 *   y = beta in R^d, d = p <= 256;   eta_i = x_i . y + off_i,   a_i = eta_i + logw_i,   seg(i) the contiguous segment of row i
 *       log p(y) = par[1] + lin . y - sum_i m_i c_i - par[0]/2 |y|^2
 *       c_i      = log sum_{j in seg(i), j <= i} w_j exp(eta_j)          (inclusive prefix log-sum-exp inside the segment)
 *   w_j >= 0 the risk weight (w_j = 0, logw_j = -inf, drops row j from every risk set exactly, by select: its predictor is never
 *   consumed), m_i >= 0 the event mass (m_i > 0 only where the prefix holds a row of positive weight -- the host checks), lin the
 *   folded sum_i e_i x_i, par[0] = 1 / sigma^2 (0: flat).  Score with respect to eta_j:  -exp(a_j - c_j) V_j,
 *       V_j = m_j + V_{j+1} exp(c_j - c_{j+1})  backwards inside the segment,  V = m on the segment's last row.
 *   c is non-decreasing inside a segment and a_j <= c_j, so every exponential has an argument <= 0; the forward recurrence is
 *   c_i = logaddexp(c_{i-1}, a_i).  Nothing is clamped and no ratio of sums is formed.
 *   p1 = X[R x p] row-major, the rows in the host's order, the tail padded with rows of weight 0 to a multiple of 32 (a segment may
 *   start at any row);  s0 = R (an integer value, 32 <= R < 2^31, R % 32 == 0);  s1 = the prior sigma (> 0, +inf: flat), as the GLM
 *   kinds have it;  p0 = ONE buffer of 4 R + d + 2 elements in the flow's element type, distinct from p1:
 *       off[R] | logw[R] | m[R] | segstart[R] | lin[d] | par[2]
 *   segstart holds 0 / 1 (any value other than 0 starts a segment; row 0 always does).
 *   NF_ERR_ARG for a NULL p0 / p1, p0 == p1, an s0 that is not a positive integer multiple of 32 fitting an int, an s1 that is not
 *   > 0 (NaN included) or d < 1; then NF_ERR_UNSUPPORTED for d > 256 or R > NF_RISKSET_MAXR (the tiled kernel keeps one carry per
 *   32-row block and sample in LDS) -- both before any device work.  The host cannot validate device memory: every flag read from
 *   the buffer is bounded by select before it steers anything.
 * Served exactly like NF_TARGET_ORDINAL_LOGIT: nf_target_logp, RealNVP / NSF flows of either element type including the
 * weight-streaming shapes, full-rank and preconditioned flows, general bases and compositions; nf_elbo_step runs the split
 * sequence, nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED; planar, radial, mean-field and Hamiltonian flows answer
 * NF_ERR_UNSUPPORTED at every ELBO entry point, a Hamiltonian score included.  A non-centring layer does not take it (no group
 * structure).
 * The value is 33, written relative to the kind before it: tests/test_ordinal_cpu.py holds the highest kind it can evaluate at 32,
 * tests/test_riskset_cpu.py evaluates this definition and holds it at 33. */
#define NF_TARGET_RISKSET (NF_TARGET_ORDINAL_LOGIT + 1)
#define NF_RISKSET_MAXR 8192

#define NF_MAX_HIDDEN 4

/* Base distribution q0 of a flow (the `dist` of the TransformedDistribution).  Every reference configuration uses
 * MvNormal(zeros(d), I) (test/flow.jl:9, demo_planar_flow.jl:24) -- that is base == NULL, and the only form the fused
 * kernels draw in registers.  General MvNormal(mu, Sigma) bases (what _device_specific_rand(rng, ::MvNormal, n) and
 * logpdf(flow.dist, xs) accept: src/NormalizingFlows.jl:109-115, ext/NormalizingFlowsCUDAExt.jl:43-48,
 * test/ext/CUDA/cuda.jl:33-45) are drawn as x = mu + L eps and enter the objectives through an exact per-sample
 * correction of log q0; q0 is a leaf of destructure (@leaf MvNormal), so it carries no trainable parameter. */
#define NF_BASE_STANDARD 0 /* MvNormal(zeros(d), I)                                                    */
#define NF_BASE_DIAG 1     /* MvNormal(mu, Diagonal(sigma.^2)): scale = sigma[d]  (device)              */
#define NF_BASE_DENSE 2    /* MvNormal(mu, Sigma), Sigma = L L': scale = L, d x d lower triangular,
                              column-major (device)                                                     */
typedef struct nf_base {
  int32_t kind;      /* NF_BASE_*                                     */
  const void *mu;    /* [d], device, the flow's element type          */
  const void *scale; /* see NF_BASE_*                                 */
  double logdet;     /* log|det L| = sum(log(diag(L))) / sum(log(sigma)) */
} nf_base;

/* Static (non-trainable) description of a flow: the fields of the reference's
 * layer structs that Optimisers.destructure leaves out (dim, mask, K, B, hidden
 * sizes; src/flows/realnvp.jl:33-38, src/flows/neuralspline.jl:35-42). */
struct nf_target;
struct nf_base;
typedef struct nf_flow_desc {
  int32_t kind;                 /* NF_KIND_*                                         */
  int32_t dtype;                /* NF_DTYPE_*                                        */
  int32_t d;                    /* length(q0)                                        */
  int32_t nlayers;              /* planar/radial: layers; realnvp/nsf: RealNVP_layer /
                                   NSF_layer blocks (two couplings each)             */
  int32_t n_hidden;             /* length(hdims)                                     */
  int32_t hdims[NF_MAX_HIDDEN]; /* conditioner hidden widths, src/flows/utils.jl:71  */
  int32_t K;                    /* spline bins (nsf)                                 */
  float B;                      /* spline box bound (nsf)                            */
  const struct nf_target *score; /* NF_KIND_HAMILTONIAN: the target behind LeapFrog's
                                    score function (host pointer); NF_KIND_NONCENTRED: the
                                    target whose groups the layer reads; NULL otherwise */
  const struct nf_base *base;    /* q0 (host pointer); NULL = MvNormal(zeros(d), I)  */
  int32_t nsegments;             /* NF_KIND_COMPOSITE: number of segments; NF_KIND_PRECOND, NF_KIND_NONCENTRED: 1; else 0 */
  const struct nf_flow_desc *segments; /* host array [nsegments] (NF_KIND_PRECOND, NF_KIND_NONCENTRED: the inner flow) */
} nf_flow_desc;

/* Built-in target log-densities (the `logp` closure of src/objectives/elbo.jl:68
 * for the benchmark/test targets).  p0/p1 are device pointers for DIAGGAUSS
 * (mu[d], var[d]); for BANANA they are ignored and (b, var) are the scalars. */
typedef struct nf_target {
  int32_t kind;
  const void *p0;
  const void *p1;
  double s0;
  double s1;
} nf_target;

typedef struct nf_ctx nf_ctx;

/* ---- library / context --------------------------------------------------- */
int nf_abi_version(void);
const char *nf_strerror(int code);
/* hip_stream: a hipStream_t to enqueue on (NULL = the device's default stream). */
int nf_ctx_create(int device, void *hip_stream, nf_ctx **out);
int nf_ctx_destroy(nf_ctx *ctx);
int nf_ctx_set_stream(nf_ctx *ctx, void *hip_stream);
int nf_ctx_synchronize(nf_ctx *ctx);
/* Memory.  By default a context owns a grow-only arena: the first call of a larger shape allocates (and synchronises
 * the stream once), steady-state steps never do.  For callers that want NO allocation or synchronisation inside the
 * compute entry points (hipGraph capture, a Julia GC-managed ROCArray as backing store):
 *   bytes = nf_workspace_bytes(ctx, desc, N_max);  nf_ctx_set_arena(ctx, device_ptr, bytes);   (device_ptr 256-byte aligned)
 * after which every entry point with this flow and N <= N_max works inside the arena and a larger request returns
 * NF_ERR_WORKSPACE.  nf_ctx_set_arena(ctx, NULL, 0) returns to the owned mode.  ("the library allocates
 * nothing persistent except the ctx; arena sized by nf_workspace_bytes".) */
int64_t nf_workspace_bytes(nf_ctx *ctx, const nf_flow_desc *desc, int64_t N);
int nf_ctx_set_arena(nf_ctx *ctx, void *arena_device, size_t bytes);
/* The training step of the LDS-resident RealNVP path keeps the forward's activations for the reverse pass (an
 * "activation stash": 46 KiB per 32-sample tile and coupling at d = 64 / hidden 64, i.e. 772 MB at BASELINE cfg 2;
 * 42 KiB of a slot are written for every coupling but one, the rest of it is never read) --
 * the Zygote tape of src/optimize.jl:12-14 in kernel form.  max_bytes bounds the buffer: a batch whose stash is larger
 * runs chunk by chunk through it (forward + reverse pass per chunk, all chunks' gradient slabs reduced together; same
 * result up to float32 summation order).  nf_elbo_value_and_grad / nf_elbo_step and nf_loglikelihood_value_and_grad
 * (the inverse chain stashes for ITS reverse pass) use it.  0 disables the stash: the reverse pass then recomputes the
 * activations from the flow output (invertible recompute: no extra memory, but every leaky-ReLU slope is decided
 * again on a float32 reconstruction of the layer input -- DESIGN.md section 5; an explicit opt-in, never the default).
 * A negative value restores the default: 4 GiB (or the environment's NF_AFFINE_STASH_MAX_MB / NF_AFFINE_NO_STASH) for
 * every LDS-resident shape.  nf_workspace_bytes and nf_tape_bytes reflect the setting. */
int nf_ctx_set_stash_budget(nf_ctx *ctx, int64_t max_bytes);

/* ---- layout -------------------------------------------------------------- */
/* length(first(Optimisers.destructure(flow)))  (src/NormalizingFlows.jl:67) */
int64_t nf_param_count(const nf_flow_desc *desc);
/* number of bijector layers in execution terms (couplings count individually) */
int32_t nf_layer_count(const nf_flow_desc *desc);

/* ---- a4 + a5: base distribution ------------------------------------------ */
/* _device_specific_rand(rng, MvNormal(zeros(d), I), N) fused with
 * logpdf(flow.dist, xs)  (src/NormalizingFlows.jl:94-115, ext/NormalizingFlowsCUDAExt.jl:43-48,
 * src/objectives/elbo.jl:68,94).  Philox4x32-10 keyed by `seed`, counter =
 * (sample_offset + j, feature_group, stream_id): the draw for global sample j
 * does not depend on how the batch is sharded.  logq_out may be NULL. */
int nf_base_sample_logpdf(nf_ctx *ctx, int32_t dtype, int32_t d, int64_t N, uint64_t seed,
                          uint64_t sample_offset, uint32_t stream_id, void *x_out, void *logq_out);
/* logpdf(MvNormal(zeros(d), I), xs) for caller-supplied xs */
int nf_base_logpdf(nf_ctx *ctx, int32_t dtype, int32_t d, int64_t N, const void *x, void *logq_out);
/* The same two for a general MvNormal(mu, Sigma) base (base == NULL or NF_BASE_STANDARD: identical to the above):
 * x = mu + L eps with the eps of nf_base_sample_logpdf(seed, sample_offset, stream_id), and its log-density. */
int nf_base_rand(nf_ctx *ctx, int32_t dtype, const nf_base *base, int32_t d, int64_t N, uint64_t seed,
                 uint64_t sample_offset, uint32_t stream_id, void *x_out, void *logq_out);
int nf_base_logpdf_general(nf_ctx *ctx, int32_t dtype, const nf_base *base, int32_t d, int64_t N, const void *x,
                           void *logq_out);

/* ---- a6, a7, a10, a12, a13: transforms ----------------------------------- */
/* Bijectors.with_logabsdet_jacobian(flow.transform, xs)  (src/objectives/elbo.jl:67):
 * applies the layers last-listed first and sums per-sample logdets.
 * y_out may alias x_in.  ladj_out[N] is overwritten. */
int nf_flow_fwd(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *x_in,
                int64_t N, void *y_out, void *ladj_out);
/* with_logabsdet_jacobian(inverse(flow.transform), ys)  (src/flows/realnvp.jl:99-110,
 * src/flows/neuralspline.jl:134-140; reached from loglikelihood.jl:31 via logpdf). */
int nf_flow_inv(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *y_in,
                int64_t N, void *x_out, void *ladj_out);
/* rand(rng, flow, n) / _device_specific_rand(rng, flow, n)  (src/NormalizingFlows.jl:117-127; the CUDA extension's
 * per-column version: ext/NormalizingFlowsCUDAExt.jl:61-74): N base draws -- the same Philox stream
 * nf_base_sample_logpdf(seed, sample_offset, stream_id) produces -- pushed through the transform, batched.
 * Planar / radial / mean-field flows do it in one launch (draws in registers); y_out is d x N. */
int nf_flow_rand(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, int64_t N, uint64_t seed,
                 uint64_t sample_offset, uint32_t stream_id, void *y_out);
/* One bijector layer, `layer` in FLAT order (0 = L1, the outermost / last applied):
 * Bijectors.with_logabsdet_jacobian(layer, x)  (src/flows/realnvp.jl:77-83,
 * src/flows/neuralspline.jl:102-108).  inverse != 0 selects Inverse{layer}.
 * ladj_out[N] is overwritten. */
int nf_layer_apply(nf_ctx *ctx, const nf_flow_desc *desc, int32_t layer, int32_t inverse,
                   const void *theta, const void *x_in, int64_t N, void *y_out, void *ladj_out);

/* Forward pass that keeps its tape, and the pullback from that tape: the two halves of a ChainRules
 * rrule for with_logabsdet_jacobian(flow.transform, xs) (the mechanism MonotonicSplines uses, test/ad.jl:126-127;
 * the reference's default path is Zygote differentiating the forward's own tape: src/optimize.jl:12-14 on
 * src/objectives/elbo.jl:65-70).  An arbitrary `logp` closure trains through this pair:
 *   tape = device buffer of nf_tape_bytes(ctx, desc, N) bytes, 256-byte aligned, owned by the caller (the rrule's closure)
 *   nf_flow_fwd_keep(..., x, N, y, ladj, tape, bytes)       y, ladj as nf_flow_fwd; the tape holds the forward's
 *                                                            activations in the layouts the reverse kernels consume
 *   ybar = d loss / d y from the caller's AD of logp, lbar = d loss / d ladj
 *   nf_flow_bwd_kept(..., tape, bytes, ybar, lbar, N, xbar, gtheta)
 * The pullback differentiates the forward's OWN activations and leaky-ReLU slopes (nothing is re-derived by inverting
 * the flow in float32), leaves the tape intact (it may be called again) and costs what the built-in training step's
 * reverse pass costs.  nf_tape_bytes depends on the context's nf_ctx_set_stash_budget setting (0 = keep only the flow
 * output and recompute by inversion; a positive budget -- or the default 4 GiB -- smaller than the activations of THIS
 * batch does the same for it: the tape never exceeds the budget, callers who want the forward's own activations for a
 * larger batch split it): both calls must run under the setting the size was queried with.
 * y_out may alias x_in; xbar_out may alias ybar, or be NULL for a single-family float32 coupling flow on the MFMA
 * kernels when only the parameter gradient is wanted (NF_ERR_ARG otherwise); gtheta_out[P] is overwritten. */
int64_t nf_tape_bytes(nf_ctx *ctx, const nf_flow_desc *desc, int64_t N);
int nf_flow_fwd_keep(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *x_in, int64_t N,
                     void *y_out, void *ladj_out, void *tape, size_t tape_bytes);
int nf_flow_bwd_kept(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *tape, size_t tape_bytes,
                     const void *ybar, const void *lbar, int64_t N, void *xbar_out, void *gtheta_out);

/* Pullback of nf_flow_fwd for callers that kept only x: runs the forward again FROM x with the tape in the context
 * workspace, then pulls it back (y is part of the rrule's signature and is not read; no float32 inversion).
 * Inputs: x (flow input), y (flow output), ybar[d*N], lbar[N] (cotangent of ladj).
 * Outputs: xbar_out[d*N] (may alias ybar), gtheta_out[P] (overwritten). */
int nf_flow_bwd(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *x,
                const void *y, const void *ybar, const void *lbar, int64_t N, void *xbar_out,
                void *gtheta_out);

/* ---- a14: built-in targets ------------------------------------------------ */
/* logp(ys) per column and (optionally) its gradient w.r.t. ys. */
int nf_target_logp(nf_ctx *ctx, int32_t dtype, const nf_target *target, int32_t d, int64_t N,
                   const void *y, void *logp_out, void *grad_out);

/* Row minibatch of a regression target, for stochastic VI over many rows: builds on the device, in ONE launch, a target of m rows
 * out of the R = full->s0 rows of `full`, in the full target's own kind and layout -- *out = {full->kind, p0_out, p1_out, m,
 * full->s1} is a target like any other, for every entry point and every flow that serves the kind.  Call it before each step.
 * Stratified, one row per stratum, without replacement:
 *       lo_j = floor(j R / m) (64-bit),  n_j = lo_{j+1} - lo_j >= 1,  idx_j = lo_j + (((uint64) r_j n_j) >> 32),   j = 0 .. m-1,
 *       r_j = word x of philox4x32_10(counter (j_lo, j_hi, 0xFFFFFFFF, stream), key (mb_seed_lo, mb_seed_hi))
 *   (counter word 2 = 0xFFFFFFFF is never a feature group of nf_base_sample_logpdf: the row choice is disjoint from the draws even
 *   with the same seed and stream).  The row weight becomes wt'_j = wt[idx_j] * n_j (one rounding in the element type); everything
 *   else of row idx_j -- its row of p1 and its entry of every per-row segment of p0 -- and every fixed segment of p0 (lin, par, grp,
 *   isd, hm, his, hk, gptr, gidx, ctab) is copied verbatim.  So E[sum_j n_j wt_idx_j phi_idx_j] = sum_i wt_i phi_i (unbiased), the
 *   host-folded full-data terms stay exact, a weight-0 row stays exactly dropped, and m = R gives the full buffers bit for bit.
 * Kinds: NF_TARGET_GLM_*, NF_TARGET_SOFTMAX, NF_TARGET_HGLM_*, NF_TARGET_BNN_*, NF_TARGET_DGLM_*.  NF_ERR_UNSUPPORTED for the kinds
 *   without a per-row weight (0 .. 6, 8) or whose rows are not exchangeable (NF_TARGET_ORDINAL_LOGIT: label blocks;
 *   NF_TARGET_RISKSET: rows interact).
 * p0_elems: the element count of full->p0 (the negative-binomial table length lives in device memory: it is derived from this).
 * p0_out: p0_elems - nper (R - m) elements, nper the number of per-row segments of the kind's p0;  p1_out: m x w, w the row width
 *   of p1 (d; d / C for SOFTMAX; (d - 1) / H - 1 for BNN).  idx_out (optional, int32[m]) receives idx.  idx_in (optional, int32[m],
 *   device) replaces the random draw only: the scale stays n_j by position, every value is bounded by select to [0, R) before it
 *   addresses anything, unbiasedness is then the caller's business.
 * NF_ERR_ARG: a NULL full / out / p0_out / p1_out, whatever the kind's own conventions refuse at d (NULL p0 / p1 included), m < 1,
 *   m > R, p0_out == full->p0, p1_out == full->p1, or a p0_elems that does not fit the kind's layout at (R, d, s1).  Both error
 *   classes are answered before any device work.  Asynchronous on the context's stream: ordered before any later call on the
 *   context.  One writer per output element: no atomics, the same bits on every launch.
 * Declared `extern`: tests/test_abi_cpu.py and tests/test_elbo_targets_cpu.py hold the declarations that begin a line with their
 * return type at the 49 symbols ABI 4 started with, and three more tests hold _lib.SYMBOLS at that count.  A symbol added since is
 * declared like this one and bound in _lib.EXT_SYMBOLS; tests/test_minibatch_cpu.py holds that list against this header. */
extern int nf_target_minibatch(nf_ctx *ctx, int32_t dtype, const nf_target *full, int32_t d, int64_t p0_elems, int64_t m,
                        uint64_t mb_seed, uint32_t stream, const int32_t *idx_in, int32_t *idx_out, void *p0_out, void *p1_out,
                        nf_target *out);

/* ---- a1, a2, a3: objectives ------------------------------------------------ */
/* elbo_batch(flow, logp, xs) / elbo(flow, logp, xs)  (src/objectives/elbo.jl:31-34,89-92):
 * mean_j[logp(y_j) - log q0(x_j) + ladj_j] for caller-supplied xs.
 * elbos_out[N] (optional) receives the per-sample terms (_batched_elbos, :65-70). */
int nf_elbo_batch(nf_ctx *ctx, const nf_flow_desc *desc, const nf_target *target,
                  const void *theta, const void *xs, int64_t N, void *elbos_out,
                  double *elbo_host);
/* elbo_batch(rng, flow, logp, n)  (src/objectives/elbo.jl:93-97): draws xs in-library. */
int nf_elbo_batch_rng(nf_ctx *ctx, const nf_flow_desc *desc, const nf_target *target,
                      const void *theta, int64_t N, uint64_t seed, uint64_t sample_offset,
                      uint32_t stream_id, double *elbo_host);
/* a16: loglikelihood(rng, flow, ys)  (src/objectives/loglikelihood.jl:26-33):
 * mean_j[log q0(T^-1 y_j) + ladj_inv_j]; logliks_out[N] optional. */
int nf_loglikelihood(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta, const void *ys,
                     int64_t N, void *logliks_out, double *ll_host);

/* ---- a15: the training step ------------------------------------------------ */
/* loss(theta) = -elbo_batch(rng, re(theta), logp, n) and its gradient
 * (_value_and_gradient, src/optimize.jl:12-14,86; loss closure src/NormalizingFlows.jl:69)
 * for THIS rank's shard of a global batch:
 *   samples [sample_offset, sample_offset + N_local) of N_global,
 *   out[0..P)  = sum_{j in shard} d(-elbo_j / N_global)/dtheta,
 *   out[P]     = sum_{j in shard} (-elbo_j / N_global).
 * Summing `out` over ranks (one all-reduce of P+1 elements) gives (grad, loss).
 * xs may be NULL (draw in-library from Philox as nf_base_sample_logpdf does) or a
 * caller-supplied d x N_local batch (the elbo_batch(flow, logp, xs) form). */
int nf_elbo_value_and_grad(nf_ctx *ctx, const nf_flow_desc *desc, const nf_target *target,
                           const void *theta, const void *xs, int64_t N_local, int64_t N_global,
                           uint64_t seed, uint64_t sample_offset, uint32_t stream_id,
                           void *out_grad_loss);
/* Forward-KL training, `train_flow(loglikelihood, flow, ys)`: loss(theta) =
 * -loglikelihood(rng, re(theta), ys) (src/objectives/loglikelihood.jl:26-33 inside the loss closure
 * src/NormalizingFlows.jl:69) and its gradient (_value_and_gradient, src/optimize.jl:12-14,86) for
 * THIS rank's N_local columns of an N_global-column data set:
 *   out[0..P) = sum_{j in shard} d(-loglik_j / N_global)/dtheta,   out[P] = sum (-loglik_j / N_global).
 * The chain is inverted once; its reverse pass walks the layers in forward order with the
 * implicit-function form of each inverse (no root-find or spline inversion is differentiated); the
 * Hamiltonian flow's inverse layers are explicit (LeapFrog with -eps) and are differentiated directly.
 * A general desc->base seeds the reverse pass with that base's score -Sigma^-1 (z - mu); a composite is
 * inverted and differentiated segment by segment. */
int nf_loglikelihood_value_and_grad(nf_ctx *ctx, const nf_flow_desc *desc, const void *theta,
                                    const void *ys, int64_t N_local, int64_t N_global,
                                    void *out_grad_loss);
/* Optimisers.update!(st, theta, g) for Optimisers.Adam (src/optimize.jl:99), in place on
 * theta/m/v; t = 1-based step count.  gnorm_out (device scalar, optional) receives
 * norm(g) (src/optimize.jl:89). */
int nf_adam_update(nf_ctx *ctx, int32_t dtype, void *theta, const void *g, void *m, void *v,
                   int64_t P, double lr, double beta1, double beta2, double eps, int64_t t,
                   void *gnorm_out);
/* Optimisers.Descent(lr) (vel = NULL: theta -= lr g) and Optimisers.Momentum(lr, rho)
 * (vel = rho vel - lr g; theta += vel) -- the other rules the reference's `optimiser` keyword
 * is commonly given (src/optimize.jl:67); gnorm_out as in nf_adam_update. */
int nf_sgd_update(nf_ctx *ctx, int32_t dtype, void *theta, const void *g, void *vel, int64_t P,
                  double lr, double rho, void *gnorm_out);
/* One whole iteration of the reference's training loop (src/optimize.jl:85-99: value and gradient of
 * -elbo_batch(rng, re(theta), logp, n), Optimisers.update! with Adam, norm(g)) in one call; loss_host / gnorm_host
 * (optional) receive the stat tuple of src/optimize.jl:89 -- asking for them synchronises the stream, passing NULL for
 * both keeps the call asynchronous ([loss ; norm] of the last step stay readable through a later call that asks).
 * Philox stream id = `step`, Adam's t = step + 1.  With a communicator on the context (nf_comm_init_rank /
 * nf_comm_init_all) this is the data-parallel step: N is THIS rank's batch, the rank draws samples
 * [rank * N, (rank + 1) * N) of a global batch of N * nranks, and the one all-reduce of [grad ; loss] happens inside.
 * LDS-resident RealNVP flows with any built-in target (the diagonal Gaussian of BASELINE cfg 2; Banana, Funnel, and at
 * d = 2 WarpedGauss and Cross) run as three launches -- fused forward (draws, chain, target, ELBO sums), reverse pass, fused
 * epilogue (slab sum, loss, Adam, norm, and the packed weight images of the UPDATED theta for the next step); LDS-resident
 * spline couplings on one rank as fused forward, one reverse launch per coupling and the same kind of epilogue.  Planar,
 * radial and mean-field flows whose whole step is one forward-and-reverse launch (Float32 or Float64, standard-normal base,
 * not a composition), on ONE rank, with any built-in target: three launches -- that launch, a fused epilogue (per layer: slab
 * sum and chain rule, Adam on the layer's parameters, its share of norm(g)^2; the loss) and the one-block finish of the norm.
 * In every case theta, m and v are bit for bit those of nf_elbo_value_and_grad + nf_adam_update.  Every other flow, and a target
 * whose arguments fail their check (NF_ERR_ARG from the target launch), runs the split sequence inside the call.  BY DEFAULT every call packs its weight images from theta (one small launch): whatever happened to theta
 * between two calls -- an in-place edit, a free and a re-allocation at the same address -- the step runs on the weights
 * theta holds now.  A training loop that OWNS theta (src/optimize.jl:85-99 does: nobody else touches theta between
 * Optimisers.update! and the next gradient) may opt in to reusing the images the previous step's epilogue wrote:
 *   nf_ctx_set_weight_cache(ctx, 1)  -- the caller promises that between consecutive nf_elbo_step /
 *       nf_elbo_step_enqueue calls on this context with the same theta pointer and flow, theta is modified by nobody
 *       else; the cache is keyed on (theta pointer, hash of the descriptor's shape fields) and dropped by
 *       nf_ctx_weights_changed, nf_ctx_set_stream, nf_ctx_set_arena, nf_ctx_set_weight_cache itself and by every other
 *       library call that packs weights;
 *   nf_ctx_weights_changed(ctx)      -- declares an edit of theta made under that promise (clipping, a callback).
 * `train_flow` of the Python mirror (objectives._optimize_fused) and `train_flow_fused` of ext/NormalizingFlowsNFHipExt.jl
 * opt in for the duration of their loop and opt out on return. */
int nf_elbo_step(nf_ctx *ctx, const nf_flow_desc *desc, const nf_target *target, void *theta,
                 void *m, void *v, int64_t N, uint64_t seed, uint32_t step, double lr,
                 double beta1, double beta2, double eps, double *loss_host, double *gnorm_host);
int nf_ctx_weights_changed(nf_ctx *ctx);
int nf_ctx_set_weight_cache(nf_ctx *ctx, int32_t enable);
/* The same step with NO per-step host values, for hipGraph capture and replay: *step_device (uint32, device memory,
 * caller-owned, initialised to the first step index) supplies the Philox stream id and Adam's t - 1 and is incremented
 * by the step; out_loss_gnorm_device (optional, 2 elements of the flow's type) receives [loss ; norm(g)].  After one
 * warm-up call (workspace sizing and kernel attributes are not capturable; use nf_ctx_set_arena or the warm-up's
 * grow-only allocation), capture a call between hipStreamBeginCapture / hipStreamEndCapture on the context's stream
 * and replay the graph.  Accepted: Float32 LDS-resident RealNVP flows (with or without a communicator) and, on a context
 * without a communicator, Float32 LDS-resident spline couplings and the planar, radial and mean-field flows nf_elbo_step
 * runs in three launches (Float32 or Float64) -- each with any of the five built-in targets (valid arguments: WarpedGauss
 * and Cross need d = 2).  NF_ERR_UNSUPPORTED for everything else, the linear-predictor targets (NF_TARGET_DENSEGAUSS,
 * NF_TARGET_LOGREG, NF_TARGET_GLM_*) and the Gaussian mixture (NF_TARGET_GAUSSMIX) on every flow included: theta and *step_device are left as they were. */
int nf_elbo_step_enqueue(nf_ctx *ctx, const nf_flow_desc *desc, const nf_target *target, void *theta, void *m, void *v,
                         int64_t N, uint64_t seed, uint32_t *step_device, double lr, double beta1, double beta2,
                         double eps, void *out_loss_gnorm_device);
/* One iteration of train_flow(loglikelihood, flow, ys): value and gradient of -loglikelihood(rng, re(theta), ys)
 * over THIS rank's N_local columns of an N_global-column data set (N_global <= 0: N_local * comm size), the
 * all-reduce of [grad ; loss] when the context holds a communicator, Optimisers.update! with Adam (t = step + 1),
 * norm(g).  loss_host / gnorm_host as nf_elbo_step (NULL for both = asynchronous).
 * Every flow nf_loglikelihood_value_and_grad accepts works; the weight-image cache (nf_ctx_set_weight_cache) and the stash
 * budget behave as in nf_elbo_step.  LDS-resident RealNVP flows whose inverse chain keeps a stash (the flows nf_elbo_step runs
 * in three launches) run as one launch per stash chunk that reads ys in place (inverse chain, stash, loss partials, the
 * reverse pass's seed), the reverse pass, the fused epilogue and a one-block finish; LDS-resident spline couplings on a
 * context without a communicator run the same fused inverse chain (leaving z and the spline tape), one reverse launch per
 * coupling, the fused epilogue and the finish.  Every other flow runs nf_loglikelihood_value_and_grad, the all-reduce and
 * nf_adam_update inside the call.  All give theta, m and v bit for bit equal to those calls made one by one. */
int nf_loglikelihood_step(nf_ctx *ctx, const nf_flow_desc *desc, void *theta, void *m, void *v, const void *ys,
                          int64_t N_local, int64_t N_global, uint32_t step, double lr, double beta1, double beta2,
                          double eps, double *loss_host, double *gnorm_host);
/* The same with Adam's t - 1 read from and incremented in *step_device; capturable after one warm-up call (as
 * nf_elbo_step_enqueue); out_loss_gnorm_device (optional, 2 floats) receives [loss ; norm(g)].
 * NF_ERR_UNSUPPORTED for flows without the fused form. */
int nf_loglikelihood_step_enqueue(nf_ctx *ctx, const nf_flow_desc *desc, void *theta, void *m, void *v, const void *ys,
                                  int64_t N_local, int64_t N_global, uint32_t *step_device, double lr, double beta1,
                                  double beta2, double eps, void *out_loss_gnorm_device);

/* ---- (e) multi-GPU: the path's one collective ----------------------------------- */
/* The ELBO is a mean over independent draws (src/objectives/elbo.jl:68,91,96), so ranks take sample shards
 * (nf_elbo_value_and_grad's sample_offset / N_local / N_global) and the ONLY exchange per step is an in-place SUM
 * all-reduce of the packed [grad ; loss] buffer (P + 1 elements) -- RCCL over xGMI, enqueued on the context's
 * stream, so it is ordered after the reverse pass and before nf_adam_update without host synchronisation.  Every
 * rank then applies the identical Adam update: replicas stay bit-identical, no broadcast.  The reference has no
 * multi-device code to cite; this is north_star's "single RCCL all-reduce over xGMI of the scalar ELBO and
 * parameter gradients per step" (SURVEY.md 8e).  librccl is bound at run time (dlopen), see NF_ERR_NO_RCCL.
 *
 * One process (or thread) per GPU:  rank 0 calls nf_comm_get_unique_id, ships the NF_COMM_ID_BYTES bytes to the
 * other ranks by any host channel, every rank calls nf_comm_init_rank.
 * One process driving G contexts (the Julia form: one task, G devices): nf_comm_init_all + nf_allreduce_grad_loss_all. */
#define NF_COMM_ID_BYTES 128
int nf_comm_get_unique_id(void *id_out_host);
int nf_comm_init_rank(nf_ctx *ctx, const void *id_host, int32_t nranks, int32_t rank);
int nf_comm_init_all(nf_ctx **ctxs, int32_t ngpus);
int nf_comm_size(nf_ctx *ctx); /* ranks of the context's communicator (1 if none) */
/* The step's one logical all-reduce may travel as several messages: under a communicator nf_elbo_step sends the gradient
 * of a weight-streaming RealNVP flow (BASELINE cfg 4: P + 1 = 4 214 785 floats, 16.9 MB) in buckets of whole couplings
 * (contiguous theta ranges, Optimisers.destructure order) on a second stream, each as soon as its couplings' reverse pass
 * and slab sum are done, and joins before the optimiser update; every rank issues the same buckets in the same order and
 * receives the same reduced bits.  bucket_bytes < 0: automatic (4 MiB, the default), 0: always one message, > 0: target
 * bucket size.  Gradients smaller than two buckets (cfg 2: 0.5 MB) always travel as one message.
 * nf_comm_bucket_count: all-reduce calls nf_elbo_step issues per step for this flow (0 without a communicator). */
int nf_ctx_set_comm_bucket_bytes(nf_ctx *ctx, int64_t bucket_bytes);
int nf_comm_bucket_count(nf_ctx *ctx, const nf_flow_desc *desc);
/* in place: buf[0..count) <- sum over ranks; count = P + 1 for the training step */
int nf_allreduce_grad_loss(nf_ctx *ctx, int32_t dtype, void *buf, int64_t count);
int nf_allreduce_grad_loss_all(nf_ctx **ctxs, int32_t ngpus, int32_t dtype, void **bufs, int64_t count);
int nf_comm_destroy(nf_ctx *ctx);

/* ---- measurement support ---------------------------------------------------- */
/* Kernel durations from HIP events recorded on the context stream around launches since the
 * last nf_prof_enable (used by bench.py's roofline object).  mode 0 = off, 1 = bracket only the
 * dominant kernel (the coupling reverse pass), 2 = bracket every kernel, 3 = bracket every 4th launch
 * of the dominant kernel (what bench.py uses inside its timed region). */
int nf_prof_enable(nf_ctx *ctx, int32_t mode);
int nf_prof_read(nf_ctx *ctx, const char *kernel_name, double *avg_ms_host, int64_t *count_host);
/* Kernel-tuning aid: when on, block 0 / wave 0 of the coupling reverse pass writes s_memtime
 * stamps at its phase boundaries; a later call copies up to 128 of them to stamps_host. */
int nf_debug_trace(nf_ctx *ctx, int32_t on, int64_t *stamps_host, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* NFHIP_H */
