"""The preconditioned coupling flow (NF_KIND_PRECOND) in numpy: y = mu + L T(x), T the oracle's RealNVP / NSF chain,
theta = [mu (d) ; L, d x d column-major ; theta_inner].  The oracle has no such kind, so this composes fullrank_ref's
fwd / inv / bwd with the oracle's flow_fwd(keep=True) / flow_bwd / flow_inv; test_precond_cpu.py validates it against
central differences.  Dtype-generic like both of its halves: float32 arrays are evaluated op by op in float32 -- the floor
tests/parity.py's `floor=` takes."""
import numpy as np

import fullrank_ref as fr
import nf_oracle as o


def head(d):
    """number of parameters of the full-rank layer"""
    return d + d * d


def split(spec, theta):
    """theta -> (theta_fr, theta_inner)"""
    h = head(spec.d)
    assert theta.shape == (h + o.param_count(spec),), (theta.shape, spec)
    return theta[:h], theta[h:]


def fwd(spec, theta, x, keep=False):
    """x (d, N) -> (y, ladj[, tape]); tape = (the inner chain's states, its output u)"""
    tf, ti = split(spec, theta)
    u, l1, states = o.flow_fwd(spec, ti, x, keep=True)
    y, l2 = fr.fwd(tf, u.astype(x.dtype))
    ladj = (l1 + l2).astype(x.dtype)
    return (y, ladj, (states, u)) if keep else (y, ladj)


def inv(spec, theta, y):
    """y (d, N) -> (x, ladj_inv): the full-rank layer's inverse first (it is the outermost)"""
    tf, ti = split(spec, theta)
    u, l2 = fr.inv(tf, y)
    x, l1 = o.flow_inv(spec, ti, u)
    return x, (l1 + l2).astype(y.dtype)


def layer(spec, theta, i, x):
    """the i-th bijector in flat order: 0 = Shift, 1 = Scale, 2... = the inner flow's layers"""
    d = spec.d
    tf, ti = split(spec, theta)
    mu, L = fr.split(tf, d)
    if i == 0:
        return x + mu[:, None], np.zeros(x.shape[1], dtype=x.dtype)
    if i == 1:
        return L @ x, np.full(x.shape[1], fr.logdet(L), dtype=x.dtype)
    return o._layer_fwd(spec, ti, o.layers_flat_order(spec)[i - 2], x)


def bwd(spec, theta, tape, ybar, lbar):
    """pullback from fwd's tape: cotangents ybar (d, N), lbar (N,) -> (xbar (d, N), gtheta (P,))"""
    tf, ti = split(spec, theta)
    states, u = tape
    ubar, g_fr = fr.bwd(tf, u, ybar, lbar)
    xbar, g_in = o.flow_bwd(spec, ti, states, ubar.astype(ybar.dtype), lbar)
    return xbar, np.concatenate([g_fr, g_in]).astype(theta.dtype)


def logpdf(spec, theta, y):
    x, li = inv(spec, theta, y)
    return (fr.std_normal_logpdf(x) + li).astype(y.dtype)


def elbos(spec, theta, x, target_fn):
    """per-sample log p(y) - log q0(x) + ladj; target_fn(y) -> (log p (N,), score (d, N))"""
    y, ladj = fwd(spec, theta, x)
    lp, _ = target_fn(y)
    return (lp - fr.std_normal_logpdf(x) + ladj).astype(x.dtype)


def neg_elbo_value_and_grad(spec, theta, x, target_fn, n_global=None):
    """(-sum_j elbo_j / N_global, its gradient with respect to theta)"""
    n = x.shape[1]
    ng = n if n_global is None else n_global
    t = x.dtype.type
    y, ladj, tape = fwd(spec, theta, x, keep=True)
    lp, sc = target_fn(y)
    e = lp - fr.std_normal_logpdf(x) + ladj
    _, g = bwd(spec, theta, tape, (-sc / t(ng)).astype(x.dtype), np.full(n, -1.0 / ng, dtype=x.dtype))
    loss = float(-e.sum(dtype=np.float64) / ng) if x.dtype == np.float64 else float(-(e.sum(dtype=x.dtype) / t(ng)))
    return loss, g


# ---- the cases of test_precond_cpu.py / test_gpu_precond.py -------------------------------------------------------------------
# name -> (inner spec, N): the smallest shapes at which each mechanism can fail
CASES = {
    "stash": (o.FlowSpec("realnvp", 5, 2, (32, 32)), 70),           # ragged diagonal block; activation-stash tape
    "spline": (o.FlowSpec("nsf", 32, 1, (32, 32), 8, 30.0), 65),    # exactly one block, three tiles; spline tape      
    "recompute": (o.FlowSpec("realnvp", 33, 1, (64,)), 65),         # one-row diagonal block; one hidden layer: recompute tape
    "wide": (o.FlowSpec("realnvp", 70, 1, (32, 32)), 40),           # three block rows; weight-streaming tape
    "envelope": (o.FlowSpec("realnvp", 256, 1, (128, 100)), 96),    # d = 256: 36 lower blocks
    "flat32": (o.FlowSpec("nsf", 6, 1, (64, 64), 8, 30.0), 70),     # Float32 on the general kernels: the standard layout
    "single": (o.FlowSpec("realnvp", 2, 1, (16, 16)), 1),           # a single sample
}
GRID_STRIDE_SPEC = o.FlowSpec("realnvp", 2, 1, (16, 16))            # N = 32 * compute units + 33: the loop over tiles


def inputs(spec, n, f64, nan_upper=True):
    """(theta (P,), x (d, n)) as float64 arrays holding the run's element type's values: [mu ; L] and x of
    fullrank_cases.inputs, the inner flow's parameters from the oracle's initialiser (seed 7)"""
    import fullrank_cases as fc

    tf, x = fc.inputs(spec.d, n, f64, nan_upper=nan_upper)
    ti = fc.rounded(o.init_params(spec, np.random.default_rng(7)), f64)
    return np.concatenate([tf, ti]), x


def upper_mask(spec):
    """boolean (P,): the entries of theta above the diagonal of L"""
    import fullrank_cases as fc

    return np.concatenate([fc.upper_mask(spec.d), np.zeros(o.param_count(spec), dtype=bool)])


def zero_upper(spec, theta):
    import fullrank_cases as fc

    h = head(spec.d)
    return np.concatenate([fc.zero_upper(theta[:h], spec.d), theta[h:]])
