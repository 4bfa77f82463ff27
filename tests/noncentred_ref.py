"""The non-centred flow (NF_KIND_NONCENTRED) in numpy: y = S(T(x)), T the inner flow -- the oracle's RealNVP / NSF chain or
fullrank_ref's full-rank family -- and S the non-centring layer over z = [beta (p) ; tau (G) (; lambda)],

    y_j = z_j exp(lam_j tau_g(j))  for j < p with g(j) = grp_j >= 0,   y_j = z_j otherwise,   ladj = sum_{j: g(j) >= 0} lam_j tau_g(j),

theta = [lam (p) ; theta_inner].  The oracle has no such kind, so this composes the inner references with the layer's formulas
(the way precond_ref.py is built); test_noncentred_cpu.py validates it against central differences.  Dtype-generic like its
parts: float32 arrays are evaluated op by op in float32 -- the floor tests/parity.py's `floor=` takes.  The lam_j of a
coefficient without a group is never used (np.where selects, it does not multiply): NaN there changes nothing."""
from dataclasses import dataclass

import numpy as np

import fullrank_ref as fr
import nf_oracle as o


@dataclass(frozen=True)
class Spec:
    """inner: an o.FlowSpec of kind realnvp / nsf, or of kind "fullrank" (d alone counts); grp: the p group indices (-1: none);
    G group log-scales; d = p + G (+ 1 for the dispersion form, whose last coordinate passes through); frozen: lam is not trained"""
    inner: o.FlowSpec
    grp: tuple
    G: int
    frozen: bool = False

    @property
    def d(self):
        return self.inner.d

    @property
    def p(self):
        return len(self.grp)


def fullrank_spec(d):
    return o.FlowSpec("fullrank", d, 1)


def groups(p, G):
    """every seventh coefficient under a fixed scale, the others dealt round-robin over the first max(G - 1, 1) groups: with
    G >= 2 the last group has no member.  p = 3, G = 2: [-1, 0, 0], groups of sizes 2 and 0."""
    return tuple(-1 if (j % 7 == 0 or G == 0) else j % max(G - 1, 1) for j in range(p))


# ---- the inner flow: one interface over the two references ---------------------------------------------------------------------------
def inner_params(g):
    return g.d + g.d * g.d if g.kind == "fullrank" else o.param_count(g)


def inner_layers(g):
    return 2 if g.kind == "fullrank" else len(o.layers_flat_order(g))


def inner_fwd(g, theta, x):
    """-> (u, ladj, tape)"""
    if g.kind == "fullrank":
        u, l = fr.fwd(theta, x)
        return u, l, x
    u, l, states = o.flow_fwd(g, theta, x, keep=True)
    return u.astype(x.dtype), l.astype(x.dtype), states


def inner_inv(g, theta, u):
    return fr.inv(theta, u) if g.kind == "fullrank" else o.flow_inv(g, theta, u)


def inner_bwd(g, theta, tape, ubar, lbar):
    if g.kind == "fullrank":
        return fr.bwd(theta, tape, ubar, lbar)
    return o.flow_bwd(g, theta, tape, ubar, lbar)


def inner_layer(g, theta, i, x):
    if g.kind != "fullrank":
        return o._layer_fwd(g, theta, o.layers_flat_order(g)[i], x)
    mu, L = fr.split(theta, g.d)
    if i == 0:
        return x + mu[:, None], np.zeros(x.shape[1], dtype=x.dtype)
    return L @ x, np.full(x.shape[1], fr.logdet(L), dtype=x.dtype)


# ---- the layer S ---------------------------------------------------------------------------------------------------------------------
def _terms(spec, lam, z):
    """(member (p,), lam_j tau_g(j) (p, N), tau_g(j) (p, N)); zeros where a coefficient has no group"""
    grp = np.asarray(spec.grp, dtype=np.int64)
    member = grp >= 0
    zero = np.zeros((spec.p, z.shape[1]), dtype=z.dtype)
    if spec.G == 0:
        return member, zero, zero
    tau = np.where(member[:, None], z[spec.p + np.maximum(grp, 0)], zero)
    lam0 = np.where(member, lam, z.dtype.type(0)).astype(z.dtype)
    return member, lam0[:, None] * tau, tau


def s_fwd(spec, lam, z, sign=1):
    """z (d, N) -> (y, ladj); sign = -1: the inverse (tau passes through, so it is read from the input either way)"""
    p, t = spec.p, z.dtype.type
    member, lt, _ = _terms(spec, lam, z)
    y = z.copy()
    y[:p] = np.where(member[:, None], z[:p] * np.exp(t(sign) * lt), z[:p])
    ladj = np.zeros(z.shape[1], dtype=z.dtype)
    for j in range(p):  # increasing j
        ladj = ladj + lt[j]
    return y, t(sign) * ladj


def s_bwd(spec, lam, z, y, ybar, lbar):
    """cotangents ybar (d, N), lbar (N,) at the layer's input z and its own output y -> (zbar (d, N), glam (p,))"""
    p = spec.p
    grp = np.asarray(spec.grp, dtype=np.int64)
    member, lt, tau = _terms(spec, lam, z)
    lam0 = np.where(member, lam, z.dtype.type(0)).astype(z.dtype)
    a = ybar[:p] * y[:p] + lbar[None, :]
    zbar = ybar.copy()
    zbar[:p] = np.where(member[:, None], ybar[:p] * np.exp(lt), ybar[:p])
    for j in range(p):  # increasing j
        if member[j]:
            zbar[p + grp[j]] = zbar[p + grp[j]] + lam0[j] * a[j]
    glam = np.where(member, (tau * a).sum(axis=1, dtype=z.dtype), z.dtype.type(0)).astype(z.dtype)
    return zbar, glam


# ---- the flow ------------------------------------------------------------------------------------------------------------------------
def param_count(spec):
    return spec.p + inner_params(spec.inner)


def layer_count(spec):
    return inner_layers(spec.inner) + 1


def split(spec, theta):
    assert theta.shape == (param_count(spec),), (theta.shape, spec)
    return theta[:spec.p], theta[spec.p:]


def fwd(spec, theta, x, keep=False):
    """x (d, N) -> (y, ladj[, tape]); tape = (the inner flow's tape, its output u, y)"""
    lam, ti = split(spec, theta)
    u, l1, tape = inner_fwd(spec.inner, ti, x)
    y, l2 = s_fwd(spec, lam, u)
    ladj = (l1 + l2).astype(x.dtype)
    return (y, ladj, (tape, u, y)) if keep else (y, ladj)


def inv(spec, theta, y):
    """y (d, N) -> (x, ladj_inv): S's inverse first (it is the outermost)"""
    lam, ti = split(spec, theta)
    u, l2 = s_fwd(spec, lam, y, sign=-1)
    x, l1 = inner_inv(spec.inner, ti, u)
    return x.astype(y.dtype), (l1 + l2).astype(y.dtype)


def layer(spec, theta, i, x):
    """the i-th bijector: the inner flow's layers in their flat order first, S the last"""
    lam, ti = split(spec, theta)
    if i == inner_layers(spec.inner):
        return s_fwd(spec, lam, x)
    return inner_layer(spec.inner, ti, i, x)


def bwd(spec, theta, tape, ybar, lbar):
    """pullback from fwd's tape -> (xbar (d, N), gtheta (P,)); a frozen lam's entries are 0"""
    lam, ti = split(spec, theta)
    inner_tape, u, y = tape
    ubar, glam = s_bwd(spec, lam, u, y, ybar, lbar)
    if spec.frozen:
        glam = np.zeros_like(glam)
    xbar, g_in = inner_bwd(spec.inner, ti, inner_tape, ubar.astype(ybar.dtype), lbar)
    return xbar, np.concatenate([glam, g_in]).astype(ybar.dtype)


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


# ---- inputs of test_noncentred_cpu.py / test_gpu_noncentred.py ----------------------------------------------------------------------
def rounded(a, f64):
    return a if f64 else a.astype(np.float32).astype(np.float64)


def inputs(spec, n, f64, lam=None, nan_fixed=False, seed=5):
    """(theta (P,), x (d, n)) as float64 arrays holding the run's element type's values: lam = 1 + 0.3 randn unless given (NaN at
    the coefficients without a group with nan_fixed), the inner flow's parameters from its reference's initialiser"""
    rng = np.random.default_rng(seed)
    g = spec.inner
    lam_ = (1.0 + 0.3 * rng.standard_normal(spec.p)) if lam is None else np.full(spec.p, float(lam))
    if nan_fixed:
        lam_ = np.where(np.asarray(spec.grp) < 0, np.nan, lam_)
    if g.kind == "fullrank":
        import fullrank_cases as fc

        ti, _ = fc.inputs(g.d, 1, True, nan_upper=False)
    else:
        ti = o.init_params(g, np.random.default_rng(7))
    x = rng.standard_normal((g.d, n))
    return rounded(np.concatenate([lam_, ti]), f64), rounded(x, f64)


def fixed_mask(spec):
    """boolean (P,): the lam entries of coefficients without a group"""
    return np.concatenate([np.asarray(spec.grp) < 0, np.zeros(inner_params(spec.inner), dtype=bool)])
