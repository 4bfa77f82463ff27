"""The full-rank Gaussian family (NF_KIND_FULLRANK) in numpy: y = mu + L x with L lower triangular,
ladj = sum_i log|L_ii|, theta = [mu(d) ; L as a d x d column-major matrix].  The oracle has no such kind, so this is
the reference of test_fullrank_cpu.py and test_gpu_fullrank.py.  The functions are dtype-generic: float64 arrays give the
reference, float32 arrays are evaluated op by op in float32 -- the floor tests/parity.py's `floor=` takes (as
glm_forms.py does).  The strict upper triangle of theta's matrix is never read (np.tril selects, it does not multiply)."""
import numpy as np
from scipy.linalg import solve_triangular

L2PI = float(np.log(2.0 * np.pi))


def split(theta, d):
    """theta -> (mu (d,), L (d, d) lower triangular) in theta's dtype"""
    assert theta.shape == (d + d * d,), (theta.shape, d)
    return theta[:d], np.tril(theta[d:].reshape(d, d).T)


def join(mu, L):
    """(mu, L) -> theta: the shift first, then L column-major"""
    return np.concatenate([mu, L.T.reshape(-1)])


def logdet(L):
    return np.log(np.abs(np.diag(L))).sum(dtype=L.dtype)


def fwd(theta, x):
    """x (d, N) -> (y (d, N), ladj (N,)); the shift is added to the product"""
    d, n = x.shape
    mu, L = split(theta, d)
    return L @ x + mu[:, None], np.full(n, logdet(L), dtype=x.dtype)


def inv(theta, y):
    """y (d, N) -> (x (d, N), ladj_inv (N,)) by forward substitution"""
    d, n = y.shape
    mu, L = split(theta, d)
    x = solve_triangular(L, y - mu[:, None], lower=True, check_finite=False).astype(y.dtype)
    return x, np.full(n, -logdet(L), dtype=y.dtype)


def bwd(theta, x, ybar, lbar):
    """pullback of fwd at x: cotangents ybar (d, N) of y and lbar (N,) of ladj -> (xbar (d, N), gtheta (P,)):
    xbar = L' ybar, g_mu = sum_j ybar_j, g_L = tril(ybar x') + (sum_j lbar_j) diag(1 / L_ii); zeros above the diagonal"""
    d, n = x.shape
    _, L = split(theta, d)
    gL = np.tril(ybar @ x.T) + lbar.sum(dtype=x.dtype) * np.diag(x.dtype.type(1) / np.diag(L))
    return L.T @ ybar, join(ybar.sum(axis=1, dtype=x.dtype), gL).astype(x.dtype)


def std_normal_logpdf(x):
    d = x.shape[0]
    return (x.dtype.type(-0.5 * d * L2PI) - x.dtype.type(0.5) * (x * x).sum(axis=0)).astype(x.dtype)


def elbos(theta, x, target_fn):
    """per-sample log p(y) - log q0(x) + ladj; target_fn(y) -> (log p (N,), score (d, N))"""
    y, ladj = fwd(theta, x)
    lp, _ = target_fn(y)
    return (lp - std_normal_logpdf(x) + ladj).astype(x.dtype)


def neg_elbo_value_and_grad(theta, x, target_fn, n_global=None):
    """(-mean elbo, its gradient): g_mu = -mean score, g_L = tril(-score x' / N) - diag(1 / L_ii)"""
    d, n = x.shape
    ng = n if n_global is None else n_global
    t = x.dtype.type
    y, ladj = fwd(theta, x)
    lp, sc = target_fn(y)
    e = lp - std_normal_logpdf(x) + ladj
    _, g = bwd(theta, x, (-sc / t(ng)).astype(x.dtype), np.full(n, -1.0 / ng, dtype=x.dtype))
    return float(-e.sum(dtype=np.float64) / ng) if x.dtype == np.float64 else float(-(e.sum(dtype=x.dtype) / t(ng))), g
