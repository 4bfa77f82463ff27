"""Inputs of the full-rank Gaussian family's tests, shared by test_fullrank_cpu.py (which checks their conditioning) and
test_gpu_fullrank.py (which runs them): generator seed 5, everything rounded through float32 for the Float32 runs.

    mu = 0.5 randn(d)
    L  = tril(0.1 randn(d, d) / sqrt(d), -1) + diag(exp(0.1 randn(d))), entry (d // 2, d // 2) negated
    x  = randn(d, N)

and the targets' data as numpy arrays with their closed forms (dtype-generic: ref(y) -> (log p, score))."""
import numpy as np

import glm_forms as gf
import nf_oracle as o
from test_mixture_cpu import cast_pack, mixture_logp_score, pack_mixture, random_mixture

L2PI = float(np.log(2.0 * np.pi))

# (d, N): the smallest shapes at which each mechanism can fail
SHAPES = [
    (1, 33),     # degenerate block; the second tile holds one sample
    (5, 70),     # ragged diagonal block; three tiles
    (32, 32),    # exactly one block, one full tile
    (33, 65),    # an off-diagonal block, a one-row diagonal block
    (70, 40),    # three block rows; waves with unequal block counts
    (256, 96),   # the envelope: 36 lower blocks
    (2, 1),      # a single sample
]
# d = 2 with more than 32 samples per workgroup of the Float32 reverse kernel (one workgroup per compute unit at most, 256
# of them on the MI355X): the kernel walks its tiles in a grid-stride loop
GRID_STRIDE_D, GRID_STRIDE_CUS = 2, 256
GRID_STRIDE_N = 32 * GRID_STRIDE_CUS + 33


def rounded(a, f64):
    return a if f64 else a.astype(np.float32).astype(np.float64)


def inputs(d, n, f64, nan_upper=True):
    """(theta (P,), x (d, n)) as float64 arrays holding the run's element type's values"""
    rng = np.random.default_rng(5)
    mu = 0.5 * rng.standard_normal(d)
    L = np.tril(0.1 * rng.standard_normal((d, d)) / np.sqrt(d), -1) + np.diag(np.exp(0.1 * rng.standard_normal(d)))
    L[d // 2, d // 2] = -L[d // 2, d // 2]
    x = rng.standard_normal((d, n))
    if nan_upper:
        L[np.triu_indices(d, 1)] = np.nan
    theta = np.concatenate([mu, L.T.reshape(-1)])
    return rounded(theta, f64), rounded(x, f64)


def zero_upper(theta, d):
    """theta with the strict upper triangle of its matrix set to 0"""
    th = theta.copy()
    M = th[d:].reshape(d, d)  # M[k, i] = L[i, k]
    M[np.tril_indices(d, -1)] = 0.0
    return th


def upper_mask(d):
    """boolean (P,): the entries of theta above the diagonal of L"""
    m = np.zeros((d, d), dtype=bool)
    m[np.tril_indices(d, -1)] = True  # (column-major storage: [k, i] with k > i)
    return np.concatenate([np.zeros(d, dtype=bool), m.reshape(-1)])


# ---- targets ---------------------------------------------------------------------------------------------------------------------
def glm_rows(d):
    return 300 if d == 256 else 45


def target_names(d, f64):
    names = ["diaggauss"]
    if d >= 2:
        names.append("funnel")
    names += ["mvnormal", "glm_logit", "glm_poisson"]
    if d <= 64:
        names.append("mixture3")
    return names


def diag_arrays(d):
    """mean 1.5 + 0.3 randn: away from q's own mean, so that the loss (a KL divergence) is not a difference near zero, where
    a relative criterion measures cancellation and not the arithmetic"""
    rng = np.random.default_rng(17 + d)
    return 1.5 + 0.3 * rng.standard_normal(d), rng.uniform(0.5, 1.5, d)


def gauss_arrays(d, seed=11):
    """the dense Gaussian of test_gpu_linpred.make_gauss: Sigma = Q diag(lambda) Q', lambda in [0.5, 2]"""
    rng = np.random.default_rng(seed + d)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = rng.uniform(0.5, 2.0, d)
    Sigma = (Q * lam) @ Q.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    return 0.5 * rng.standard_normal(d), Sigma


def glm_arrays(family, d):
    """rows = 45 (300 at d = 256), data rows randn / sqrt(d) (x 0.5 for poisson), a zero weight on every 7th row"""
    rows = glm_rows(d)
    rng = np.random.default_rng(23 + d + (0 if family == "logit" else 1))
    A = rng.standard_normal((rows, d)) / np.sqrt(d) * (0.5 if family == "poisson" else 1.0)
    wt = np.ones(rows)
    wt[::7] = 0.0
    return A, wt


def gauss_logp_score(y, mu, W, logdet_w):
    d = y.shape[0]
    u = W @ (y - mu[:, None])
    return y.dtype.type(-0.5 * d * L2PI + logdet_w) - y.dtype.type(0.5) * (u * u).sum(0), -(W.T @ u)


def numpy_target(name, d, f64):
    """ref(y) -> (log p, score) from numpy data alone (the device tests build theirs from the device targets' own arrays)"""
    if name == "diaggauss":
        mu, var = (rounded(a, f64) for a in diag_arrays(d))
        return lambda y: (o.target_logp(("diaggauss", mu.astype(y.dtype), var.astype(y.dtype)), y),
                          o.target_grad(("diaggauss", mu.astype(y.dtype), var.astype(y.dtype)), y))
    if name == "funnel":
        return lambda y: (o.target_logp(("funnel", 0.0, 3.0), y), o.target_grad(("funnel", 0.0, 3.0), y))
    if name == "mvnormal":
        mu, Sigma = gauss_arrays(d)
        Lc = np.linalg.cholesky(Sigma)
        W = rounded(np.tril(np.linalg.solve(Lc, np.eye(d))), f64)
        mu = rounded(mu, f64)
        ld = -np.log(np.diag(Lc)).sum()
        return lambda y: gauss_logp_score(y, mu.astype(y.dtype), W.astype(y.dtype), ld)
    if name.startswith("glm_"):
        family = name[4:]
        A, wt = glm_arrays(family, d)
        rows = A.shape[0]
        A = rounded(A, f64)
        p0 = np.concatenate([np.zeros(d), np.zeros(rows), wt, [0.0, 0.0]])
        return lambda y: gf.logp_score(family, y, A, p0, 2.0)
    assert name == "mixture3", name
    pack = cast_pack(pack_mixture(*random_mixture(d, 3)), np.float64)
    pack = tuple(rounded(a, f64) for a in pack)
    return lambda y: mixture_logp_score(y, *cast_pack(pack, y.dtype))
