"""The generalised linear-predictor form (NF_TARGET_GLM_*) in numpy, shared by test_glm_cpu.py and test_gpu_glm.py:

    log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) + lin . y - |y|^2 / (2 sigma^2) - d/2 log(2 pi sigma^2),   u = A y + off
    grad     = A' (wt o phi'(u)) + lin - y / sigma^2

evaluated from a target's own `A` and `p0` = lin | off | wt | par.  The functions are dtype-generic: float64 arrays give the
reference (scipy's log_ndtr / erfcx closed forms), float32 arrays are evaluated op by op in float32 -- the floor that
tests/parity.py's `floor=` takes.  The float32 probit follows the form the kernel uses (erfcx on the left tail, erfc on
the right)."""
import numpy as np
from scipy import special as sp

L2PI = float(np.log(2.0 * np.pi))
FAMILIES = ("logit", "probit", "poisson", "student", "normal")


def phi(family, u, par):
    """phi(u; par), phi'(u; par) element-wise, in u's dtype"""
    t = u.dtype.type
    if family == "logit":
        e = np.exp(-np.abs(u))
        return np.minimum(u, t(0)) - np.log1p(e), np.where(u >= 0, e, t(1)) / (t(1) + e)
    if family == "probit":
        if u.dtype == np.float64:
            lp = sp.log_ndtr(u)
            return lp, np.exp(-0.5 * u * u - 0.5 * L2PI - lp)
        neg = u < 0
        un, up = np.where(neg, u, t(0)), np.where(neg, t(0), u)
        tx = sp.erfcx(-un * t(np.sqrt(0.5)))
        c = t(0.5) * sp.erfc(up * t(np.sqrt(0.5)))
        lp = np.where(neg, t(-0.5) * un * un + np.log(t(0.5) * tx), np.log1p(-c))
        dp = np.where(neg, t(np.sqrt(2.0 / np.pi)) / tx, t(1.0 / np.sqrt(2.0 * np.pi)) * np.exp(t(-0.5) * up * up) / (t(1) - c))
        return lp, dp
    if family == "poisson":
        e = np.exp(u)
        return -e, -e
    if family == "student":
        nu = t(par)
        u2 = u * u
        return t(-0.5) * (nu + t(1)) * np.log1p(u2 / nu), -(nu + t(1)) * u / (nu + u2)
    assert family == "normal", family
    return t(-0.5) * u * u, -u


def split_p0(p0, d, rows):
    assert p0.shape == (d + 2 * rows + 2,), (p0.shape, d, rows)
    return p0[:d], p0[d:d + rows], p0[d + rows:d + 2 * rows], p0[d + 2 * rows:]


def logp_score(family, y, A, p0, sigma):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; A and p0 are cast to it"""
    t = y.dtype.type
    rows, d = A.shape
    A, p0 = A.astype(y.dtype), p0.astype(y.dtype)
    lin, off, wt, par = split_p0(p0, d, rows)
    u = A @ y + off[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        ph, dp = phi(family, u, par[0])
        live = (wt != 0)[:, None]
        ph = np.where(live, wt[:, None] * ph, t(0))  # a zero-weight row contributes exactly 0, whatever phi returns there
        dp = np.where(live, wt[:, None] * dp, t(0))
    pw = 0.0 if np.isinf(sigma) else 1.0 / sigma**2
    c = 0.0 if np.isinf(sigma) else -0.5 * d * (L2PI + 2.0 * np.log(sigma))
    lp = t(par[1] + t(c)) + ph.sum(0) + lin @ y - t(0.5 * pw) * (y * y).sum(0)
    return lp, A.T @ dp + lin[:, None] - t(pw) * y


def target_arrays(tgt):
    """a GLMTarget's own A and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 reference on the device's own (rounded) data; float32 y -> the float32 floor"""
    A, p0 = target_arrays(tgt)
    return lambda y: logp_score(tgt.family, y, A, p0, tgt.prior_sigma)
