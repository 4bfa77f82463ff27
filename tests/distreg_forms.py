"""The distributional regression form (NF_TARGET_DR_*) in numpy, shared by test_distreg_cpu.py and test_gpu_distreg.py:
    y = [beta (p) ; gamma (q)],   u = X beta + offu,   v = Z gamma + offv,   A = [X | Z]
    log p(y) = par[1] + sum_i wt_i phi(u_i, v_i; a_i, par[3]) + lin . y - par[0] |beta|^2 / 2 - par[2] |gamma|^2 / 2
from a target's own `A` and `p0` = offu | offv | wt | aux | lin | par[4].  float64 arrays give the reference (the definition, through
np.logaddexp), float32 arrays are evaluated op by op in float32 in the order the kernels use: the floor tests/parity.py's `floor=` takes."""
import numpy as np

FAMILIES = ("normal", "student", "zipoisson", "weibull")
R = 166  # five full 32-row blocks and a ragged one: two waves of the tiled kernel take two blocks
NU = 3.0


def tensor(a, dtype=None, device="cpu"):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float64, device=device)


def _sig(x):  # log1p(exp(-|x|)), sigmoid(x), sigmoid(-x)
    t = x.dtype.type
    e = np.exp(-np.abs(x))
    r = t(1) / (t(1) + e)
    return np.log1p(e), np.where(x >= 0, r, e * r), np.where(x >= 0, e * r, r)


def phi(family, u, v, a, nu):
    """phi, d phi / d u, d phi / d v element-wise, in u's dtype; a: boolean"""
    t = u.dtype.type
    if family in ("normal", "student"):
        ei = np.exp(-v)
        z = u * ei
        if family == "normal":
            return t(-0.5) * z * z - v, -z * ei, z * z - t(1)
        nu, r = t(nu), t(1) / (t(nu) + z * z)
        return t(-0.5) * (nu + t(1)) * np.log1p(z * z * (t(1) / nu)) - v, -(nu + t(1)) * z * ei * r, (nu + t(1)) * (t(1) - nu * r) - t(1)
    if family == "zipoisson":
        m = np.exp(u)
        lv, sv, smv = _sig(v)
        lt, st, smt = _sig(v + m)
        sp = np.maximum(v, t(0)) + lv
        zero = (np.logaddexp(v, -m) - sp) if u.dtype == np.float64 else np.where(v > 0, t(0), np.maximum(v, -m)) + (lt - lv)
        return np.where(a, zero, -m - sp), np.where(a, -m * smt, -m), np.where(a, np.where(v >= 0, smv - smt, st - sv), -sv)
    assert family == "weibull", family
    ev = np.exp(v)
    w = u * ev
    ew, af = np.exp(w), a.astype(u.dtype)
    return af * (v + w) - ew, (af - ew) * ev, af + w * (af - ew)


def split_p0(p0, d, rows):
    assert p0.shape == (4 * rows + d + 4,), (p0.shape, d, rows)
    return np.split(p0, np.cumsum([rows, rows, rows, rows, d]))  # offu, offv, wt, aux, lin, par


def predictors(y, A, p0, p):
    rows, d = A.shape
    offu, offv = split_p0(p0.astype(y.dtype), d, rows)[:2]
    A = A.astype(y.dtype)
    return A[:, :p] @ y[:p] + offu[:, None], A[:, p:] @ y[p:] + offv[:, None]


def logp_score(family, y, A, p0, p):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; A and p0 are cast to it"""
    t = y.dtype.type
    rows, d = A.shape
    A, p0 = A.astype(y.dtype), p0.astype(y.dtype)
    offu, offv, wt, aux, lin, par = split_p0(p0, d, rows)
    with np.errstate(over="ignore", invalid="ignore"):
        u, v = predictors(y, A, p0, p)
        ph, du, dv = phi(family, u, v, (aux != 0)[:, None], par[3])
        live = (wt != 0)[:, None]  # a zero-weight row contributes exactly 0, whatever phi returns there
        ph, du, dv = (np.where(live, wt[:, None] * x, t(0)) for x in (ph, du, dv))
    pw = np.concatenate([np.full(p, par[0]), np.full(d - p, par[2])])[:, None]
    lp = par[1] + ph.sum(0) + lin @ y - t(0.5) * (pw * y * y).sum(0)
    return lp, np.concatenate([A[:, :p].T @ du, A[:, p:].T @ dv]) + lin[:, None] - pw * y


def target_arrays(tgt):
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):  # ref(y): float64 y -> the reference on the device's own (rounded) data; float32 y -> the float32 floor
    A, p0 = target_arrays(tgt)
    return lambda y: logp_score(tgt.family, y, A, p0, tgt.p)


def case_arrays(d, rows=R, seed=23):  # A randn / sqrt(d), offsets 0.5 randn, weights in [0.3, 2.5] with every fifth 0, aux random 0 / 1
    rng = np.random.default_rng(seed + 7 * d + rows)
    A, ou, ov = rng.standard_normal((rows, d)) / np.sqrt(d), 0.5 * rng.standard_normal(rows), 0.5 * rng.standard_normal(rows)
    wt, aux, lin = rng.uniform(0.3, 2.5, rows), rng.integers(0, 2, rows).astype(np.float64), 0.5 * rng.standard_normal(d)
    wt[2::5] = 0.0
    return A, ou, ov, wt, aux, lin


def make_target(nf, family, d, p, dtype=None, device="cpu", shift=(0.0, 0.0), arrays=None):
    """the general form over case_arrays (const 0.7, prior sigmas 2 and 3, nu = 3); `shift`: added to offu / offv with alternating sign.
    Weibull's Z is scaled by 0.2: with Z = randn / sqrt(d) and y = 1.5 randn, v = z . gamma + offv reaches 5.5 over 166 x 37 predictors
    and u 4, so exp(u exp(v)) = exp(980) is infinite in FLOAT64 -- there is nothing to compare with.  Under 0.2 Z, v stays below 2.8
    (offv alone reaches 1.7) and u exp(v) below float32's 88."""
    A, ou, ov, wt, aux, lin = arrays or case_arrays(d)
    if family == "weibull":
        A = np.hstack([A[:, :p], 0.2 * A[:, p:]])
    sg = np.where(np.arange(A.shape[0]) % 2 == 0, 1.0, -1.0)
    sg2 = np.where(np.arange(A.shape[0]) % 4 < 2, 1.0, -1.0)  # (so that all four sign pairs of the two shifts occur)
    tz = lambda a: tensor(a, dtype, device)  # noqa: E731
    return nf.DistributionalRegressionTarget(family, tz(A[:, :p]), tz(A[:, p:]), tz(ou + shift[0] * sg), tz(ov + shift[1] * sg2), tz(wt), tz(aux), tz(lin),
                                             const=0.7, param=NU if family == "student" else 0.0, prior_sigma=2.0, prior_sigma_aux=3.0)
