"""The scaled-block GLM form (NF_TARGET_SCALEGLM) in numpy, shared by test_scaled_glm_cpu.py and test_gpu_scaled_glm.py:
    y = [beta (p) ; tau (S)],   u = A y + off,   z_i = exp(-tau_{s_b}) u_i   (s_b = -1: z = u)
    log p(y) = par[1] + sum_b sum_{i in b} wt_i phi_{f_b}(z_i; q_b) + lin . y - sum_j fom_j y_j^2 / 2 + sum_s h_s(tau_s - hm_s)
from a target's own `A` and `p0` = lin | off | wt | fam | bpar | sidx | fom | hm | his | hk | par, block b = rows [32 b, 32 b + 32).
float64 arrays give the reference, float32 arrays the floor that tests/parity.py's `floor=` takes.  `fixture` is the target both
test files use."""
import numpy as np

import glm_forms as gf
import mixed_forms as mf

HYPERS = ("lognormal", "halfnormal", "halfcauchy")
SEED = 29  # of the row data: the check rows' |z| stay >= 1e-3 at every (p, S, N, element type) test_gpu_scaled_glm.py evaluates


def layout(S):
    """(family, rows, param, scale) per component: six families; student and normal under scale 0 (their bins meet across waves); a check
    and a second normal run under scales of their own where S has room; three runs with no scale; the last scale has no block"""
    return (("normal", 40, 0.0, 0), ("logit", 33, 0.0, None), ("check", 7, 0.3, 1 if S > 2 else 0), ("student", 33, 3.0, 0),
            ("poisson", 31, 0.0, None), ("normal", 65, 0.0, S - 2 if S > 3 else 0), ("probit", 5, 0.0, None))


def fixture(nf, p, S, dtype=None, device="cpu", seed=SEED, edit=None):
    """one ScaledGLMTarget over mixed_forms.block_arrays (every fifth weight 0): lin 0.5 randn, const 0.7, fixed sigmas in [0.5, 2], the last
    coefficient flat, the three hyper-prior forms in turn.  `edit(i, A, off, wt)` may replace a component's arrays."""
    rng = np.random.default_rng(seed + p + 17 * S)
    comps, sof = [], []
    for i, (f, n, q, s) in enumerate(layout(S)):
        arrs = mf.block_arrays(f, p, n, seed + i)
        arrs = edit(i, *arrs) if edit else arrs
        comps.append(nf.GLMBlock(f, *(mf.tensor(a, dtype, device) for a in arrs), param=q, const=0.1 * i))
        sof.append(s)
    sig = rng.uniform(0.5, 2.0, p)
    sig[-1] = np.inf
    return nf.ScaledGLMTarget(comps, sof, S, lin=mf.tensor(0.5 * rng.standard_normal(p), dtype, device), const=0.7, fixed_sigma=sig.tolist(),
                              hyper=[HYPERS[s % 3] for s in range(S)], hyper_loc=rng.uniform(-0.5, 0.5, S).tolist(),
                              hyper_scale=rng.uniform(0.5, 2.0, S).tolist())


def split_p0(p0, d, R, S):
    B = R // 32
    assert R % 32 == 0 and p0.shape == (2 * d + 2 * R + 3 * B + 3 * S + 2,), (p0.shape, d, R, S)
    return np.split(p0, np.cumsum([d, R, R, B, B, B, d, S, S, S]))  # lin, off, wt, fam, bpar, sidx, fom, hm, his, hk, par


def hyper(kind, x, his):
    """h(x) and h'(x) at x = tau - hm: 0 log-normal, 1 half-normal, otherwise half-Cauchy (densities over tau)"""
    t = x.dtype.type
    if kind == 0:
        return t(-0.5) * (x * his) ** 2, -x * his * his
    if kind == 1:
        return t(-0.5) * np.exp(t(2) * x), -np.exp(t(2) * x)
    return -np.logaddexp(t(0), t(2) * x), t(-2) / (t(1) + np.exp(t(-2) * x))


def logp_score(y, A, p0, S, check_z=None):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; `check_z`: a list that receives the check-family rows' |z| of live rows"""
    t = y.dtype.type
    R, d = A.shape
    p = d - S
    A, p0 = A.astype(y.dtype), p0.astype(y.dtype)
    lin, off, wt, fam, bpar, sidx, fom, hm, his, hk, par = split_p0(p0, d, R, S)
    u = A @ y + off[:, None]
    lp, du, gtau = np.zeros(y.shape[1], y.dtype), np.zeros_like(u), np.zeros((S, y.shape[1]), y.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(R // 32):
            rows = slice(32 * b, 32 * b + 32)
            code = int(fam[b]) if 0 <= fam[b] < 6 else -1  # (NaN fails both comparisons)
            s = int(sidx[b]) if 0 <= sidx[b] < S else -1
            em = np.exp(-y[p + s]) if s >= 0 else np.ones(y.shape[1], y.dtype)
            z = u[rows] * em
            ph, dp = mf.phi(code, z, bpar[b])
            live = (wt[rows] != 0)[:, None]
            if code == 5 and check_z is not None:
                check_z.append(np.abs(z[wt[rows] != 0]))
            ph = np.where(live, wt[rows, None] * ph, t(0))  # a zero-weight row contributes exactly 0, whatever phi returns there
            dp = np.where(live, wt[rows, None] * dp, t(0))
            lp += ph.sum(0)
            du[rows] = dp * em
            if s >= 0:
                gtau[s] -= np.where(live, dp * z, t(0)).sum(0)
    grad = A.T @ du + lin[:, None] - fom[:, None] * y
    lp = par[1] + lp + lin @ y - t(0.5) * (fom[:, None] * y * y).sum(0)
    for s in range(S):
        hv, hd = hyper(hk[s], y[p + s] - hm[s], his[s])
        lp, grad[p + s] = lp + hv, grad[p + s] + gtau[s] + hd
    return lp, grad


def ref_of(tgt):  # ref(y): float64 y -> the reference on the device's own (rounded) data; float32 y -> the float32 floor
    A, p0 = gf.target_arrays(tgt)
    return lambda y, check_z=None: logp_score(y, A, p0, tgt.S, check_z)
