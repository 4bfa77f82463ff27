"""The mixed-family GLM form (NF_TARGET_MIXGLM) in numpy, shared by test_mixed_glm_cpu.py and test_gpu_mixed_glm.py:
    log p(y) = par[1] + sum_b sum_{i in b} wt_i phi_{f_b}(u_i; q_b) + lin . y - |y|^2 / (2 sigma^2),   u = A y + off
    grad     = A' (wt o phi') + lin - y / sigma^2
from a target's own `A` and `p0` = lin | off | wt | fam | bpar | par, block b = rows [32 b, 32 b + 32).  Codes 0 .. 4: glm_forms.phi's
families, 5: the check function, any other drops its block.  float64 arrays give the reference, float32 arrays the floor that
tests/parity.py's `floor=` takes.  `six_families` is the target both test files use."""
import numpy as np

import glm_forms as gf

FAMILIES = gf.FAMILIES + ("check",)
COUNTS = (("logit", 1, 0.0), ("probit", 33, 0.0), ("poisson", 31, 0.0), ("student", 32, 3.0), ("normal", 65, 0.0), ("check", 7, 0.3),
          ("student", 5, 7.5))  # the six families' row counts, and a second Student run with another nu
SEED = 19  # of the row data: the check rows' |u| stay >= 1e-3 at every (d, N, element type) test_gpu_mixed_glm.py evaluates


def tensor(a, dtype=None, device="cpu"):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float64, device=device)


def block_arrays(family, d, rows, seed):  # one run's rows: A randn / sqrt(d), offsets 0.5 randn, weights in [0.3, 2.5], every fifth 0
    rng = np.random.default_rng(seed + 7 * d + rows + 131 * FAMILIES.index(family))
    A, off, wt = rng.standard_normal((rows, d)) / np.sqrt(d), 0.5 * rng.standard_normal(rows), rng.uniform(0.3, 2.5, rows)
    if rows > 1:
        wt[2::5] = 0.0
    return A, off, wt


def six_families(nf, d, dtype=None, device="cpu", counts=COUNTS, seed=SEED):
    # one MixedGLMTarget over `counts` (handed over in REVERSE order: the host sorts), lin 0.5 randn, const 0.7, prior sigma 2
    blocks = [nf.GLMBlock(f, *(tensor(a, dtype, device) for a in block_arrays(f, d, n, seed + i)), param=q, const=0.1 * i)
              for i, (f, n, q) in enumerate(counts)]
    lin = 0.5 * np.random.default_rng(seed + d).standard_normal(d)
    return nf.MixedGLMTarget(blocks[::-1], lin=tensor(lin, dtype, device), const=0.7, prior_sigma=2.0)


def phi(code, u, q):
    t = u.dtype.type
    if 0 <= code < 5:
        return gf.phi(gf.FAMILIES[code], u, q)
    if code == 5:
        s = t(q) - (u < 0).astype(u.dtype)
        return -u * s, -s
    return np.zeros_like(u), np.zeros_like(u)


def split_p0(p0, d, R):
    B = R // 32
    assert R % 32 == 0 and p0.shape == (d + 2 * R + 2 * B + 2,), (p0.shape, d, R)
    cut = np.cumsum([d, R, R, B, B])
    return np.split(p0, cut)  # lin, off, wt, fam, bpar, par


def logp_score(y, A, p0, sigma, check_u=None):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; `check_u`: a list that receives the check-family rows' |u| of live rows"""
    t = y.dtype.type
    R, d = A.shape
    A, p0 = A.astype(y.dtype), p0.astype(y.dtype)
    lin, off, wt, fam, bpar, par = split_p0(p0, d, R)
    u = A @ y + off[:, None]
    ph, dp = np.zeros_like(u), np.zeros_like(u)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(R // 32):
            rows = slice(32 * b, 32 * b + 32)
            code = int(fam[b]) if 0 <= fam[b] < 6 else -1  # (NaN fails both comparisons)
            ph[rows], dp[rows] = phi(code, u[rows], bpar[b])
            if code == 5 and check_u is not None:
                check_u.append(np.abs(u[rows][wt[rows] != 0]))
        live = (wt != 0)[:, None]
        ph = np.where(live, wt[:, None] * ph, t(0))  # a zero-weight row contributes exactly 0, whatever phi returns there
        dp = np.where(live, wt[:, None] * dp, t(0))
    pw = 0.0 if np.isinf(sigma) else 1.0 / sigma**2
    lp = par[1] + ph.sum(0) + lin @ y - t(0.5 * pw) * (y * y).sum(0)
    return lp, A.T @ dp + lin[:, None] - t(pw) * y


def ref_of(tgt):  # ref(y): float64 y -> the reference on the device's own (rounded) data; float32 y -> the float32 floor
    A, p0 = gf.target_arrays(tgt)
    return lambda y, check_u=None: logp_score(y, A, p0, tgt.prior_sigma, check_u)
