"""The ordinal (cumulative-logit) regression form (NF_TARGET_ORDINAL_LOGIT) in numpy, shared by test_ordinal_cpu.py and
test_gpu_ordinal.py:

    y = [beta (p) ; gamma (C - 1)],  c_1 = gamma_1,  c_k = c_{k-1} + exp(gamma_k),  eta_i = x_i . beta + off_i
    log p(y) = par[1] + sum_i wt_i ([k_i < C-1] log sigmoid(c_{k_i+1} - eta_i) + [k_i > 0] log sigmoid(eta_i - c_{k_i}))
               + sum_{k=1}^{C-2} n_k log1mexp(exp(gamma_{k+1})) - par[0]/2 |beta|^2 - par[2]/2 sum_k (c_k - par[3])^2 + sum_{k>=2} gamma_k
    g_i = wt_i ([k_i > 0] sigmoid(c_{k_i} - eta_i) - [k_i < C-1] sigmoid(eta_i - c_{k_i+1})),   d beta = X' g - par[0] beta
    d c_m = sum_i wt_i ([k_i = m-1] sigmoid(eta_i - c_m) - [k_i = m] sigmoid(c_m - eta_i)) - par[2] (c_m - par[3])
    d gamma_1 = sum_m d c_m,   d gamma_k = exp(gamma_k) sum_{m>=k} d c_m + n_{k-1} D / expm1(D) + 1,  D = exp(gamma_k)

(the FACTORED form the kernels evaluate) from a target's own label-blocked `X` [R, p] and `p0` = off[R] | wt[R] | lab[R/32] | par[4]
| nk[C].  `logp_score` is dtype-generic: float64 arrays give the reference, float32 arrays are evaluated op by op in float32 -- the
floor that tests/parity.py's `floor=` takes.  `unfactored_logp` is the definition log(sigmoid(a) - sigmoid(b)) itself, the
independent check: through mpmath at 50 digits where importable, else in float64 (only meaningful while |c - eta| <= 30).  `pack`
is the host packing written directly.  Also the inputs and the shapes of the tests: X ~ N(0, 1) / sqrt(p) rounded to float32 (no
intercept column: the cutpoints are the intercepts), labels uniform on 0..C-1, off ~ 0.3 N(0, 1), wt from {1, 1, 2, 0.5, 0}; prior
sigmas 2 (beta) and 3 (cutpoints, around 0.5); beta ~ 0.5 N(0, 1), gamma ~ s N(0, 1) with s in {0.5, 2}, float32-representable."""
import numpy as np

try:
    import mpmath
except ImportError:  # the float64 fallback of unfactored_logp
    mpmath = None

SIGMA_BETA, SIGMA_CUT, CUT_LOC = 2.0, 3.0, 0.5
WEIGHTS = (1.0, 1.0, 2.0, 0.5, 0.0)
GAMMA_SCALES = (0.5, 2.0)
# (C, p, rows)
SHAPES = [(2, 3, 33),      # d = 4: the smallest C
          (5, 4, 70),      # d = 8
          (5, 30, 40),     # d = 34: the gamma rows straddle the first 32-feature block
          (3, 30, 33),     # d = 32: the DB = 1 edge
          (5, 60, 133),    # d = 64
          (16, 6, 133),    # d = 21
          (4, 67, 40),     # d = 70
          (16, 241, 70)]   # d = 256: the widest
N_SIZES = (1, 33)  # one tile with one valid lane; two tiles with one valid lane in the second
LN2 = 0.6931471805599453


def dim(C, p):
    return p + C - 1


def split_p0(p0, R, C):
    nb = R // 32
    assert R % 32 == 0 and p0.shape == (2 * R + nb + 4 + C,), (p0.shape, R, C)
    return p0[:R], p0[R:2 * R], p0[2 * R:2 * R + nb], p0[2 * R + nb:2 * R + nb + 4], p0[2 * R + nb + 4:]


def log_sigmoid(u):
    """log sigmoid(u) = min(u, 0) - log1p(exp(-|u|)) ; sigmoid(-u), the forms of the logit row function"""
    e = np.exp(-np.abs(u))
    return np.minimum(u, 0) - np.log1p(e), np.where(u >= 0, e, 1) / (1 + e)


def log1mexp(D):
    """log(1 - exp(-D)) ; D / expm1(D) for D >= 0"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        val = np.where(D <= LN2, np.log(-np.expm1(-D)), np.log1p(-np.exp(-D)))
        return val, D / np.expm1(D)


def cutpoints(gam):
    """gamma [C - 1, N] -> (c [C - 1, N], exp(gamma_k) for k >= 2 [C - 2, N])"""
    with np.errstate(over="ignore"):
        e = np.exp(gam[1:])
    return np.cumsum(np.concatenate([gam[:1], e]), axis=0), e


def logp_score(y, X, p0, C):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; X and p0 are cast to it"""
    t = y.dtype.type
    R, p = X.shape
    d, N = y.shape
    nc = C - 1
    assert d == dim(C, p), (d, C, p)
    X, p0 = X.astype(y.dtype), p0.astype(y.dtype)
    off, wt, lab, par, nk = split_p0(p0, R, C)
    k = np.repeat(lab.astype(np.int64), 32)
    assert ((k >= 0) & (k < C)).all()
    beta, gam = y[:p], y[p:]
    c, e = cutpoints(gam)
    live, hasU, hasL = (wt != 0)[:, None], (k < nc)[:, None], (k > 0)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        eta = X @ beta + off[:, None]
        pu, du = log_sigmoid(c[np.minimum(k, nc - 1)] - eta)
        pl, dl = log_sigmoid(eta - c[np.maximum(k - 1, 0)])
        ph = np.where(hasU, pu, t(0)) + np.where(hasL, pl, t(0))
        lik = np.where(live, wt[:, None] * ph, t(0)).sum(0)   # a zero-weight row contributes exactly 0, whatever it holds
        au = np.where(live & hasU, wt[:, None] * du, t(0))
        al = np.where(live & hasL, wt[:, None] * dl, t(0))
        g = np.where(live, wt[:, None] * (np.where(hasL, dl, t(0)) - np.where(hasU, du, t(0))), t(0))
        Xl = np.where(live, X, t(0))                          # (0 * a non-finite x would be NaN in numpy; the row is dropped)
    dev = c - par[3]
    dc = np.stack([au[k == m - 1].sum(0) - al[k == m].sum(0) for m in range(1, C)]) - par[2] * dev
    suffix = np.cumsum(dc[::-1], axis=0)[::-1]
    lv, ld = log1mexp(e)
    n = nk[1:nc][:, None]
    table = np.where(n != 0, n * lv, t(0))
    lp = par[1] + lik + table.sum(0) - t(0.5) * par[0] * (beta * beta).sum(0) - t(0.5) * par[2] * (dev * dev).sum(0) + gam[1:].sum(0)
    with np.errstate(over="ignore", invalid="ignore"):
        ggam = np.concatenate([suffix[:1], e * suffix[1:] + np.where(n != 0, n * ld, t(0)) + t(1)])
    return lp.astype(y.dtype), np.concatenate([Xl.T @ g - par[0] * beta, ggam]).astype(y.dtype)


def unfactored_logp(y, X, p0, C):
    """the definition: par[1] + sum_i wt_i log(sigmoid(c_{k_i+1} - eta_i) - sigmoid(c_{k_i} - eta_i)) + priors + Jacobian, float64 out"""
    R, p = X.shape
    off, wt, lab, par, nk = split_p0(p0, R, C)
    k = np.repeat(lab.astype(np.int64), 32)
    out = np.empty(y.shape[1])
    if mpmath is None:
        c, _ = cutpoints(y[p:])
        eta = X @ y[:p] + off[:, None]
        sig = lambda u: 1.0 / (1.0 + np.exp(-u))
        hi = np.where((k < C - 1)[:, None], sig(c[np.minimum(k, C - 2)] - eta), 1.0)
        lo = np.where((k > 0)[:, None], sig(c[np.maximum(k - 1, 0)] - eta), 0.0)
        lik = np.where((wt != 0)[:, None], wt[:, None] * np.log(hi - lo), 0.0).sum(0)
        dev = c - par[3]
        return par[1] + lik - 0.5 * par[0] * (y[:p] ** 2).sum(0) - 0.5 * par[2] * (dev * dev).sum(0) + y[p + 1:].sum(0)
    with mpmath.workdps(50):
        mp = mpmath.mpf
        sig = lambda u: 1 / (1 + mpmath.exp(-u))
        for j in range(y.shape[1]):
            gam = [mp(float(v)) for v in y[p:, j]]
            c = [gam[0]]
            for v in gam[1:]:
                c.append(c[-1] + mpmath.exp(v))
            acc = mp(float(par[1]))
            for i in np.nonzero(wt != 0)[0]:
                eta = mpmath.fsum(mp(float(a)) * mp(float(b)) for a, b in zip(X[i], y[:p, j])) + mp(float(off[i]))
                hi = sig(c[k[i]] - eta) if k[i] < C - 1 else mp(1)
                lo = sig(c[k[i] - 1] - eta) if k[i] > 0 else mp(0)
                acc += mp(float(wt[i])) * mpmath.log(hi - lo)
            acc -= mp(float(par[0])) / 2 * mpmath.fsum(mp(float(b)) ** 2 for b in y[:p, j])
            acc -= mp(float(par[2])) / 2 * mpmath.fsum((cm - mp(float(par[3]))) ** 2 for cm in c)
            acc += mpmath.fsum(gam[1:])
            out[j] = float(acc)
    return out


def pack(X, lab, off, wt, C, sigma_beta=SIGMA_BETA, sigma_cut=SIGMA_CUT, cut_loc=CUT_LOC, const=0.0):
    """the host packing written directly, float64: rows sorted by label (stably), every label padded to whole 32-row blocks with
    rows of weight 0 -> (X [R, p], p0)"""
    rows, p = X.shape
    lab = np.asarray(lab, dtype=np.int64)
    Xs, os_, ws, bl = [], [], [], []
    for k in range(C):
        idx = np.nonzero(lab == k)[0]
        pad = -len(idx) % 32
        Xs += [X[idx], np.zeros((pad, p))]
        os_ += [off[idx], np.zeros(pad)]
        ws += [wt[idx], np.zeros(pad)]
        bl += [float(k)] * ((len(idx) + pad) // 32)
    c, prec = const, []
    for s, n in ((sigma_beta, p), (sigma_cut, C - 1)):
        prec.append(0.0 if np.isinf(s) else 1.0 / s**2)
        c += 0.0 if np.isinf(s) else -0.5 * n * np.log(2.0 * np.pi * s**2)
    nk = np.array([wt[lab == k].sum() for k in range(C)])
    return np.concatenate(Xs), np.concatenate(os_ + ws + [bl, [prec[0], c, prec[1], cut_loc], nk])


def target_arrays(tgt):
    """an OrdinalRegressionTarget's own X and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 reference on the device's own (rounded) data; float32 y -> the float32 floor"""
    X, p0 = target_arrays(tgt)
    return lambda y: logp_score(y, X, p0, tgt.n_categories)


def arrays(C, p, rows, seed=5):
    """X (float32-representable), labels, off, wt of one case, float64"""
    rng = np.random.default_rng(seed + 1000 * C + 7 * p + rows)
    X = (rng.standard_normal((rows, p)) / np.sqrt(p)).astype(np.float32).astype(np.float64)
    lab = rng.integers(0, C, rows)
    off = (0.3 * rng.standard_normal(rows)).astype(np.float32).astype(np.float64)
    wt = rng.choice(np.array(WEIGHTS), rows)
    return X, lab, off, wt


def sample_ys(C, p, n, gscale, seed=1):
    """beta ~ 0.5 N(0, 1), gamma ~ gscale N(0, 1), float32-representable, (d, n)"""
    d = dim(C, p)
    y = np.random.default_rng(seed + d + n + int(10 * gscale)).standard_normal((d, n))
    y[:p] *= 0.5
    y[p:] *= gscale
    return y.astype(np.float32).astype(np.float64)
