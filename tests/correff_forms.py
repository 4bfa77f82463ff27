"""The correlated-random-effects targets (NF_TARGET_CRE_*) as their DEFINITION, shared by test_correff_cpu.py and test_gpu_correff.py:
per level torch.distributions.MultivariateNormal(0, D R D) (through scale_tril = D L, the same distribution), per term
LKJCholesky(k, eta).log_prob(L) + CorrCholeskyTransform().log_abs_det_jacobian(omega, L), the hyper-priors as torch densities over
sigma = exp(tau) with their Jacobian, the likelihood's row functions, and the score by torch.autograd -- nothing of the kernel's
algebra (no W, no pullback, no closed-form LKJ exponent).  ref_of(case)(y): float64 y -> the float64 reference, float32 y -> the same
formula evaluated in float32, the floor tests/parity.py's `floor=` takes.  `packed_logp` evaluates the packed device layout in numpy."""
import math

import numpy as np
import torch
from torch.distributions import HalfCauchy, HalfNormal, LKJCholesky, MultivariateNormal, Normal
from torch.distributions.transforms import CorrCholeskyTransform

import glm_forms as gf
import hier_forms as hf

HYPERS = hf.HYPERS
# geometry: (p, [(k, G, eta, hypers)], rows)
GEOMETRIES = {
    "a": (2, [(2, 3, 2.5, ("halfcauchy", "lognormal"))], 40),                                # one ragged row block
    "b": (0, [(4, 9, 1.0, ("halfnormal",) * 4)], 37),                                        # the level loop wraps past q = 8; no fixed effects
    "c": (3, [(1, 5, 1.0, ("lognormal",)), (3, 4, 2.5, HYPERS)], 33),                        # k = 1 beside k = 3, every hyper family, two weight-0 rows
    "d": (5, [(4, 60, 2.0, ("halfnormal", "halfcauchy", "lognormal", "halfnormal"))], 64),  # d = 255: DB = 8, two feature chunks
}


def case(geo, family, f64, seed=5):
    """the host data of one test target, float32-representable when not f64 (so both element types see the same numbers)"""
    p, terms, rows = GEOMETRIES[geo]
    pa = p + sum(k * G for k, G, _, _ in terms)
    rng = np.random.default_rng(seed + 17 * pa + rows)
    r = (lambda a: a) if f64 else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    wt = rng.uniform(0.3, 2.5, rows)
    if geo == "c":
        wt[[4, 20]] = 0.0
    sig = rng.uniform(0.5, 2.0, p)
    if p > 1:
        sig[0] = np.inf
    tm = [(k, G, eta, list(h), r(0.3 * rng.standard_normal(k)).tolist(), r(rng.uniform(0.7, 1.8, k)).tolist()) for k, G, eta, h in terms]
    return dict(family=family, p=p, terms=tm, A=r(rng.standard_normal((rows, pa)) / np.sqrt(pa)), off=r(0.5 * rng.standard_normal(rows)), wt=r(wt),
                lin=r(0.5 * rng.standard_normal(pa)), const=0.75, param=3.0 if "student" in family else 0.0, sig=r(sig),
                disp=("halfnormal", 0.0, 1.25) if family[0] == "d" else None, d=pa + sum(k + k * (k - 1) // 2 for k, *_ in tm) + (family[0] == "d"))


def build(nf, c, dtype, device):
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device=device)
    dh = c["disp"] or ("halfcauchy", 0.0, 1.0)
    return nf.CorrelatedEffectsTarget(c["family"], t(c["A"]), [tuple(x) for x in c["terms"]], t(c["off"]), t(c["wt"]), t(c["lin"]), c["const"], c["param"],
                                      c["sig"].tolist(), dh[0], dh[1], dh[2])


def log_hyper(h, loc, scl, tau):
    """log density over tau of sigma = exp(tau) ~ h"""
    if h == "lognormal":
        return Normal(loc, scl).log_prob(tau)
    return (HalfNormal(scl) if h == "halfnormal" else HalfCauchy(scl)).log_prob(torch.exp(tau)) + tau


def phi(family, u, nu):
    fam = family.lstrip("d") if family in ("dnormal", "dstudent") else family
    if fam == "logit":
        return torch.nn.functional.logsigmoid(u)
    if fam == "poisson":
        return -torch.exp(u)
    if fam == "normal":
        return -0.5 * u * u
    assert fam == "student", family
    return -0.5 * (nu + 1.0) * torch.log1p(u * u / nu)


def logp(c, y):
    """y (d, N) torch -> log p (N,), every operation in y's dtype"""
    T = lambda v: torch.as_tensor(np.asarray(v), dtype=y.dtype)
    p, n = c["p"], y.shape[1]
    A, wt, lin = T(c["A"]), T(c["wt"]), T(c["lin"])
    coef, at = [y[:p]], p
    lp = torch.full((n,), c["const"], dtype=y.dtype)
    sig = T(c["sig"])
    for j in range(p):
        if math.isfinite(c["sig"][j]):
            lp = lp + Normal(0.0, sig[j]).log_prob(y[j])
    for k, G, eta, hyp, loc, scl in c["terms"]:
        b, tau, om = y[at:at + k * G], y[at + k * G:at + k * G + k], y[at + k * G + k:at + k * G + k + k * (k - 1) // 2]
        coef.append(b)
        at += k * G + k + k * (k - 1) // 2
        L = CorrCholeskyTransform()(om.T) if k > 1 else torch.ones(n, 1, 1, dtype=y.dtype)
        mvn = MultivariateNormal(torch.zeros(n, k, dtype=y.dtype), scale_tril=torch.exp(tau.T)[:, :, None] * L)
        lp = lp + mvn.log_prob(b.reshape(G, k, n).permute(0, 2, 1)).sum(0)
        if k > 1:
            lp = lp + LKJCholesky(k, T(eta)).log_prob(L) + CorrCholeskyTransform().log_abs_det_jacobian(om.T, L)
        for i in range(k):
            lp = lp + log_hyper(hyp[i], T(loc[i]), T(scl[i]), tau[i])
    u = A @ torch.cat(coef) + T(c["off"])[:, None]
    if c["disp"]:
        lam = y[-1]
        ph = phi(c["family"], u * torch.exp(-lam), c["param"]) - lam
        lp = lp + log_hyper(c["disp"][0], T(c["disp"][1]), T(c["disp"][2]), lam)
    else:
        ph = phi(c["family"], u, c["param"])
    return lp + torch.where(wt[:, None] > 0, wt[:, None] * ph, torch.zeros((), dtype=y.dtype)).sum(0) + lin @ torch.cat(coef)


def ref_of(c):
    def ref(y):
        yt = torch.tensor(np.ascontiguousarray(y), dtype=torch.float64 if y.dtype == np.float64 else torch.float32, requires_grad=True)
        lp = logp(c, yt)
        (g,) = torch.autograd.grad(lp.sum(), yt)
        return lp.detach().numpy().astype(y.dtype), g.numpy().astype(y.dtype)
    return ref


def packed_logp(tgt, y):
    """log p (N,) of y (d, N) from a target's own A and p0 = lin | off | wt | par[4] | fom | tab[4][24] | lamh[4], in numpy float64"""
    A, p0 = tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()
    rows, d = A.shape
    assert p0.shape == (2 * d + 2 * rows + 104,)
    lin, off, wt, par, fom = p0[:d], p0[d:d + rows], p0[d + rows:d + 2 * rows], p0[d + 2 * rows:d + 2 * rows + 4], p0[d + 2 * rows + 4:2 * d + 2 * rows + 4]
    tab, lamh = p0[2 * d + 2 * rows + 4:-4].reshape(4, 24), p0[-4:]
    u = A @ y + off[:, None]
    fam = tgt.family.lstrip("d") if tgt.disp else tgt.family
    ph = gf.phi(fam, u * np.exp(-y[-1]) if tgt.disp else u, par[0])[0]
    lp = par[1] + (wt[:, None] * ph).sum(0) + lin @ y - 0.5 * (fom[:, None] * y * y).sum(0)
    if tgt.disp:
        lp = lp + hf.hyper(int(lamh[0]), y[-1] - lamh[1], lamh[2])[0]
    for f in range(int(tgt.c.s1)):
        k, G, ib, it, io = (int(v) for v in tab[f, :5])
        tau, z = y[it:it + k], np.tanh(y[io:io + k * (k - 1) // 2])
        L, n = np.zeros((k, k) + y.shape[1:]), 0
        for i in range(k):
            rem = np.ones(y.shape[1])
            for j in range(i):
                L[i, j] = z[n] * np.sqrt(rem)
                rem = rem - L[i, j] ** 2
                lp = lp + tab[f, 5 + n] * np.log1p(-z[n] ** 2)
                n += 1
            L[i, i] = np.sqrt(rem)
            lp = lp - G * (tau[i] + np.log(L[i, i])) + hf.hyper(int(tab[f, 11 + i]), tau[i] - tab[f, 15 + i], tab[f, 19 + i])[0]
        for s in range(y.shape[1]):
            a = np.exp(-tau[:, s])[:, None] * y[ib:it, s].reshape(G, k).T
            lp[s] -= 0.5 * (np.linalg.solve(L[:, :, s], a) ** 2).sum()
    return lp
