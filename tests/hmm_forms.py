"""The hidden-Markov-model form (NF_TARGET_HMM_*) in numpy, shared by test_hmm_cpu.py and test_gpu_hmm.py: a LOG-SPACE forward-backward
with scipy's logsumexp over explicit K x K arrays -- on purpose another formulation than the kernels' scaled recursion --
    y = [iota (K) ; Lambda (K x K) ; emission block (E x K)],   log p(y) = par[1] + sum_sequences log L(y) - sum_j ((y_j - pm_j) pis_j)^2 / 2
from a target's own `p0` = x | off | wt | seg and `A` = pm | pis | par.  float64 arrays give the reference, float32 arrays the floor
that tests/parity.py's `floor=` takes.  `fixture` is the target both test files use."""
import numpy as np
from scipy.special import logsumexp

import glm_forms as gf

SEED = 41
E_OF = {"normal": 2, "poisson": 1, "bernoulli": 1}


def emissions(family, em, x, off, wt):
    """l (R, K, N) = wt logf and [wt dlogf / d parameter] per emission parameter; rows of weight 0 give exactly 0, whatever x holds"""
    t = em.dtype.type
    live = (wt != 0)[:, None, None]
    x, o, w = np.where(wt != 0, x, t(0))[:, None, None], off[:, None, None], wt[:, None, None]
    if family == "normal":
        einv = np.exp(-em[1])
        z = (x - o - em[0]) * einv
        lf, dl = t(-0.5) * z * z - em[1], [z * einv, z * z - t(1)]
    else:
        eta = em[0] + o
        if family == "poisson":
            lf, dl = x * eta - np.exp(eta), [x - np.exp(eta)]
        else:
            lf, dl = x * eta - np.logaddexp(t(0), eta), [x - t(1) / (t(1) + np.exp(-eta))]
    return np.where(live, w * lf, t(0)), [np.where(live, w * g, t(0)) for g in dl]


def logp_score(family, K, y, p0, pr):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype"""
    t = y.dtype.type
    d, N = y.shape
    E, R = E_OF[family], p0.size // 4
    assert d == K + K * K + E * K and p0.size == 4 * R and pr.size == 2 * d + 2
    x, off, wt, seg = p0.astype(y.dtype).reshape(4, R)
    pm, pis, par = np.split(pr.astype(y.dtype), [d, 2 * d])
    start = seg != 0
    start[0] = True
    last = np.append(start[1:], True)  # the last row of a sequence
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        lpi = y[:K] - logsumexp(y[:K], axis=0)
        Lam = y[K:K + K * K].reshape(K, K, N)
        lP = Lam - logsumexp(Lam, axis=1, keepdims=True)
        ell, dl = emissions(family, y[K + K * K:].reshape(E, K, N), x, off, wt)
        la, lb = np.empty((R, K, N), y.dtype), np.zeros((R, K, N), y.dtype)
        for i in range(R):
            la[i] = (lpi if start[i] else logsumexp(la[i - 1][:, None, :] + lP, axis=0)) + ell[i]
        for i in range(R - 2, -1, -1):
            if not last[i]:
                lb[i] = logsumexp(lP + (ell[i + 1] + lb[i + 1])[None], axis=1)
        ll = logsumexp(la[last], axis=1)        # (sequences, N): each sequence's log L, from its last row
        llseq = ll[np.cumsum(start) - 1]        # (R, N): that of the sequence a row belongs to
        gam = np.exp(la + lb - llseq[:, None, :])
        xi = np.exp(la[:-1][:, :, None, :] + lP[None] + (ell[1:] + lb[1:])[:, None, :, :] - llseq[1:][:, None, None, :])  # (R-1, K, K, N)
        xi = np.where(start[1:][:, None, None, None], t(0), xi)
        gprev = np.where(start[1:][:, None, None], t(0), gam[:-1])
        g_lam = xi.sum(0) - np.exp(lP) * gprev.sum(0)[:, None, :]
        g_iota = gam[start].sum(0) - t(start.sum()) * np.exp(lpi)
        g_em = [(gam * g).sum(0) for g in dl]
    dv = (y - pm[:, None]) * pis[:, None]
    grad = np.concatenate([g_iota, g_lam.reshape(K * K, N)] + g_em) - dv * pis[:, None]
    return par[1] + ll.sum(0) - t(0.5) * (dv * dv).sum(0), grad.astype(y.dtype)


def ref_of(tgt):  # ref(y): float64 y -> the reference on the device's own (rounded) data; float32 y -> the float32 floor
    pr, p0 = gf.target_arrays(tgt)
    return lambda y: logp_score(tgt.family, tgt.K, y, p0, pr)


def fixture(nf, family, K, R, starts=(0,), dtype=None, device="cpu", seed=SEED, x_edit=None):
    """one seeded HiddenMarkovTarget: data from well-separated regimes, offsets 0.3 randn, weights in [0.5, 1.5] with ONE weight-0 row
    (row R // 2, where R > 1: a single row stays live), sequences starting at `starts`, prior locations 0.3 randn and scales in
    [0.5, 2] with the last coordinate flat, const 0.7.  `x_edit(x, wt, off)` may replace the data (in place)."""
    import torch
    rng = np.random.default_rng(seed + 7 * K + R + 131 * sorted(E_OF).index(family))
    st = rng.integers(0, K, R)
    x = {"normal": lambda: 2.0 * st + 0.5 * rng.standard_normal(R), "poisson": lambda: rng.poisson(1.0 + 3.0 * st).astype(np.float64),
         "bernoulli": lambda: (rng.uniform(size=R) < (st + 0.5) / K).astype(np.float64)}[family]()
    off, wt, seg = 0.3 * rng.standard_normal(R), rng.uniform(0.5, 1.5, R), np.zeros(R)
    if R > 1:
        wt[R // 2] = 0.0
    seg[list(starts)] = 1.0
    if x_edit:
        x_edit(x, wt, off)
    d = K + K * K + E_OF[family] * K
    scl = rng.uniform(0.5, 2.0, d)
    scl[-1] = np.inf
    dtype = dtype or torch.float64
    tens = lambda a: torch.tensor(a, dtype=dtype, device=device)  # noqa: E731
    return nf.HiddenMarkovTarget(family, tens(x), K, offset=tens(off), weights=tens(wt), sequence_start=tens(seg),
                                 prior_loc=(0.3 * rng.standard_normal(d)).tolist(), prior_scale=scl.tolist(), const=0.7)
