"""The hierarchical GLM form (NF_TARGET_HGLM_*) in numpy, shared by test_hier_cpu.py and test_gpu_hier.py:

    y        = [beta (p) ; tau (G)],   u = A y + off
    w_j(y)   = isd_j^2  if grp_j < 0,   exp(-2 tau_{grp_j})  otherwise
    h_g(x)   = -(x his_g)^2 / 2 | -exp(2 x) / 2 | -softplus(2 x)   (hk_g = 0 | 1 | 2),   x_g = tau_g - hm_g
    log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) + lin . y - sum_j beta_j^2 w_j / 2 + sum_g h_g(x_g)
    d beta_j = [A' (wt o phi')]_j + lin_j - beta_j w_j
    d tau_g  = [A' (wt o phi')]_{p+g} + lin_{p+g} + exp(-2 tau_g) sum_{j: grp_j = g} beta_j^2 + h_g'(x_g)

evaluated from a target's own `A` and `p0` = lin | off | wt | par | grp | isd | hm | his | hk | gptr | gidx (the members of a group
are taken from gptr / gidx, in list order, as the kernels take them).  The functions are dtype-generic and reuse glm_forms.phi:
float64 arrays give the reference, float32 arrays are evaluated op by op in float32 -- the floor tests/parity.py's `floor=` takes."""
import numpy as np

import glm_forms as gf

FAMILIES = gf.FAMILIES
HYPERS = ("lognormal", "halfnormal", "halfcauchy")


def split_p0(p0, d, rows, G):
    p = d - G
    assert p0.shape == (4 * d + 2 * rows + 3 + G,), (p0.shape, d, rows, G)
    sizes = [("lin", d), ("off", rows), ("wt", rows), ("par", 2), ("grp", p), ("isd", p), ("hm", G), ("his", G), ("hk", G),
             ("gptr", G + 1), ("gidx", p)]
    out, at = {}, 0
    for name, n in sizes:
        out[name] = p0[at:at + n]
        at += n
    assert at == p0.size
    return out


def hyper(kind, x, his):
    """h(x), h'(x) of one hyper-prior form element-wise, in x's dtype"""
    t = x.dtype.type
    if kind == 0:
        z = x * t(his)
        return t(-0.5) * z * z, -z * t(his)
    if kind == 1:
        e = np.exp(t(2) * x)
        return t(-0.5) * e, -e
    assert kind == 2, kind
    ph, dp = gf.phi("logit", t(-2) * x, 0.0)  # log sigmoid(-2 x) = -softplus(2 x); phi' = sigmoid(2 x)
    return ph, t(-2) * dp


def logp_score(family, y, A, p0, G):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; A and p0 are cast to it"""
    t = y.dtype.type
    rows, d = A.shape
    p = d - G
    A, q = A.astype(y.dtype), split_p0(p0.astype(y.dtype), d, rows, G)
    u = A @ y + q["off"][:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        ph, dp = gf.phi(family, u, q["par"][0])
        live = (q["wt"] != 0)[:, None]
        ph = np.where(live, q["wt"][:, None] * ph, t(0))
        dp = np.where(live, q["wt"][:, None] * dp, t(0))
        beta, tau = y[:p], y[p:]
        grp = q["grp"].astype(np.int64)
        om = np.where((grp >= 0)[:, None], np.exp(t(-2) * tau[np.maximum(grp, 0)]) if G else t(0), (q["isd"] * q["isd"])[:, None])
        prior = (t(-0.5) * (beta * beta) * om).sum(0)
        grad = A.T @ dp + q["lin"][:, None]
        grad[:p] -= beta * om
        gptr, gidx = q["gptr"].astype(np.int64), q["gidx"].astype(np.int64)
        for g in range(G):
            ss = np.zeros(y.shape[1], dtype=y.dtype)
            for k in range(gptr[g], gptr[g + 1]):
                ss = ss + beta[gidx[k]] * beta[gidx[k]]
            hv, hd = hyper(int(q["hk"][g]), tau[g] - q["hm"][g], q["his"][g])
            prior = prior + hv
            grad[p + g] += ss * np.exp(t(-2) * tau[g]) + hd
        lp = q["par"][1] + ph.sum(0) + q["lin"] @ y + prior
    return lp, grad


def target_arrays(tgt):
    """a HierarchicalGLMTarget's own A and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 reference on the device's own (rounded) data; float32 y -> the float32 floor"""
    A, p0 = target_arrays(tgt)
    return lambda y: logp_score(tgt.family, y, A, p0, tgt.G)


# ---- the GPU tests' inputs ----------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1), (5, 2), (35, 2), (64, 8)]  # (d, G)
ROWS = (1, 33, 133)
NS = (1, 37)


def arrays(family, d, G, rows, seed=5):
    """test_gpu_glm.glm_arrays' row data over the p = d - G coefficients (every fifth weight 0), grp random in {-1 .. G-1} with the
    last group left without a member (G >= 2), fixed sigmas in [0.5, 2] with one flat coefficient, and the three hyper-priors in turn"""
    p = d - G
    rng = np.random.default_rng(seed + 7 * d + rows + 131 * FAMILIES.index(family) + 1009 * G)
    A = rng.standard_normal((rows, p)) / np.sqrt(p)
    off = 0.5 * rng.standard_normal(rows)
    wt = rng.uniform(0.3, 2.5, rows)
    if rows > 1:
        wt[2::5] = 0.0
    lin = 0.5 * rng.standard_normal(p)
    hi = G - 1 if G >= 2 else G  # groups that may have members
    grp = rng.integers(-1, hi, p)
    if hi >= 1:
        grp[p - 1] = 0  # at least one member somewhere
    sig = rng.uniform(0.5, 2.0, p)
    if p > 1:
        grp[0], sig[0] = -1, np.inf  # a coefficient under a flat prior
    hyp = [HYPERS[(g + G) % 3] for g in range(G)]  # G = 1: half-normal; G = 2: half-Cauchy, log-normal; G = 8: every form
    loc = 0.3 * rng.standard_normal(G)
    scl = rng.uniform(0.7, 1.8, G)
    return dict(A=A, off=off, wt=wt, lin=lin, grp=grp, sig=sig, hyper=hyp, loc=loc, scl=scl)


def sample_ys(d, n, f64, seed=1):
    """standard normal draws (the log-scales stay within a few units: exp(-2 tau) does not leave float32's comfortable range)"""
    ys = np.random.default_rng(seed + d + n).standard_normal((d, n))
    return ys if f64 else ys.astype(np.float32).astype(np.float64)


def build(nf, family, d, G, rows, dtype, device, seed=5):
    """the HierarchicalGLMTarget of `arrays` in one element type on one device"""
    import torch

    a = arrays(family, d, G, rows, seed)
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device=device)
    return nf.HierarchicalGLMTarget(family, t(a["A"]), torch.tensor(a["grp"], device=device), G, t(a["off"]), t(a["wt"]), t(a["lin"]), const=0.7,
                                    param=3.0 if family == "student" else 0.0, fixed_sigma=a["sig"].tolist(), hyper=a["hyper"],
                                    hyper_loc=a["loc"].tolist(), hyper_scale=a["scl"].tolist())
