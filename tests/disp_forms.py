"""The dispersion GLM form (NF_TARGET_DGLM_*) in numpy, shared by test_disp_cpu.py and test_gpu_disp.py:

    y        = [beta (p) ; tau (G) ; lambda],   u = A y + off
    w_j, h_g   hier_forms' (entry G of hm / his / hk is lambda's hyper-prior, with no member list)
    log p(y) = par[1] + sum_i wt_i phi_i(u_i, lambda) + lin . y - sum_j beta_j^2 w_j / 2 + sum_{g<G} h_g(tau_g - hm_g)
               + h_G(lambda - hm_G) + T(lambda)
    normal / student   z = u exp(-lambda):  phi = phi_fam(z) ;  d/du = exp(-lambda) phi'(z) ;  d/dlambda = -phi'(z) z ;  T = 0
    negbin             x = u - lambda, r = exp(lambda):  phi = -(k + r) softplus(x) ;  d/du = -(k + r) sigmoid(x) ;
                       d/dlambda = -r softplus(x) + (k + r) sigmoid(x) ;  T = sum_j ctab[j] log1p((j + 1) exp(-lambda))

evaluated from a target's own `A` and `p0` = lin | off | wt | par[4] | grp | isd | hm | his | hk | gptr | gidx | cnt | ctab.  The
functions are dtype-generic and reuse glm_forms.phi / hier_forms.hyper: float64 arrays give the reference, float32 arrays are
evaluated op by op in float32 -- the floor tests/parity.py's `floor=` takes."""
import numpy as np

import glm_forms as gf
import hier_forms as hf

FAMILIES = ("normal", "student", "negbin")
HYPERS = hf.HYPERS


def split_p0(p0, d, rows, G, negbin):
    p = d - G - 1
    fixed = [("lin", d), ("off", rows), ("wt", rows), ("par", 4), ("grp", p), ("isd", p), ("hm", G + 1), ("his", G + 1), ("hk", G + 1),
             ("gptr", G + 1), ("gidx", p)]
    out, at = {}, 0
    for name, n in fixed:
        out[name] = p0[at:at + n]
        at += n
    mt = int(out["par"][2])
    if negbin:
        out["cnt"], out["ctab"] = p0[at:at + rows], p0[at + rows:at + rows + mt]
        at += rows + mt
    else:
        assert mt == 0
    assert at == p0.size and out["par"][3] == 0, (p0.shape, d, rows, G, negbin, mt)
    return out


def row_terms(family, u, lam, cnt, par0):
    """phi, d phi / d u, d phi / d lambda of every row [rows, N] at the samples' lambda [N], in u's dtype"""
    t = u.dtype.type
    if family == "negbin":
        nsp, sg = gf.phi("logit", lam[None, :] - u, 0.0)  # log sigmoid(lambda - u) = -softplus(u - lambda) ; sigmoid(u - lambda)
        el = np.exp(lam)[None, :]
        kr = cnt[:, None] + el
        return kr * nsp, -kr * sg, el * nsp + kr * sg
    einv = np.exp(-lam)[None, :]
    z = u * einv
    ph, dz = gf.phi(family, z, par0)
    return ph, einv * dz, -dz * z


def table(ctab, lam):
    """T(lambda), T'(lambda) [N] in lam's dtype"""
    t = lam.dtype.type
    tv, td = np.zeros_like(lam), np.zeros_like(lam)
    einv, el = np.exp(-lam), np.exp(lam)
    for j in range(ctab.size):
        m = t(j + 1)
        tv = tv + ctab[j] * np.log1p(m * einv)
        td = td - ctab[j] * m / (el + m)
    return tv, td


def logp_score(family, y, A, p0, G):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; A and p0 are cast to it"""
    t = y.dtype.type
    rows, d = A.shape
    p = d - G - 1
    A, q = A.astype(y.dtype), split_p0(p0.astype(y.dtype), d, rows, G, family == "negbin")
    u = A @ y + q["off"][:, None]
    beta, tau, lam = y[:p], y[p:p + G], y[d - 1]
    with np.errstate(over="ignore", invalid="ignore"):
        ph, du, dl = row_terms(family, u, lam, q.get("cnt"), q["par"][0])
        live = (q["wt"] != 0)[:, None]
        w = q["wt"][:, None]
        ph, du, dl = np.where(live, w * ph, t(0)), np.where(live, w * du, t(0)), np.where(live, w * dl, t(0))
        grp = q["grp"].astype(np.int64)
        om = np.where((grp >= 0)[:, None], np.exp(t(-2) * tau[np.maximum(grp, 0)]) if G else t(0), (q["isd"] * q["isd"])[:, None])
        prior = (t(-0.5) * (beta * beta) * om).sum(0)
        grad = A.T @ du + q["lin"][:, None]
        grad[:p] -= beta * om
        gptr, gidx = q["gptr"].astype(np.int64), q["gidx"].astype(np.int64)
        for g in range(G):
            ss = np.zeros(y.shape[1], dtype=y.dtype)
            for k in range(gptr[g], gptr[g + 1]):
                ss = ss + beta[gidx[k]] * beta[gidx[k]]
            hv, hd = hf.hyper(int(q["hk"][g]), tau[g] - q["hm"][g], q["his"][g])
            prior = prior + hv
            grad[p + g] += ss * np.exp(t(-2) * tau[g]) + hd
        hv, hd = hf.hyper(int(q["hk"][G]), lam - q["hm"][G], q["his"][G])
        tv, td = table(q["ctab"], lam) if family == "negbin" else (np.zeros_like(lam), np.zeros_like(lam))
        prior = prior + hv + tv
        grad[d - 1] += dl.sum(0) + hd + td
        lp = q["par"][1] + ph.sum(0) + q["lin"] @ y + prior
    return lp, grad


def target_arrays(tgt):
    """a DispersionGLMTarget's own A and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 reference on the device's own (rounded) data; float32 y -> the float32 floor"""
    A, p0 = target_arrays(tgt)
    return lambda y: logp_score(tgt.family, y, A, p0, tgt.G)


# ---- the GPU tests' inputs ----------------------------------------------------------------------------------------------------------
SHAPES = [(2, 0), (5, 2), (33, 0), (35, 2), (64, 8)]  # (d, G); (33, 0) puts lambda alone in the second 32-feature block
ROWS = (1, 33, 133)
NS = (1, 37)
MAXK = (0, 1, 2, 18)  # table lengths 0, 0, 1 and 17 (more entries than the eight summing threads)


def arrays(family, d, G, rows, seed=5, maxk=18, disp=None):
    """hier_forms.arrays' data over the p = d - G - 1 coefficients (every fifth weight 0; p = 1 allowed), counts in 0..maxk with
    the maximum present on a live row (and a larger one on a zero-weight row, which must not enter the table), lambda's
    hyper-prior: the three forms in turn over ROWS (starting at d) unless `disp` names one"""
    p = d - G - 1
    rng = np.random.default_rng(seed + 7 * d + rows + 131 * FAMILIES.index(family) + 1009 * G)
    A = rng.standard_normal((rows, p)) / np.sqrt(p)
    off = 0.5 * rng.standard_normal(rows)
    wt = rng.uniform(0.3, 2.5, rows)
    if rows > 1:
        wt[2::5] = 0.0
    lin = 0.5 * rng.standard_normal(p)
    hi = G - 1 if G >= 2 else G  # groups that may have members
    grp = rng.integers(-1, hi, p) if hi >= 1 else np.full(p, -1)
    if hi >= 1:
        grp[p - 1] = 0  # at least one member somewhere
    sig = rng.uniform(0.5, 2.0, p)
    if p > 1:
        grp[0], sig[0] = -1, np.inf  # a coefficient under a flat prior
    hyp = [HYPERS[(g + G) % 3] for g in range(G)]
    loc = 0.3 * rng.standard_normal(G)
    scl = rng.uniform(0.7, 1.8, G)
    cnt = rng.integers(0, maxk + 1, rows)
    cnt[0] = maxk  # row 0 is live (weights are zeroed from row 2 on)
    if rows > 2:
        cnt[2] = maxk + 5  # a zero-weight row
    dh = disp if disp is not None else HYPERS[(d + (ROWS.index(rows) if rows in ROWS else 0)) % 3]
    return dict(A=A, off=off, wt=wt, lin=lin, grp=grp, sig=sig, hyper=hyp, loc=loc, scl=scl, cnt=cnt, disp_hyper=dh,
                disp_loc=float(0.2 * rng.standard_normal()), disp_scale=float(rng.uniform(0.7, 1.8)))


def sample_ys(d, n, f64, seed=1):
    """standard normal draws (the log-scales and lambda stay within a few units)"""
    ys = np.random.default_rng(seed + d + n).standard_normal((d, n))
    return ys if f64 else ys.astype(np.float32).astype(np.float64)


def from_arrays(nf, family, a, G, dtype, device):
    import torch

    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device=device)
    return nf.DispersionGLMTarget(family, t(a["A"]), counts=t(a["cnt"]) if family == "negbin" else None, groups=torch.tensor(a["grp"], device=device),
                                  n_groups=G, offset=t(a["off"]), weights=t(a["wt"]), lin=t(a["lin"]), const=0.7,
                                  param=3.0 if family == "student" else 0.0, fixed_sigma=a["sig"].tolist(), hyper=a["hyper"],
                                  hyper_loc=a["loc"].tolist(), hyper_scale=a["scl"].tolist(), disp_hyper=a["disp_hyper"], disp_loc=a["disp_loc"],
                                  disp_scale=a["disp_scale"])


def build(nf, family, d, G, rows, dtype, device, seed=5, maxk=18, disp=None):
    """the DispersionGLMTarget of `arrays` in one element type on one device"""
    return from_arrays(nf, family, arrays(family, d, G, rows, seed, maxk, disp), G, dtype, device)
