"""The one-hidden-layer Bayesian neural-network form (NF_TARGET_BNN_*) in numpy, shared by test_bnn_cpu.py and test_gpu_bnn.py:

    y = [w_0; ...; w_{H-1}; v; c],  a_ik = tanh(x_i . w_k),  f_i = c + sum_k v_k a_ik,  u_i = scl_i f_i + off_i
    log p(y) = par[1] + sum_i wt_i phi(u_i; par[0]) - par[2]/2 sum_k |w_k|^2 - par[3]/2 (|v|^2 + c^2)
    g_i = wt_i phi'(u_i; par[0]) scl_i,   d c = sum_i g_i - par[3] c,   d v_k = sum_i g_i a_ik - par[3] v_k,
    d w_k = sum_i g_i v_k (1 - a_ik^2) x_i - par[2] w_k

evaluated from a target's own `X` and `p0` = scl | off | wt | par[4], with the row functions of tests/glm_forms.py.  The functions
are dtype-generic: float64 arrays give the reference, float32 arrays are evaluated op by op in float32 (numpy's tanh) -- the floor
that tests/parity.py's `floor=` takes.  Also the inputs and the shapes of the tests: X ~ N(0, 1) / sqrt(p) rounded to float32 with
a ones column, wt from {1, 1, 2, 0.5, 0}; logit / probit: scl in {-1, +1}, off = 0; normal / student (nu = 4): scl = 2,
off = -2 t, t ~ N(0, 1); poisson: scl = 0.25; prior sigmas 3 (hidden) and 2 (output); y ~ N(0, 1) float32-representable."""
import numpy as np

import glm_forms as gf

FAMILIES = gf.FAMILIES
SIGMA_HIDDEN, SIGMA_OUT, NU = 3.0, 2.0, 4.0
WEIGHTS = (1.0, 1.0, 2.0, 0.5, 0.0)
# (H, p, rows): the smallest shapes at which each part of the kernels can go wrong
SHAPES = [(1, 1, 1),       # d = 3
          (3, 5, 33),      # d = 19: odd p (a k-step pair crosses a unit boundary), a ragged second row block
          (2, 14, 133),    # d = 31: v, c share W's only block; the waves wrap to a second round of row blocks
          (4, 14, 40),     # d = 61: DB 2
          (2, 31, 64),     # d = 65: DB 4 starts; v and c straddle a 32-feature block boundary
          (16, 14, 70),    # d = 241: DB 8, the largest H
          (1, 128, 35)]    # d = 130: the largest p
N_FULL = 70  # two tiles and a ragged third


def dim(H, p):
    return H * (p + 1) + 1


def n_of(shape):
    """the batch sizes of a shape: 1, 33 and 70 at the first three, 70 elsewhere"""
    return (1, 33, N_FULL) if shape in SHAPES[:3] else (N_FULL,)


def split_p0(p0, rows):
    assert p0.shape == (3 * rows + 4,), (p0.shape, rows)
    return p0[:rows], p0[rows:2 * rows], p0[2 * rows:3 * rows], p0[3 * rows:]


def logp_score(y, X, p0, H, family):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; X and p0 are cast to it"""
    t = y.dtype.type
    rows, p = X.shape
    d, N = y.shape
    assert d == dim(H, p), (d, H, p)
    X, p0 = X.astype(y.dtype), p0.astype(y.dtype)
    scl, off, wt, par = split_p0(p0, rows)
    HP = H * p
    W, v, c = y[:HP].reshape(H, p, N), y[HP:HP + H], y[d - 1]
    live = wt != 0
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.tanh(np.einsum("if,kfn->ikn", X, W))                       # [rows, H, N]
        f = c[None, :] + np.einsum("ikn,kn->in", a, v)                    # [rows, N]
        u = scl[:, None] * f + off[:, None]
        ph, dp = gf.phi(family, u, par[0])
        ph = np.where(live[:, None], wt[:, None] * ph, t(0))              # a zero-weight row contributes exactly 0, whatever it holds
        g = np.where(live[:, None], wt[:, None] * dp * scl[:, None], t(0))
        ga = np.where(live[:, None, None], g[:, None, :] * a, t(0))       # [rows, H, N]
        D = np.where(live[:, None, None], g[:, None, :] * v[None, :, :] * (t(1) - a * a), t(0))
        Xl = np.where(live[:, None], X, t(0))                             # (0 * a non-finite x would be NaN in numpy; the row is dropped)
    lp = par[1] + ph.sum(0) - t(0.5) * par[2] * (y[:HP] * y[:HP]).sum(0) - t(0.5) * par[3] * (y[HP:] * y[HP:]).sum(0)
    gW = np.einsum("if,ikn->kfn", Xl, D).reshape(HP, N) - par[2] * y[:HP]
    gv = ga.sum(0) - par[3] * v
    gc = g.sum(0) - par[3] * c
    return lp.astype(y.dtype), np.concatenate([gW, gv, gc[None, :]]).astype(y.dtype)


def target_arrays(tgt):
    """a BNNTarget's own X and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 reference on the device's own (rounded) data; float32 y -> the float32 floor"""
    X, p0 = target_arrays(tgt)
    return lambda y: logp_score(y, X, p0, tgt.n_hidden, tgt.family)


def arrays(family, H, p, rows, seed=5):
    """X (float32-representable, first column 1), scl, off, wt, param of one case, float64"""
    rng = np.random.default_rng(seed + 1000 * H + 7 * p + rows + 100000 * FAMILIES.index(family))
    X = (rng.standard_normal((rows, p)) / np.sqrt(p)).astype(np.float32).astype(np.float64)
    X[:, 0] = 1.0
    wt = rng.choice(np.array(WEIGHTS), rows)
    tv = rng.standard_normal(rows).astype(np.float32).astype(np.float64)
    sign = rng.choice(np.array([-1.0, 1.0]), rows)
    if family in ("logit", "probit"):
        scl, off = sign, np.zeros(rows)
    elif family == "poisson":
        scl, off = np.full(rows, 0.25), np.zeros(rows)
    else:
        scl, off = np.full(rows, 2.0), -2.0 * tv
    return X, scl, off, wt, (NU if family == "student" else 0.0)


def sample_ys(d, n, seed=1, scale=1.0):
    """y ~ N(0, 1) (times `scale`), float32-representable"""
    return (scale * np.random.default_rng(seed + d + n).standard_normal((d, n))).astype(np.float32).astype(np.float64)


def p0_of(scl, off, wt, param, H, p, sigma_hidden=SIGMA_HIDDEN, sigma_out=SIGMA_OUT, const=0.0):
    """the buffer the constructor folds, in float64"""
    c, prec = const, []
    for s, n in ((sigma_hidden, H * p), (sigma_out, H + 1)):
        prec.append(0.0 if np.isinf(s) else 1.0 / s**2)
        c += 0.0 if np.isinf(s) else -0.5 * n * np.log(2.0 * np.pi * s**2)
    return np.concatenate([scl, off, wt, [param, c, prec[0], prec[1]]])
