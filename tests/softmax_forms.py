"""The softmax regression form (NF_TARGET_SOFTMAX) in numpy, shared by test_softmax_cpu.py and test_gpu_softmax.py:

    y = [w_0; ...; w_{C-1}],  u_{i,c} = x_i . w_c
    log p(y)   = par[1] + sum_i wt_i (u_{i,c_i} - logsumexp_c u_{i,c}) - par[0] |y|^2 / 2
    grad_{w_c} = sum_i wt_i (1[c_i = c] - softmax_c(u_i)) x_i - par[0] w_c

evaluated from a target's own `X` and `p0` = lab | wt | par.  The functions are dtype-generic: float64 arrays give the reference,
float32 arrays are evaluated op by op in float32 -- the floor that tests/parity.py's `floor=` takes.  Also the inputs and the
shapes of the tests (X ~ N(0, 1) / sqrt(p) rounded to float32 with a ones column, wt from {1, 1, 2, 0.5, 0},
sigma = 3, y ~ N(0, 1) float32-representable)."""
import numpy as np

SIGMA = 3.0
WEIGHTS = (1.0, 1.0, 2.0, 0.5, 0.0)
# (C, p, rows): the smallest shapes at which each part of the kernels can go wrong
SHAPES = [(2, 1, 1), (3, 5, 33), (3, 21, 133), (4, 16, 40), (2, 40, 64), (16, 16, 70), (2, 128, 35)]
N_FULL = 70  # two tiles and a ragged third


def n_of(shape):
    """the batch sizes of a shape: 1, 33 and 70 at the first three, 70 elsewhere"""
    return (1, 33, N_FULL) if shape in SHAPES[:3] else (N_FULL,)


def split_p0(p0, rows):
    assert p0.shape == (2 * rows + 2,), (p0.shape, rows)
    return p0[:rows], p0[rows:2 * rows], p0[2 * rows:]


def logp_score(y, X, p0, C):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype; X and p0 are cast to it"""
    t = y.dtype.type
    rows, p = X.shape
    d, N = y.shape
    assert d == C * p
    X, p0 = X.astype(y.dtype), p0.astype(y.dtype)
    lab, wt, par = split_p0(p0, rows)
    W = y.reshape(C, p, N)
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.einsum("if,cfn->icn", X, W)                         # [rows, C, N]
        m = u.max(1, keepdims=True)
        e = np.exp(u - m)
        s = e.sum(1, keepdims=True)
        onehot = (lab[:, None] == np.arange(C)[None, :]).astype(y.dtype)   # [rows, C]
        ul = u[np.arange(rows), lab.astype(np.int64), :]           # the label's logit [rows, N]
        ph = (ul - m[:, 0]) - np.log(s[:, 0])                      # [rows, N]
        dp = onehot[:, :, None] - e / s                            # [rows, C, N]
        live = wt != 0
        ph = np.where(live[:, None], wt[:, None] * ph, t(0))       # a zero-weight row contributes exactly 0, whatever its logits are
        dp = np.where(live[:, None, None], wt[:, None, None] * dp, t(0))
        Xl = np.where(live[:, None], X, t(0))                      # (0 * a non-finite x would be NaN in numpy; the row is dropped)
    lp = par[1] + ph.sum(0) - t(0.5) * par[0] * (y * y).sum(0)
    g = np.einsum("if,icn->cfn", Xl, dp).reshape(d, N) - par[0] * y
    return lp.astype(y.dtype), g.astype(y.dtype)


def target_arrays(tgt):
    """a SoftmaxRegressionTarget's own X and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 reference on the device's own (rounded) data; float32 y -> the float32 floor"""
    X, p0 = target_arrays(tgt)
    return lambda y: logp_score(y, X, p0, tgt.n_classes)


def arrays(C, p, rows, seed=5):
    """X (float32-representable, first column 1), labels, weights of one case, float64"""
    rng = np.random.default_rng(seed + 1000 * C + 7 * p + rows)
    X = (rng.standard_normal((rows, p)) / np.sqrt(p)).astype(np.float32).astype(np.float64)
    X[:, 0] = 1.0
    lab = rng.integers(0, C, rows).astype(np.float64)
    wt = rng.choice(np.array(WEIGHTS), rows)
    return X, lab, wt


def sample_ys(d, n, seed=1):
    """y ~ N(0, 1), float32-representable"""
    return np.random.default_rng(seed + d + n).standard_normal((d, n)).astype(np.float32).astype(np.float64)


def p0_of(lab, wt, d, sigma=SIGMA, const=0.0):
    """the buffer the constructor folds, in float64"""
    return np.concatenate([lab, wt, [1.0 / sigma**2, const - 0.5 * d * np.log(2.0 * np.pi * sigma**2)]])
