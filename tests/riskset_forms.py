"""The risk-set regression form (NF_TARGET_RISKSET: Cox partial likelihood, conditional logit) in numpy, shared by
test_riskset_cpu.py and test_gpu_riskset.py, from a target's own `X` [R, p] and `p0` = off[R] | logw[R] | m[R] | segstart[R] | lin[p]
| par[2]:

    eta_i = x_i . y + off_i,   a_i = eta_i + logw_i,   log p(y) = par[1] + lin . y - sum_i m_i c_i - par[0]/2 |y|^2,
    c_i = log sum_{j in seg(i), j <= i} w_j exp(eta_j)

`definition` is the reference, float64, written from the DEFINITION: for every row with an event mass the explicit risk set (the
live rows of its segment up to it), one log-sum-exp over it, and the gradient as the mass times the softmax-weighted mean of the
risk set's rows -- O(R^2), no recurrence.  `logp_score` is the RESTATEMENT the kernels evaluate, dtype-generic:
c_i = logaddexp(c_{i-1}, a_i) forward, V_j = m_j + V_{j+1} exp(c_j - c_{j+1}) backward, r_j = -exp(a_j - c_j) V_j; float64 arrays
give a second reference, float32 arrays are evaluated op by op in float32 -- the floor that tests/parity.py's `floor=` takes.
`pack` is the host packing written directly.  Also the inputs and the cases of the tests: X ~ N(0, 1) / sqrt(p) rounded to float32,
off ~ 0.3 N(0, 1), risk weights from {1, 1, 2, 0.5, 1, 1, 0} (about 15 % zeros), masses from {0, 0, 1, 2, 0.5}; y ~ s N(0, 1) with
s = 0.5 (predictors of order 1) or 12 (|eta| up to about 60), float32-representable."""
import functools

import numpy as np

SIGMA = 2.0
WEIGHTS = (1.0, 1.0, 2.0, 0.5, 1.0, 1.0, 0.0)
MASSES = (0.0, 0.0, 1.0, 2.0, 0.5)
REGIMES = {"unit": 0.5, "spread": 12.0}
D_SIZES = (1, 7, 33, 64, 130, 256)  # every DB, odd widths, two chunks of the image, the cap
N_SIZES = (1, 31, 33, 70)           # one sample, partial tiles, three tiles


def split_p0(p0, R, p):
    assert R % 32 == 0 and p0.shape == (4 * R + p + 2,), (p0.shape, R, p)
    return p0[:R], p0[R:2 * R], p0[2 * R:3 * R], p0[3 * R:4 * R], p0[4 * R:4 * R + p], p0[4 * R + p:]


def segments(seg):
    """segstart [R] -> the segment index of every row (row 0 always starts one)"""
    s = np.asarray(seg) != 0
    s[0] = True
    return np.cumsum(s) - 1


def definition(y, X, p0):
    """float64 y (d, N) -> (log p (N,), grad (d, N)) from explicit risk sets"""
    assert y.dtype == np.float64
    R, p = X.shape
    off, lw, m, seg, lin, par = split_p0(p0.astype(np.float64), R, p)
    X = X.astype(np.float64)
    sid = segments(seg)
    live = lw > -np.inf
    lp = par[1] + lin @ y - 0.5 * par[0] * (y * y).sum(0)
    alive = np.nonzero(live)[0]
    a_all = np.full((R, y.shape[1]), -np.inf)
    a_all[alive] = X[alive] @ y + (off[alive] + lw[alive])[:, None]
    W = np.zeros((R, y.shape[1]))                           # row j: sum over the event rows i with j in R(i) of m_i softmax_{R(i)}(j)
    for i in np.nonzero(m > 0)[0]:
        risk = np.nonzero(live & (sid == sid[i]) & (np.arange(R) <= i))[0]
        assert risk.size, "an event mass on an empty risk set"
        a = a_all[risk]                                     # [|risk|, N]
        top = a.max(0)
        e = np.exp(a - top)
        lp = lp - m[i] * (top + np.log(e.sum(0)))
        W[risk] += m[i] * (e / e.sum(0))
    return lp, lin[:, None] - par[0] * y - X[alive].T @ W[alive]


def logp_score(y, X, p0):
    """y (d, N) -> (log p (N,), grad (d, N)) in y's dtype by the two recurrences; X and p0 are cast to it"""
    t = y.dtype.type
    R, p = X.shape
    X, p0 = X.astype(y.dtype), p0.astype(y.dtype)
    off, lw, m, seg, lin, par = split_p0(p0, R, p)
    start = np.asarray(seg) != 0
    start[0] = True
    live = lw > -np.inf
    ninf = t(-np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        Xl = np.where(live[:, None], X, t(0))   # (0 * a non-finite x would be NaN in numpy; the row is dropped)
        a = np.where(live[:, None], Xl @ y + off[:, None] + lw[:, None], ninf)
        c = np.empty_like(a)
        for i in range(R):
            c[i] = a[i] if start[i] else np.logaddexp(c[i - 1], a[i])
        r = np.zeros_like(a)
        V = np.zeros(y.shape[1], dtype=y.dtype)
        for i in range(R - 1, -1, -1):
            if i == R - 1 or start[i + 1]:
                V = np.full(y.shape[1], m[i], dtype=y.dtype)
            else:
                V = m[i] + V * np.where(c[i] == ninf, t(0), np.exp(c[i] - c[i + 1]))
            if live[i]:
                r[i] = -np.exp(a[i] - c[i]) * V
        mc = np.where((m > 0)[:, None], m[:, None] * c, t(0)).sum(0)
    lp = par[1] + lin @ y - mc - t(0.5) * par[0] * (y * y).sum(0)
    return lp.astype(y.dtype), (Xl.T @ r + lin[:, None] - par[0] * y).astype(y.dtype)


def pack(X, seg, m, w, off, lin, const=0.0, sigma=SIGMA):
    """the host packing written directly, float64: the tail padded to a whole 32-row block with rows of weight 0 -> (X [R, p], p0)"""
    rows, p = X.shape
    pad = -rows % 32
    s = np.asarray(seg, dtype=np.float64).copy()
    s[0] = 1.0
    with np.errstate(divide="ignore"):
        lw = np.log(np.asarray(w, dtype=np.float64))
    flat = np.isinf(sigma)
    c = const + (0.0 if flat else -0.5 * p * np.log(2.0 * np.pi * sigma**2))
    z = np.zeros(pad)
    return (np.vstack([X, np.zeros((pad, p))]),
            np.concatenate([off, z, lw, np.full(pad, -np.inf), m, z, s, z, lin, [0.0 if flat else 1.0 / sigma**2, c]]))


def target_arrays(tgt):
    """a RiskSetTarget's own X and p0 as float64 numpy arrays (exact for either element type)"""
    return tgt.A.detach().double().cpu().numpy(), tgt.p0.detach().double().cpu().numpy()


def ref_of(tgt):
    """ref(y): float64 y -> the float64 DEFINITION on the device's own (rounded) data; float32 y -> the float32 floor (the recurrences)"""
    X, p0 = target_arrays(tgt)
    return lambda y: definition(y, X, p0) if y.dtype == np.float64 else logp_score(y, X, p0)


# ---- the segment geometries: name -> (rows, segment starts, rows of weight 0 forced, rows of mass forced) ------------------------------
# The tiled kernel takes the 32-row blocks four at a time, wave w the block 4 k + w: a block is a wave's range, 128 rows a round.
def _strata(rows, seed=11):
    rng = np.random.default_rng(seed)
    starts, i = [], 0
    while i < rows:
        starts.append(i)
        i += int(rng.integers(2, 6))
    return starts


GEOMETRIES = {
    "one_segment": (288, [0], [], []),                               # R = 288: the carry crosses all four waves and three rounds
    "boundary_inside_a_block": (96, [0, 45], [], []),                # R = 96: fewer blocks than waves
    "boundary_at_a_block_edge": (96, [0, 32, 64], [], []),           # (a block is a wave's range: the edge of a wave's range)
    "boundary_at_a_round_edge": (160, [0, 128], [], []),             # R = 160: an uneven split, the carry over the barrier is cut
    "one_row_segment": (70, [0, 40, 41], [], [40]),                  # its row carries a mass: c = a, V = m
    "strata_2_to_5": (150, _strata(150), [], []),                    # conditional logit
    "dead_block_mid_segment": (160, [0], list(range(64, 96)), []),   # a whole block of weight-0 rows inside a segment
    "dead_rows_at_segment_start": (90, [0, 50], [0, 1, 2] + list(range(50, 56)), []),
    "mass_on_last_live_row": (20, [0, 9], [], [19]),                 # R = 32: one block, three waves idle; 12 padding rows behind it
}


def padded(rows):
    return (rows + 31) // 32 * 32


assert {padded(g[0]) for g in GEOMETRIES.values()} == {32, 96, 160, 288}


@functools.lru_cache(maxsize=None)
def arrays(geometry, p, seed=5):
    """(X, seg, m, w, off, lin) of one case, float64, X / off / lin float32-representable; masses only where the risk set is not empty"""
    rows, starts, dead, massed = GEOMETRIES[geometry]
    rng = np.random.default_rng(seed + 7 * p + rows)
    X = (rng.standard_normal((rows, p)) / np.sqrt(p)).astype(np.float32).astype(np.float64)
    off = (0.3 * rng.standard_normal(rows)).astype(np.float32).astype(np.float64)
    w = rng.choice(np.array(WEIGHTS), rows)
    m = rng.choice(np.array(MASSES), rows)
    seg = np.zeros(rows)
    seg[starts] = 1.0
    w[dead] = 0.0
    sid = segments(seg)
    for i in massed:
        w[i], m[i] = 1.0, 2.0
    seen = np.zeros(sid[-1] + 1, dtype=bool)
    for i in range(rows):  # no mass before the segment's first live row
        seen[sid[i]] |= w[i] > 0
        if not seen[sid[i]]:
            m[i] = 0.0
    lin = (m @ X).astype(np.float32).astype(np.float64)
    return X, seg, m, w, off, lin


def sample_ys(p, n, regime, seed=1):
    """y ~ REGIMES[regime] N(0, 1), float32-representable, (p, n)"""
    y = REGIMES[regime] * np.random.default_rng(seed + p + n).standard_normal((p, n))
    return y.astype(np.float32).astype(np.float64)


# (geometry, d) pairs of the GPU tests: every geometry at an odd narrow width and at the two-chunk width, every width at the two
# geometries that load all waves
CASES = [(g, d) for g in GEOMETRIES for d in (7, 130)] + [(g, d) for g in ("one_segment", "strata_2_to_5") for d in (1, 33, 64, 256)]
