"""The row-minibatch rule of nf_target_minibatch in numpy (include/nfhip.h), over the oracle's Philox: the strata, the indices of a
(seed, stream), the gather of a target's two buffers along its segment table, and the cases the CPU and GPU tests share."""
import numpy as np

import nf_oracle as orc

# the main grid of the issue: R = 77 rows, batches of 1, 7, 33 and all 77 rows, d = 6
R_MAIN, M_MAIN, D_MAIN = 77, (1, 7, 33, 77), 6
KINDS = ("glm", "hglm", "dglm_normal", "dglm_negbin", "softmax", "bnn")
# the row-width cases: (d, R, m) -- 16-byte rows of the widest flow, and rows that are not aligned
WIDTH_CASES = ((256, 40, 9), (255, 5, 2))


def strata(R, m):
    """lo_j = floor(j R / m) for j = 0 .. m (m + 1 values, int64) and n_j = lo_{j+1} - lo_j"""
    lo = np.array([(j * R) // m for j in range(m + 1)], dtype=np.int64)  # python integers: exact
    return lo, np.diff(lo)


def indices(R, m, seed, stream):
    """idx_j = lo_j + ((r_j n_j) >> 32), r_j = word x of philox4x32_10((j_lo, j_hi, 0xFFFFFFFF, stream), (seed_lo, seed_hi))"""
    lo, n = strata(R, m)
    j = np.arange(m, dtype=np.uint64)
    r = orc.philox4x32_10((j & np.uint64(0xFFFFFFFF)).astype(np.uint32), (j >> np.uint64(32)).astype(np.uint32),
                          np.full(m, 0xFFFFFFFF, dtype=np.uint32), np.full(m, stream & 0xFFFFFFFF, dtype=np.uint32),
                          np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))[0]
    return (lo[:-1] + ((r.astype(np.uint64) * n.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)).astype(np.int64)


def gather(p0, p1, segments, wseg, R, m, idx):
    """(p0', p1') of a batch: host copies p0 [elems] and p1 [R, w] in the element type, the segment table [(per_row, length)],
    idx [m] (already inside 0 .. R-1).  The weight is multiplied by n_j in the element type: one rounding."""
    t = p0.dtype.type
    _, n = strata(R, m)
    out, at = [], 0
    for s, (per_row, length) in enumerate(segments):
        if per_row:
            v = p0[at:at + R][idx]
            out.append(v * n.astype(p0.dtype) if s == wseg else v)
            at += R
        else:
            out.append(p0[at:at + length])
            at += length
    assert at == p0.size, (at, p0.size)
    res = np.concatenate(out).astype(p0.dtype)
    assert res.dtype.type is t
    return res, p1[idx].copy()


def build(nf, kind, dtype, device, d=D_MAIN, rows=R_MAIN, seed=3):
    """one full target of the main grid: every per-row segment random (every fifth weight 0), so that a wrong row shows"""
    import torch

    rng = np.random.default_rng(seed + 17 * KINDS.index(kind) + d + 1000 * rows)
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device=device)
    wt = rng.uniform(0.25, 2.0, rows)
    wt[::5] = 0.0
    off = 0.3 * rng.standard_normal(rows)
    if kind == "glm":
        A = rng.standard_normal((rows, d)) / np.sqrt(d)
        return nf.GLMTarget("logit", t(A), offset=t(off), weights=t(wt), lin=t(0.1 * rng.standard_normal(d)), const=0.5, prior_sigma=2.0)
    if kind == "hglm":  # p = 4, G = 2
        A = rng.standard_normal((rows, 4)) / 2.0
        return nf.HierarchicalGLMTarget("poisson", t(A), torch.tensor([0, -1, 1, 0], device=device), 2, offset=t(off), weights=t(wt),
                                        lin=t(0.1 * rng.standard_normal(4)), const=0.25, fixed_sigma=1.5, hyper=["halfnormal", "lognormal"])
    if kind in ("dglm_normal", "dglm_negbin"):  # p = 3, G = 2
        A = rng.standard_normal((rows, 3)) / 2.0
        cnt = rng.integers(0, 6, rows)
        cnt[1] = 5  # a live row (weight != 0) holds the maximum: Mt = 4
        return nf.DispersionGLMTarget(kind[5:], t(A), counts=torch.tensor(cnt, device=device) if kind == "dglm_negbin" else None,
                                      groups=torch.tensor([0, -1, 1], device=device), n_groups=2, offset=t(off), weights=t(wt),
                                      lin=t(0.1 * rng.standard_normal(3)), const=0.125)
    if kind == "softmax":  # C = 2, p = 3: rows of three elements
        X = rng.standard_normal((rows, 3))
        return nf.SoftmaxRegressionTarget(t(X), torch.tensor(rng.integers(0, 2, rows), device=device), 2, weights=t(wt), prior_sigma=3.0)
    if kind == "bnn":  # H = 1, p = 4
        X = rng.standard_normal((rows, 4)) / 2.0
        return nf.BNNTarget("normal", t(X), 1, scale=t(rng.uniform(0.5, 1.5, rows)), offset=t(off), weights=t(wt))
    raise ValueError(kind)


def build_wide(nf, d, rows, dtype, device, seed=11):
    import torch

    rng = np.random.default_rng(seed + d + rows)
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device=device)
    return nf.GLMTarget("normal", t(rng.standard_normal((rows, d)) / np.sqrt(d)), offset=t(rng.standard_normal(rows)), weights=t(rng.uniform(0.5, 2.0, rows)))
