"""CPU checks of the mixed-family GLM target (NF_TARGET_MIXGLM, kind 35): host packing, the fold of a GLMTarget component, the helper
blocks' constants against scipy.stats, nf_target_check's answers before any device work, and the constant in header, mirror and Julia file."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import stats

import glm_forms as gf
import mixed_forms as mf
from mixed_forms import COUNTS, SEED, block_arrays, six_families
from __graft_entry__ import ROOT, build, load_package

KIND = 35


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def test_packing_sorts_by_family_pads_every_run_and_labels_every_block(nf):
    d = 5
    tgt = six_families(nf, d)
    runs = sorted(((mf.FAMILIES.index(f), q, n, i) for i, (f, n, q) in enumerate(COUNTS)))
    A, p0 = gf.target_arrays(tgt)
    lin, off, wt, fam, bpar, par = mf.split_p0(p0, d, tgt.rows)
    assert tgt.rows == sum(-(-n // 32) * 32 for _, _, n, _ in runs) == 320 and tgt.d == d and A.shape == (320, d)
    i0, b0 = 0, 0
    for code, q, n, i in runs:
        Ab, ob, wb = block_arrays(mf.FAMILIES[code], d, n, SEED + i)
        nb = -(-n // 32)
        assert np.array_equal(A[i0:i0 + n], Ab) and np.array_equal(off[i0:i0 + n], ob) and np.array_equal(wt[i0:i0 + n], wb)
        pad = slice(i0 + n, i0 + 32 * nb)
        assert not A[pad].any() and not off[pad].any() and not wt[pad].any()
        assert (fam[b0:b0 + nb] == code).all() and (bpar[b0:b0 + nb] == q).all()
        assert tgt.families[b0:b0 + nb] == [mf.FAMILIES[code]] * nb
        i0, b0 = i0 + 32 * nb, b0 + nb
    assert par[0] == 0.0 and par[1] == pytest.approx(0.7 + 0.1 * sum(range(7)) - 0.5 * d * math.log(2 * math.pi * 4.0), abs=1e-12)
    assert tgt.c.kind == KIND and tgt.c.s0 == 320.0 and tgt.c.s1 == tgt.prior_sigma == pytest.approx(2.0, abs=1e-15)
    with pytest.raises(nf.NFHipError):
        nf.MinibatchTarget(tgt, 8)


def test_a_glm_target_component_folds_its_rows_lin_const_and_prior(nf):
    d, rows = 4, 9
    rng = np.random.default_rng(3)
    X, k = rng.standard_normal((rows, d)) / 2, rng.poisson(2.0, rows)
    glm = nf.PoissonRegressionTarget(mf.tensor(X), mf.tensor(k), exposure=mf.tensor(rng.uniform(0.5, 2.0, rows)), prior_sigma=2.0)
    S = np.diff(np.eye(d), axis=0).T @ np.diff(np.eye(d), axis=0)  # the first-order random-walk penalty: rank d - 1
    tgt = nf.MixedGLMTarget([glm, nf.gaussian_penalty(mf.tensor(S), mf.tensor(X))], const=0.3, prior_sigma=3.0)
    assert tgt.families == ["poisson", "normal"] and tgt.rows == 64 and tgt.precision == pytest.approx(1 / 4 + 1 / 9, rel=1e-15)
    y = rng.standard_normal((d, 6))
    lp, sc = mf.ref_of(tgt)(y)
    lg, sg = gf.ref_of(glm)(y)
    want = lg + 0.3 - 0.5 * np.einsum("in,ij,jn->n", y, S, y) + stats.norm.logpdf(y, 0.0, 3.0).sum(0)
    assert np.allclose(lp, want, rtol=1e-13, atol=1e-12) and np.allclose(sc, sg - S @ y - y / 9.0, rtol=1e-12, atol=1e-12)
    for bad in (np.triu(np.ones((d, d))), -np.eye(d), np.diag([1.0, -0.5, 1.0, 1.0]), np.zeros((d, d))):
        with pytest.raises(nf.NFHipError):
            nf.gaussian_penalty(mf.tensor(bad), mf.tensor(X))


@pytest.mark.parametrize("family", ["normal", "student", "check"])
def test_coefficient_prior_is_the_scipy_log_density(nf, family):
    d, idx = 6, [4, 0, 3]
    loc, scale, y = np.array([0.3, -1.0, 0.0]), np.array([0.5, 2.0, 1.3]), np.random.default_rng(5).standard_normal((6, 4))
    dist = {"normal": stats.norm(loc, scale), "student": stats.t(2.5, loc, scale), "check": stats.laplace(loc, scale)}[family]
    tgt = nf.MixedGLMTarget([nf.coefficient_prior(family, d, torch.zeros(1, dtype=torch.float64), idx, loc, scale, param=2.5)])
    lp, _ = mf.ref_of(tgt)(y)
    assert np.allclose(lp, dist.logpdf(y[idx].T).sum(1), rtol=1e-13, atol=1e-13) and math.isinf(tgt.prior_sigma)


def test_quantile_regression_is_the_asymmetric_laplace_posterior(nf):
    rng = np.random.default_rng(6)
    X, t, tau, s, y = rng.standard_normal((11, 3)), rng.standard_normal(11), 0.3, 0.7, rng.standard_normal((3, 5))
    tgt = nf.QuantileRegressionTarget(mf.tensor(X), mf.tensor(t), tau, scale=s, prior_sigma=1.5)
    ald = stats.laplace_asymmetric.logpdf(t[:, None], math.sqrt(tau / (1 - tau)), loc=X @ y, scale=s / math.sqrt(tau * (1 - tau)))  # (scipy's kappa, scale)
    assert np.allclose(mf.ref_of(tgt)(y)[0], ald.sum(0) + stats.norm.logpdf(y, 0.0, 1.5).sum(0), rtol=1e-12, atol=1e-12) and tgt.rows == 32


def test_target_check_errors_come_before_device_work_34_is_no_kind_and_the_constants_agree(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf, buf2 = (C.c_double * 64)(), (C.c_double * 64)()
    p, x = C.cast(buf, C.c_void_p).value, C.cast(buf2, C.c_void_p).value
    ctx = C.cast((C.c_char * 4096)(), C.c_void_p)

    logp = lambda t, d=8, n=0, dtype=0: lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)  # noqa: E731

    for dtype in (0, 1):
        assert [logp(Target(KIND, *pp, 64.0, 2.0), dtype=dtype) for pp in ((0, x), (p, 0), (p, p))] == [-1] * 3  # a NULL buffer; p0 == p1
        for s0 in (0.0, -32.0, 33.0, 48.0, 32.5, 2147483648.0, math.nan, math.inf):
            assert logp(Target(KIND, p, x, s0, 2.0), dtype=dtype) == -1, s0        # not a positive multiple of 32 that fits an int
        for s1 in (0.0, -1.0, -math.inf, math.nan):
            assert logp(Target(KIND, p, x, 64.0, s1), dtype=dtype) == -1, s1       # the prior sigma is > 0
        assert logp(Target(KIND, p, x, 64.0, 2.0), d=0, dtype=dtype) == logp(Target(KIND, p, x, 33.0, 2.0), d=257, dtype=dtype) == -1  # an argument error first
        assert logp(Target(KIND, p, x, 64.0, 2.0), d=257, dtype=dtype) == logp(Target(KIND, p, x, 64.0, 2.0), d=257, n=4, dtype=dtype) == -2  # d > 256
        assert logp(Target(KIND, p, x, 32.0, math.inf), d=1, dtype=dtype) >= 0 and logp(Target(KIND, p, x, 64.0, 0.5), d=256, dtype=dtype) >= 0
    assert logp(Target(34, p, x, 64.0, 2.0)) == -1  # no such kind
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    assert re.search(r"^#define NF_TARGET_MIXGLM \(NF_TARGET_RISKSET \+ 1 \+ 1\)\s*$", hdr, re.M) and nf._lib.NF_TARGET_RISKSET + 2 == nf._lib.NF_TARGET_MIXGLM == KIND
    assert 34 not in [v for k, v in vars(nf._lib).items() if k.startswith("NF_TARGET_")]
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    assert int(re.search(r"const NF_TARGET_MIXGLM = Int32\((\d+)\)", jl).group(1)) == KIND
    assert nf.load_library().nf_abi_version() == 4 and len(nf.SYMBOLS) == 49
