"""CPU checks of the distributional regression targets (NF_TARGET_DR_*, kinds 36 .. 39): every wrapper's folded form against
scipy.stats summed over rows, the score of tests/distreg_forms.py against central differences, nf_target_check's answers before any
device work, and the constants in header, mirror and Julia file."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import stats

import distreg_forms as df
from __graft_entry__ import ROOT, build, load_package

KINDS = (36, 37, 38, 39)


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def wrapper_case(nf, family):
    """-> (target, row log-likelihood (beta, gamma) -> [rows]) of a small case: 11 rows, p = 3, q = 2, weights with a zero"""
    rng = np.random.default_rng(8)
    n, X, Z, w = 11, rng.standard_normal((11, 3)) / 2, rng.standard_normal((11, 2)) / 2, rng.uniform(0.5, 2.0, 11)
    w[4] = 0.0
    T, kw = df.tensor, {"weights": df.tensor(w), "prior_sigma": 2.0, "prior_sigma_aux": 3.0}
    if family in ("normal", "student"):
        t, nu = rng.standard_normal(n), None if family == "normal" else 4.5
        dist = (lambda m, s: stats.norm(m, s)) if nu is None else (lambda m, s: stats.t(nu, m, s))
        return nf.LocationScaleRegressionTarget(T(X), T(t), T(Z), nu=nu, **kw), w, lambda b, g: dist(X @ b, np.exp(Z @ g)).logpdf(t)
    if family == "zipoisson":
        k, ex = rng.poisson(1.2, n) * rng.integers(0, 2, n), rng.uniform(0.5, 2.0, n)

        def ll(b, g):
            pi, pois = 1.0 / (1.0 + np.exp(-Z @ g)), stats.poisson(ex * np.exp(X @ b))
            return np.log(pi * (k == 0) + (1.0 - pi) * pois.pmf(k))
        return nf.ZeroInflatedPoissonTarget(T(X), T(k), T(Z), exposure=T(ex), **kw), w, ll
    tm, ev = rng.uniform(0.2, 3.0, n), rng.integers(0, 2, n)

    def ll(b, g):
        dist = stats.weibull_min(np.exp(Z @ g), scale=np.exp(X @ b))
        return np.where(ev == 1, dist.logpdf(tm), dist.logsf(tm))
    return nf.WeibullRegressionTarget(T(X), T(tm), T(ev), T(Z), **kw), w, ll


@pytest.mark.parametrize("family", df.FAMILIES)
def test_the_folded_form_is_the_scipy_log_likelihood_and_its_score_the_derivative(nf, family):
    tgt, w, ll = wrapper_case(nf, family)
    assert tgt.family == family and (tgt.d, tgt.p, tgt.q, tgt.rows) == (5, 3, 2, 11) and tgt.c.kind == KINDS[df.FAMILIES.index(family)]
    assert tgt.c.s0 == 11.0 and tgt.c.s1 == 3.0 and tgt.A.shape == (11, 5) and tgt.p0.shape == (4 * 11 + 5 + 4,)
    ref, y = df.ref_of(tgt), 0.7 * np.random.default_rng(9).standard_normal((5, 6))
    lp, sc = ref(y)
    prior = stats.norm.logpdf(y[:3], 0.0, 2.0).sum(0) + stats.norm.logpdf(y[3:], 0.0, 3.0).sum(0)
    want = np.array([w @ ll(y[:3, j], y[3:, j]) for j in range(6)]) + prior
    assert np.allclose(lp, want, rtol=1e-12, atol=1e-12)
    h = 1e-6
    for i in range(5):
        e = np.zeros((5, 1))
        e[i] = h
        assert np.allclose(sc[i], (ref(y + e)[0] - ref(y - e)[0]) / (2 * h), rtol=1e-6, atol=1e-7), i
    b, g = tgt.unpack(df.tensor(y))
    assert torch.equal(b, df.tensor(y[:3])) and torch.equal(g, df.tensor(y[3:]))
    with pytest.raises(nf.NFHipError):
        nf.MinibatchTarget(tgt, 4)


def test_z_none_is_a_column_of_ones_and_predict_returns_the_natural_parameters(nf):
    rng = np.random.default_rng(2)
    X, t, y = rng.standard_normal((7, 2)), rng.standard_normal(7), df.tensor([0.3, -0.2, 0.5])
    tgt = nf.LocationScaleRegressionTarget(df.tensor(X), df.tensor(t))
    assert tgt.q == 1 and bool((tgt.A[:, 2] == 1).all())
    mean, sigma = tgt.predict(y, df.tensor(X))
    assert np.allclose(mean.numpy(), X @ [0.3, -0.2]) and np.allclose(sigma.numpy(), math.exp(0.5))
    assert np.allclose(df.ref_of(tgt)(y.numpy()[:, None])[0], stats.norm(X @ [0.3, -0.2], math.exp(0.5)).logpdf(t).sum() + stats.norm.logpdf(y.numpy()).sum())


def test_target_check_errors_come_before_device_work_and_the_constants_agree(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf, buf2 = (C.c_double * 64)(), (C.c_double * 64)()
    p, x = C.cast(buf, C.c_void_p).value, C.cast(buf2, C.c_void_p).value
    ctx = C.cast((C.c_char * 4096)(), C.c_void_p)

    logp = lambda t, d=8, n=0, dtype=0: lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)  # noqa: E731

    for kind in KINDS:
        for dtype in (0, 1):
            assert [logp(Target(kind, *pp, 5.0, 3.0), dtype=dtype) for pp in ((0, x), (p, 0), (p, p))] == [-1] * 3  # a NULL buffer; p0 == p1
            for s0 in (0.0, -3.0, 2.5, 2147483648.0, math.nan, math.inf):
                assert logp(Target(kind, p, x, s0, 3.0), dtype=dtype) == -1, s0         # not a positive integer that fits an int
            for s1 in (0.0, 8.0, -1.0, 2.5, math.nan, math.inf):
                assert logp(Target(kind, p, x, 5.0, s1), dtype=dtype) == -1, s1         # p is an integer in 1 .. d - 1
            assert logp(Target(kind, p, x, 5.0, 1.0), d=1, dtype=dtype) == logp(Target(kind, p, x, 5.0, 257.0), d=257, dtype=dtype) == -1  # an argument error first
            assert logp(Target(kind, p, x, 5.0, 3.0), d=257, dtype=dtype) == logp(Target(kind, p, x, 5.0, 256.0), d=257, n=4, dtype=dtype) == -2  # d > 256
            assert logp(Target(kind, p, x, 1.0, 1.0), d=2, dtype=dtype) >= 0 and logp(Target(kind, p, x, 5.0, 255.0), d=256, dtype=dtype) >= 0
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    names = [f"NF_TARGET_DR_{f.upper()}" for f in df.FAMILIES]
    for i, (name, kind) in enumerate(zip(names, KINDS)):
        assert re.search(rf"^#define {name} \(NF_TARGET_MIXGLM \+ {i + 1}\)\s*$", hdr, re.M) and getattr(nf._lib, name) == nf._lib.NF_TARGET_MIXGLM + i + 1 == kind
    assert re.search(r"const " + ", ".join(names) + r" =\s*Int32\(36\), Int32\(37\), Int32\(38\), Int32\(39\)", jl)
    assert nf.load_library().nf_abi_version() == 4 and len(nf.SYMBOLS) == 49
