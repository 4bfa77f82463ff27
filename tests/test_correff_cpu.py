"""CPU tests of the correlated-random-effects wrappers (CorrelatedEffectsTarget, MixedEffectsRegressionTarget): the folded device
buffers reproduce the definition (tests/correff_forms.py) through a numpy float64 evaluation of the packed layout, limits raise, the
kind numbers agree across the header, the package and the Julia extension, and unpack round-trips."""
import os
import re

import numpy as np
import pytest
import torch

import correff_forms as cf
from __graft_entry__ import ROOT, load_package

nf = load_package()
KINDS = ("LOGIT", "PROBIT", "POISSON", "STUDENT", "NORMAL", "DNORMAL", "DSTUDENT")


def test_kind_numbers_agree():
    hdr, jl = open(os.path.join(ROOT, "include", "nfhip.h")).read(), open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    assert nf._lib.NF_TARGET_DR_WEIBULL == 39
    vals = re.search(r"NF_TARGET_CRE_DSTUDENT =\s*" + r",\s*".join([r"Int32\((\d+)\)"] * 7), jl).groups()
    for i, name in enumerate(KINDS):
        assert getattr(nf._lib, "NF_TARGET_CRE_" + name) == 40 + i == int(vals[i])
        assert f"#define NF_TARGET_CRE_{name} (NF_TARGET_DR_WEIBULL + {i + 1})" in hdr


@pytest.mark.parametrize("geo,family", [("a", "logit"), ("a", "dstudent"), ("b", "normal"), ("c", "poisson"), ("c", "dnormal"), ("d", "normal")])
def test_the_folded_buffers_reproduce_the_definition(geo, family):
    c = cf.case(geo, family, True)
    tgt = cf.build(nf, c, torch.float64, "cpu")
    assert tgt.d == c["d"] and tgt.c.s1 == len(c["terms"]) and tgt.c.s0 == c["A"].shape[0]
    ys = 0.7 * np.random.default_rng(3).standard_normal((tgt.d, 5))
    want = cf.ref_of(c)(ys)[0]
    np.testing.assert_allclose(cf.packed_logp(tgt, ys), want, rtol=1e-11, atol=1e-11)


def test_mixed_effects_regression_folds_the_response():
    """sleepstudy's shape: t ~ N(x . beta + z . b_level, sigma^2) is the dnormal target on offset -t with the normalisers folded"""
    rng = np.random.default_rng(8)
    rows, G = 30, 4
    X, lev, t = torch.tensor(rng.standard_normal((rows, 2))), torch.tensor(rng.integers(0, G, rows)), torch.tensor(rng.standard_normal(rows))
    tgt = nf.MixedEffectsRegressionTarget("dnormal", X, [(X, lev, G, 2.0)], t=t, fixed_sigma=2.0, hyper="halfnormal", disp_hyper="lognormal", disp_scale=0.5)
    A = np.zeros((rows, 2 + 2 * G))
    A[:, :2] = X.numpy()
    for i in range(rows):
        A[i, 2 + 2 * int(lev[i]):4 + 2 * int(lev[i])] = X[i].numpy()
    c = dict(family="dnormal", p=2, terms=[(2, G, 2.0, ["halfnormal"] * 2, [0.0, 0.0], [1.0, 1.0])], A=A, off=-t.numpy(), wt=np.ones(rows), lin=np.zeros(2 + 2 * G),
             const=-0.5 * rows * np.log(2 * np.pi), param=0.0, sig=np.full(2, 2.0), disp=("lognormal", 0.0, 0.5))
    ys = 0.7 * rng.standard_normal((tgt.d, 3))
    np.testing.assert_allclose(cf.packed_logp(tgt, ys), cf.ref_of(c)(ys)[0], rtol=1e-11, atol=1e-11)
    y = torch.tensor(ys)
    eta = tgt.predict(y, X, X, lev)
    np.testing.assert_allclose(eta.numpy(), A @ ys[:2 + 2 * G], rtol=1e-12, atol=1e-12)


def test_limits_raise():
    X = torch.zeros(6, 3, dtype=torch.float64)
    with pytest.raises(nf.NFHipError, match="k = 5"):
        nf.CorrelatedEffectsTarget("normal", torch.zeros(6, 10, dtype=torch.float64), [(5, 2, 1.0, "halfcauchy", 0.0, 1.0)])
    with pytest.raises(nf.NFHipError, match="d = 257"):
        nf.CorrelatedEffectsTarget("normal", torch.zeros(6, 247, dtype=torch.float64), [(4, 60, 1.0, "halfcauchy", 0.0, 1.0)])
    with pytest.raises(nf.NFHipError, match="levels must be in 0..1"):
        nf.MixedEffectsRegressionTarget("normal", X, [(X[:, :2], torch.tensor([0, 1, 2, 0, 1, 0]), 2, 1.0)])
    with pytest.raises(nf.NFHipError, match="terms"):
        nf.CorrelatedEffectsTarget("normal", X, [])


def test_unpack_round_trips():
    c = cf.case("c", "dnormal", True)
    tgt = cf.build(nf, c, torch.float64, "cpu")
    y = torch.tensor(np.random.default_rng(2).standard_normal((tgt.d, 4)))
    beta, bs, sds, corrs, sigma = tgt.unpack(y)
    back, at = [beta], 3
    for (k, G, ib, it, io), b, sd, R in zip(tgt.layout, bs, sds, corrs):
        assert b.shape == (G, k, 4) and R.shape == (4, k, k) and torch.allclose(torch.diagonal(R, dim1=-2, dim2=-1), torch.ones(4, k, dtype=torch.float64))
        om = torch.distributions.transforms.CorrCholeskyTransform().inv(torch.linalg.cholesky(R)).T if k > 1 else y[:0]
        back += [b.reshape(G * k, 4), torch.log(sd), om]
    assert torch.allclose(torch.cat(back + [torch.log(sigma)[None]]), y, rtol=1e-9, atol=1e-9)
    assert tgt.unpack(y[:, 0])[1][1].shape == (4, 3)
