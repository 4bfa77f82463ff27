"""CPU checks of the hidden-Markov-model targets (NF_TARGET_HMM_*, kinds 48 .. 50): tests/hmm_forms.py against central differences,
host packing and the normaliser folds against scipy.stats on a case worked by brute force over the state paths, nf_target_check's
answers, argument errors, the constants' three copies."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import stats
from scipy.special import softmax

import glm_forms as gf
import hmm_forms as hf
from __graft_entry__ import ROOT, build, load_package

KINDS = {"normal": 48, "poisson": 49, "bernoulli": 50}


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("family", list(KINDS))
def test_the_numpy_form_agrees_with_central_differences(nf, family, K):
    tgt = hf.fixture(nf, family, K, 9, starts=(0, 4))
    ref, d = hf.ref_of(tgt), tgt.d
    y = 0.7 * np.random.default_rng(4).standard_normal((d, 3))
    lp, g = ref(y)
    assert np.isfinite(lp).all() and np.abs(g).max() > 0.1
    h = 1e-6
    for j in range(d):
        e = np.zeros((d, 1))
        e[j] = h
        assert np.allclose((ref(y + e)[0] - ref(y - e)[0]) / (2 * h), g[j], rtol=2e-6, atol=2e-6), j


@pytest.mark.parametrize("family", list(KINDS))
def test_packing_and_the_folds_against_brute_force_over_the_state_paths(nf, family):
    """two rows, two states: log p = const + log sum over the four paths of pi0 P emission^wt, with scipy.stats' normalised densities"""
    x = {"normal": [0.4, -1.1], "poisson": [2.0, 0.0], "bernoulli": [1.0, 0.0]}[family]
    off, wt, loc, scl = [0.2, -0.3], [1.5, 0.5], np.linspace(-0.5, 0.5, 10), [0.5, 2.0, math.inf, 1.0, 1.5, 0.7, 2.5, 1.0, 3.0, 0.9]
    d = 10 if family == "normal" else 8
    tgt = nf.HiddenMarkovTarget(family, torch.tensor(x, dtype=torch.float64), 2, offset=off, weights=wt, prior_loc=loc[:d].tolist(), prior_scale=scl[:d], const=0.3)
    pr, p0 = gf.target_arrays(tgt)
    assert np.array_equal(p0, np.concatenate([x, off, wt, [1.0, 0.0]])) and np.array_equal(pr[:d], loc[:d]) and pr[2 * d] == 0 and pr[d + 2] == 0
    assert tgt.c.kind == KINDS[family] and tgt.c.s0 == 2.0 and tgt.c.s1 == 2.0 and tgt.d == d and pr.shape == (2 * d + 2,)
    y = np.random.default_rng(6).standard_normal(d)
    pi0, P, em = softmax(y[:2]), softmax(y[2:6].reshape(2, 2), axis=1), y[6:].reshape(-1, 2)

    def logf(t, k):
        if family == "normal":
            return stats.norm.logpdf(x[t] - off[t], em[0, k], math.exp(em[1, k]))
        eta = em[0, k] + off[t]
        return stats.poisson.logpmf(x[t], math.exp(eta)) if family == "poisson" else stats.bernoulli.logpmf(x[t], 1 / (1 + math.exp(-eta)))

    like = sum(pi0[a] * math.exp(wt[0] * logf(0, a)) * P[a, b] * math.exp(wt[1] * logf(1, b)) for a in (0, 1) for b in (0, 1))
    fin = np.isfinite(scl[:d])
    want = 0.3 + math.log(like) + stats.norm.logpdf(y[fin], loc[:d][fin], np.asarray(scl[:d])[fin]).sum()
    assert np.allclose(hf.ref_of(tgt)(y[:, None])[0], want, rtol=1e-13, atol=1e-12)
    upi, uP, uem = tgt.unpack(torch.tensor(y))
    nat = {"normal": lambda: (em[0], np.exp(em[1])), "poisson": lambda: (np.exp(em[0]),), "bernoulli": lambda: (1 / (1 + np.exp(-em[0])),)}[family]()
    assert np.allclose(upi, pi0) and np.allclose(uP, P) and all(np.allclose(a, b) for a, b in zip(uem, nat))
    filt = np.array([sum(pi0[a] * math.exp(wt[0] * logf(0, a)) * P[a, b] for a in (0, 1)) * math.exp(wt[1] * logf(1, b)) for b in (0, 1)])
    assert np.allclose(tgt.predict(torch.tensor(y)), filt / filt.sum(), rtol=1e-12)


def test_argument_errors(nf):
    x = torch.tensor([0.0, 1.0, 1.0])
    for fam, xs, kw, match in (("normal", x, dict(n_states=1), "n_states"), ("normal", x, dict(n_states=9), "n_states"), ("gamma", x, dict(n_states=2), "family"),
                               ("normal", torch.zeros(nf._lib.NF_HMM_MAXR + 1), dict(n_states=2), "rows exceed"),
                               ("normal", x, dict(n_states=2, sequence_start=[0, 1, 0]), "row 0"), ("normal", x, dict(n_states=2, weights=[1.0, -1.0, 1.0]), "weights"),
                               ("bernoulli", torch.tensor([0.0, 1.5]), dict(n_states=2), r"\[0, 1\]"), ("poisson", torch.tensor([3.0, -1.0]), dict(n_states=2), ">= 0"),
                               ("normal", x, dict(n_states=2, prior_scale=[1.0] * 7), "prior_scale")):
        with pytest.raises(nf.NFHipError, match=match):
            nf.HiddenMarkovTarget(fam, xs, **kw)
    tgt = nf.HiddenMarkovTarget("bernoulli", torch.tensor([0.0, 7.0]), 2, weights=[1.0, 0.0])  # (a missing row's x may hold anything)
    with pytest.raises(nf.NFHipError, match="MinibatchTarget"):
        nf.MinibatchTarget(tgt, 1)
    with pytest.raises(nf.NFHipError, match="noncentred"):
        nf.noncentred(None, tgt)


def test_target_check_errors_come_before_device_work_and_the_constants_agree(nf):
    from normalizingflows_jl_amd._lib import Target
    lib, L = nf.load_library(), nf._lib
    buf, buf2 = (C.c_double * 64)(), (C.c_double * 64)()
    p, x = C.cast(buf, C.c_void_p).value, C.cast(buf2, C.c_void_p).value
    ctx = C.cast((C.c_char * 4096)(), C.c_void_p)
    logp = lambda t, d, n=0, dtype=0: lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)  # noqa: E731

    for dtype in (0, 1):
        for kind, E in ((48, 2), (49, 1), (50, 1)):
            dk = lambda K: K + K * K + E * K  # noqa: E731
            assert [logp(Target(kind, *pp, 8.0, 2.0), dk(2), dtype=dtype) for pp in ((0, x), (p, 0), (p, p))] == [-1] * 3  # a NULL buffer; p0 == p1
            for s0 in (0.0, -4.0, 1.5, 2147483648.0, math.nan, math.inf):
                assert logp(Target(kind, p, x, s0, 2.0), dk(2), dtype=dtype) == -1, s0        # R: a positive integer that fits an int
            for s1 in (0.0, 1.0, -2.0, 2.5, math.nan, math.inf, -math.inf):
                assert logp(Target(kind, p, x, 8.0, s1), dk(2), dtype=dtype) == -1, s1        # K: an integer >= 2
            assert logp(Target(kind, p, x, 8.0, 3.0), dk(3) + 1, dtype=dtype) == logp(Target(kind, p, x, 8.0, 9.0), dk(8), dtype=dtype) == -1  # d is checked exactly, first
            assert logp(Target(kind, p, x, 8.0, 9.0), dk(9), n=4, dtype=dtype) == logp(Target(kind, p, x, L.NF_HMM_MAXR + 1.0, 2.0), dk(2), n=4, dtype=dtype) == -2
            assert logp(Target(kind, p, x, 1.0, 2.0), dk(2), dtype=dtype) >= 0 and logp(Target(kind, p, x, float(L.NF_HMM_MAXR), 8.0), dk(8), dtype=dtype) >= 0
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    for i, (fam, kind) in enumerate(KINDS.items()):
        name = "NF_TARGET_HMM_" + fam.upper()
        assert re.search(rf"^#define {name} \(NF_TARGET_SCALEGLM \+ {i + 1}\)\s*$", hdr, re.M) and L.NF_TARGET_SCALEGLM + i + 1 == getattr(L, name) == kind
        assert int(re.search(rf"const {name} = Int32\((\d+)\)", jl).group(1)) == kind
    assert int(re.search(r"^#define NF_HMM_MAXR (\d+)\s*$", hdr, re.M).group(1)) == L.NF_HMM_MAXR == 4096
    assert int(re.search(r"^#define NF_HMM_SEGMENT (\d+)\s*$", hdr, re.M).group(1)) == L.NF_HMM_SEGMENT == 64
    assert lib.nf_abi_version() == 4 and len(nf.SYMBOLS) == 49
