"""CPU checks of the scaled-block GLM target (NF_TARGET_SCALEGLM, kind 47): host packing and the normaliser fold, tests/scaled_forms.py
against central differences and the mixed-family form, nf_target_check's answers, argument errors, the constant's three copies."""
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
import scaled_forms as sf
from __graft_entry__ import ROOT, build, load_package

KIND = 47


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def test_packing_sorts_by_scale_then_family_pads_every_run_and_folds_the_normalisers(nf):
    p, S = 5, 4
    tgt = sf.fixture(nf, p, S)
    A, p0 = gf.target_arrays(tgt)
    lin, off, wt, fam, bpar, sidx, fom, hm, his, hk, par = sf.split_p0(p0, p + S, tgt.rows, S)
    runs = sorted((-1 if s is None else s, mf.FAMILIES.index(f), q, n, i) for i, (f, n, q, s) in enumerate(sf.layout(S)))
    assert [r[:2] for r in runs] == [(-1, 0), (-1, 1), (-1, 2), (0, 3), (0, 4), (1, 5), (2, 4)] and tgt.rows == 384 and A.shape == (384, 9)
    i0, b0, n_s = 0, 0, np.zeros(S)
    for s, code, q, n, i in runs:
        Ab, ob, wb = mf.block_arrays(mf.FAMILIES[code], p, n, sf.SEED + i)
        nb = -(-n // 32)
        assert np.array_equal(A[i0:i0 + n, :p], Ab) and np.array_equal(off[i0:i0 + n], ob) and np.array_equal(wt[i0:i0 + n], wb)
        assert not A[i0 + n:i0 + 32 * nb].any() and not wt[i0 + n:i0 + 32 * nb].any() and not A[:, p:].any()
        assert (fam[b0:b0 + nb] == code).all() and (bpar[b0:b0 + nb] == q).all() and (sidx[b0:b0 + nb] == s).all()
        assert tgt.families[b0:b0 + nb] == [mf.FAMILIES[code]] * nb and tgt.scales[b0:b0 + nb] == [s] * nb
        if s >= 0:
            n_s[s] += wb.sum()
        i0, b0 = i0 + 32 * nb, b0 + nb
    jac = np.array([0.0, 1.0, 1.0, 0.0])  # lognormal | halfnormal | halfcauchy | lognormal: the half families' + tau
    assert np.allclose(lin[p:], jac - n_s, rtol=1e-14) and n_s[3] == 0 and (hk == [0, 1, 2, 0]).all() and fom[p - 1] == 0 and not fom[p:].any()
    assert tgt.c.kind == KIND and tgt.c.s0 == 384.0 and tgt.c.s1 == S and tgt.d == p + S
    y = torch.arange(18.0).reshape(9, 2)
    assert torch.equal(tgt.unpack(y)[0], y[:5]) and torch.equal(tgt.unpack(y)[1], y[5:])


@pytest.mark.parametrize("p,S", [(3, 2), (31, 4)])
def test_the_numpy_form_agrees_with_central_differences(nf, p, S):
    ref = sf.ref_of(sf.fixture(nf, p, S))
    y, cz = np.random.default_rng(4).standard_normal((p + S, 3)), []
    lp, g = ref(y, cz)
    assert min(c.min() for c in cz) >= 1e-3 and np.isfinite(lp).all()
    h = 1e-6
    for j in range(p + S):
        e = np.zeros((p + S, 1))
        e[j] = h
        assert np.allclose((ref(y + e)[0] - ref(y - e)[0]) / (2 * h), g[j], rtol=2e-6, atol=2e-6), j


def test_without_scales_it_is_the_mixed_family_target_plus_the_hyper_prior(nf):
    p = 5
    blocks = lambda: [nf.GLMBlock(f, *(mf.tensor(a) for a in mf.block_arrays(f, p, n, 3 + i)), param=q, const=0.1 * i) for i, (f, n, q) in enumerate(mf.COUNTS)]  # noqa: E731
    lin = mf.tensor(np.linspace(-1, 1, p))
    sc = nf.ScaledGLMTarget(blocks(), [None] * len(mf.COUNTS), 1, lin=lin, const=0.7, fixed_sigma=2.0, hyper="lognormal", hyper_loc=0.3, hyper_scale=0.7)
    mx = nf.MixedGLMTarget(blocks(), lin=lin, const=0.7, prior_sigma=2.0)
    assert sc.families == mx.families and sc.scales == [-1] * 10
    y = np.random.default_rng(5).standard_normal((p + 1, 6))
    (ls, gs), (lm, gm) = sf.ref_of(sc)(y), mf.ref_of(mx)(y[:p])
    assert np.allclose(ls, lm + stats.norm.logpdf(y[p], 0.3, 0.7), rtol=1e-13, atol=1e-12)
    assert np.allclose(gs[:p], gm, rtol=1e-13, atol=1e-12) and np.allclose(gs[p], -(y[p] - 0.3) / 0.49, rtol=1e-13, atol=1e-12)


def test_additive_regression_builds_one_penalty_per_smooth(nf):
    rng = np.random.default_rng(6)
    rows, m = 20, 6
    X, B1, B2, t = (torch.tensor(rng.standard_normal(s)) for s in ((rows, 2), (rows, m), (rows, m), (rows,)))
    D2 = np.diff(np.eye(m), 2, axis=0)
    tgt = nf.AdditiveRegressionTarget("normal", X, [(B1, torch.tensor(D2.T @ D2)), (B2, torch.eye(m, dtype=torch.float64))], t=t, prior_sigma=5.0, hyper="halfcauchy")
    lin = gf.target_arrays(tgt)[1][2 + 2 * m:tgt.d]  # by hand: the half-Cauchy's + tau less the penalty's RANK, m - 2 and m
    assert tgt.d == 2 + 2 * m + 2 and tgt.scales == [-1, 0, 1] and tgt.families == ["normal"] * 3 and lin.tolist() == [1.0 - (m - 2), 1.0 - m]
    y = rng.standard_normal((tgt.d, 3))
    beta, tau = y[:2 + 2 * m], y[2 + 2 * m:]
    eta = np.hstack([X.numpy(), B1.numpy(), B2.numpy()]) @ beta
    b1, b2 = beta[2:2 + m], beta[2 + m:]
    want = stats.norm.logpdf(t.numpy()[:, None], eta, 1.0).sum(0) + stats.norm.logpdf(beta, 0, 5.0).sum(0) \
        - 0.5 * ((D2 @ b1) ** 2).sum(0) * np.exp(-2 * tau[0]) - (m - 2) * (tau[0] + 0.5 * math.log(2 * math.pi)) + stats.norm.logpdf(b2, 0, np.exp(tau[1])).sum(0) \
        + (stats.halfcauchy.logpdf(np.exp(tau)) + tau).sum(0)
    assert np.allclose(sf.ref_of(tgt)(y)[0], want, rtol=1e-12, atol=1e-11)
    assert torch.allclose(tgt.predict(torch.tensor(y), X, [B1, B2]), torch.tensor(eta), rtol=1e-13, atol=1e-13)


def test_argument_errors(nf):
    like = torch.zeros(1, dtype=torch.float64)
    blk = lambda f, q=0.0: nf.GLMBlock(f, torch.ones(3, 4, dtype=torch.float64), param=q)  # noqa: E731
    for comps, sof, S, match in (([blk("logit")], [0], 1, "scale families"), ([blk("poisson"), blk("normal")], [1, 0], 2, "scale families"),
                                 ([blk("normal")], [0], 17, "n_scales"), ([blk("normal")], [0], 0, "n_scales"), ([blk("normal")], [1], 1, "scale_of"),
                                 ([blk("normal")], [0, 0], 1, "scale_of"), ([blk("normal")], [0.0], 1, "scale_of"), ([], [], 1, "components"),
                                 ([nf.coefficient_prior("normal", 250, like)], [0], 7, "d = 257")):
        with pytest.raises(nf.NFHipError, match=match):
            nf.ScaledGLMTarget(comps, sof, S)
    tgt = nf.ScaledGLMTarget([blk("student", 3.0)], [0], 1)
    with pytest.raises(nf.NFHipError, match="MinibatchTarget"):
        nf.MinibatchTarget(tgt, 8)
    with pytest.raises(nf.NFHipError, match="noncentred"):
        nf.noncentred(None, tgt)


def test_target_check_errors_come_before_device_work_and_the_constants_agree(nf):
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
        for s1 in (0.0, -1.0, 1.5, 8.0, 9.0, math.inf, -math.inf, math.nan):
            assert logp(Target(KIND, p, x, 64.0, s1), dtype=dtype) == -1, s1       # S is an integer in 1 .. d - 1
        assert logp(Target(KIND, p, x, 33.0, 2.0), d=257, dtype=dtype) == logp(Target(KIND, p, x, 64.0, 17.0), d=17, dtype=dtype) == -1  # an argument error first
        assert logp(Target(KIND, p, x, 64.0, 2.0), d=257, dtype=dtype) == logp(Target(KIND, p, x, 64.0, 17.0), d=18, n=4, dtype=dtype) == -2  # d > 256; S > 16
        assert logp(Target(KIND, p, x, 32.0, 1.0), d=2, dtype=dtype) >= 0 and logp(Target(KIND, p, x, 64.0, 16.0), d=256, dtype=dtype) >= 0
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    assert re.search(r"^#define NF_TARGET_SCALEGLM \(NF_TARGET_CRE_DSTUDENT \+ 1\)\s*$", hdr, re.M) and nf._lib.NF_TARGET_CRE_DSTUDENT + 1 == nf._lib.NF_TARGET_SCALEGLM == KIND
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    assert int(re.search(r"const NF_TARGET_SCALEGLM = Int32\((\d+)\)", jl).group(1)) == KIND
    assert nf.load_library().nf_abi_version() == 4 and len(nf.SYMBOLS) == 49
