"""CPU checks of the GLM targets with a learned dispersion (NF_TARGET_DGLM_NORMAL / STUDENT / NEGBIN, kinds 29..31): the constants,
nf_target_check's argument conventions as nf_target_logp reports them BEFORE any device work (a stand-in context is enough), the
refusals of the flows that evaluate their target in their own kernels, the host folding of DispersionGLMTarget and the four
constructors over it against the models written DIRECTLY in float64 (scipy.special.gammaln for the negative binomial, the textbook
Normal / Student-t log-densities with sigma = exp(lambda), scipy.stats for the priors), the score of tests/disp_forms.py against
central differences, the constructors' refusals, the routing of the Python mirror and the new kernels' resources."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import special as sp
from scipy import stats

import disp_forms as df
from __graft_entry__ import ROOT, build, load_package

DGLM_KINDS = {"normal": 29, "student": 30, "negbin": 31}


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def test_constants_match_the_header_and_the_abi_version_stays(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M)}
    for fam, v in DGLM_KINDS.items():
        name = "NF_TARGET_DGLM_" + fam.upper()
        assert defs[name] == getattr(nf._lib, name) == v
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    mirror = [v for k, v in vars(nf._lib).items() if k.startswith("NF_TARGET_")]
    for absent in (7, 14, 21, 27, 28):
        assert absent not in defs.values() and absent not in mirror
    assert max(defs.values()) == 31
    from normalizingflows_jl_amd import flows

    assert flows._DGLM_KINDS == DGLM_KINDS and flows._DGLM_MAX_COUNT == 4097
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    m = re.search(r"const NF_TARGET_DGLM_NORMAL, NF_TARGET_DGLM_STUDENT, NF_TARGET_DGLM_NEGBIN =\s*Int32\((\d+)\), Int32\((\d+)\), Int32\((\d+)\)", jl)
    assert m and [int(x) for x in m.groups()] == [29, 30, 31]
    lib = nf.load_library()
    assert lib.nf_abi_version() == 4
    assert not any("dglm" in s.lower() or "disp" in s.lower() for s in nf.SYMBOLS)  # new kinds, no new symbol


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) and NF_ERR_UNSUPPORTED (-2) for every violated convention of kinds 29..31 without touching the context
    (N = 0: nothing is launched, and a good target's answer is no error)"""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=6, n=4, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)

    for kind in DGLM_KINDS.values():
        for dtype in (0, 1):
            assert logp(Target(kind, 0, p, 8.0, 2.0), dtype=dtype) == -1             # p0 = NULL
            assert logp(Target(kind, p, 0, 8.0, 2.0), dtype=dtype) == -1             # p1 = NULL
            assert logp(Target(kind, p, p, 0.0, 2.0), dtype=dtype) == -1             # rows = 0
            assert logp(Target(kind, p, p, -3.0, 2.0), dtype=dtype) == -1            # negative rows
            assert logp(Target(kind, p, p, 2.5, 2.0), dtype=dtype) == -1             # rows not integral
            assert logp(Target(kind, p, p, 2147483648.0, 2.0), dtype=dtype) == -1    # rows = 2^31
            assert logp(Target(kind, p, p, math.nan, 2.0), dtype=dtype) == -1        # NaN rows
            assert logp(Target(kind, p, p, 8.0, -1.0), dtype=dtype) == -1            # negative G
            assert logp(Target(kind, p, p, 8.0, 1.5), dtype=dtype) == -1             # G not integral
            assert logp(Target(kind, p, p, 8.0, math.nan), dtype=dtype) == -1        # NaN G
            assert logp(Target(kind, p, p, 8.0, 5.0), dtype=dtype) == -1             # G = d - 1: no coefficient left
            assert logp(Target(kind, p, p, 8.0, 6.0), dtype=dtype) == -1             # G = d
            assert logp(Target(kind, p, p, 8.0, math.inf), dtype=dtype) == -1
            assert logp(Target(kind, p, p, 8.0, 0.0), d=1, dtype=dtype) == -1        # d = 1 leaves room for no coefficient
            assert logp(Target(kind, p, p, 8.0, 300.0), d=257, dtype=dtype) == -1    # an argument error first
            assert logp(Target(kind, p, p, 8.0, 2.0), d=257, dtype=dtype) == -2      # d > 256
            assert logp(Target(kind, p, p, 8.0, 0.0), d=257, n=0, dtype=dtype) == -2
            assert logp(Target(kind, p, p, 8.0, 0.0), n=0, dtype=dtype) >= 0         # G = 0: past the check
            assert logp(Target(kind, p, p, 8.0, 4.0), n=0, dtype=dtype) >= 0         # G = d - 2
            assert logp(Target(kind, p, p, 8.0, 0.0), d=2, n=0, dtype=dtype) >= 0    # the smallest: one coefficient and lambda
            assert logp(Target(kind, p, p, 8.0, 8.0), d=256, n=0, dtype=dtype) >= 0  # d at its cap
            assert logp(Target(kind, p, p, 2147483647.0, 2.0), n=0, dtype=dtype) >= 0
    for absent in (7, 14, 21, 27, 28, 32):
        assert logp(Target(absent, p, p, 8.0, 2.0)) == -1  # no such kinds


def _five(lib, ctx, p, val, desc, tgt):
    return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
            lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
            lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
            lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
            lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with a
    dispersion kind as the target and as the Hamiltonian score -- the stand-in context is never used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    for tk in DGLM_KINDS.values():
        dg = Target(tk, p.value, p.value, 4.0, 1.0)
        for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1), ("planar", 1)):
            desc = FlowDesc()
            desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
            assert _five(lib, ctx, p, val, desc, dg) == [-2] * 5, (kind, tk)
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
        hd.score = C.cast(C.pointer(diag), C.c_void_p)  # a supported score, a dispersion ELBO target
        assert _five(lib, ctx, p, val, hd, dg) == [-2] * 5, tk
        hd.score = C.cast(C.pointer(dg), C.c_void_p)    # a dispersion score
        assert _five(lib, ctx, p, val, hd, diag) == [-2] * 5, tk


def test_realnvp_and_fullrank_get_past_every_refusal(nf):
    """RealNVP and full-rank descriptors of either element type with a dispersion kind: the ELBO entry points get past every refusal
    that comes before device work and stop at the stand-in context's device ordinal (a positive HIP error code); the graph form is
    never an argument error (its NF_ERR_UNSUPPORTED comes after the device ordinal for RealNVP: test_gpu_disp.py)"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    keep = (C.c_char * 4096)()
    C.cast(keep, C.POINTER(C.c_int32))[0] = 1 << 20  # no such device
    ctx = C.cast(keep, C.c_void_p)
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    for kind in ("realnvp", "fullrank"):
        for dtype in (0, 1):
            desc = FlowDesc()
            desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 5, 2 if kind == "realnvp" else 1
            if kind == "realnvp":
                desc.n_hidden = 2
                desc.hdims[0] = desc.hdims[1] = 32
            for tk in DGLM_KINDS.values():
                got = _five(lib, ctx, p, val, desc, Target(tk, p.value, p.value, 4.0, 2.0))
                assert all(c > 0 for c in got[:4]) and (got[4] > 0 or got[4] == -2), (kind, dtype, tk, got)


# ---- host folding against direct float64 evaluations -------------------------------------------------------------------------------
P_, ROWS, N_ = 4, 9, 5
NU = 3.5


def _data(seed=0):
    g = np.random.default_rng(seed)
    X = g.standard_normal((ROWS, P_)) / np.sqrt(P_)
    w = g.uniform(0.3, 2.5, ROWS)
    w[2] = 0.0  # one dropped row
    off = 0.4 * g.standard_normal(ROWS)
    return g, X, w, off


def _hyper_logpdf(name, x, loc, scl):
    """log-density over x = log s of s under the named prior (the half-families carry the Jacobian d s / d x = s)"""
    if name == "lognormal":
        return stats.norm.logpdf(x, loc, scl)
    s = np.exp(x)
    return (stats.halfnorm if name == "halfnormal" else stats.halfcauchy).logpdf(s, scale=scl) + x


def _prior(beta, tau, lam, grp, sig, hyper, loc, scl, dh, dloc, dscl):
    out = _hyper_logpdf(dh, lam, dloc, dscl)
    for j in range(beta.shape[0]):
        if grp[j] >= 0:
            out = out + stats.norm.logpdf(beta[j], 0.0, np.exp(tau[grp[j]]))
        elif np.isfinite(sig[j]):
            out = out + stats.norm.logpdf(beta[j], 0.0, sig[j])
    for g in range(len(hyper)):
        out = out + _hyper_logpdf(hyper[g], tau[g], loc[g], scl[g])
    return out


def _loglik(family, eta, lam, w, k=None):
    """sum_i w_i log p(row i): the textbook densities with sigma = exp(lambda); gammaln for the negative binomial"""
    if family == "normal":
        ll = stats.norm.logpdf(eta, 0.0, np.exp(lam)[None, :]) + 0.5 * np.log(2.0 * np.pi)  # (the -log(2 pi)/2 is the caller's const)
    elif family == "student":
        ll = stats.t.logpdf(eta, NU, scale=np.exp(lam)[None, :]) - (sp.gammaln(0.5 * (NU + 1)) - sp.gammaln(0.5 * NU) - 0.5 * np.log(NU * np.pi))
    else:
        r = np.exp(lam)[None, :]
        kk = k[:, None]
        ll = sp.gammaln(kk + r) - sp.gammaln(r) - sp.gammaln(kk + 1.0) + r * np.log(r) + kk * eta - (kk + r) * np.log(r + np.exp(eta))
    return (w[:, None] * ll).sum(0)


def _check_score(tgt, y0):
    ref = df.ref_of(tgt)
    sc = ref(y0)[1][:, 0]
    for i in range(tgt.d):
        e = np.zeros_like(y0)
        e[i] = 1e-6
        fd = (ref(y0 + e)[0][0] - ref(y0 - e)[0][0]) / 2e-6
        assert abs(fd - sc[i]) <= 1e-7 * max(1.0, abs(sc[i])), (i, fd, sc[i])


def _close(got, direct, rtol=1e-12):
    assert got.shape == direct.shape
    assert (np.abs(got - direct) <= rtol * np.maximum(1.0, np.abs(direct))).all(), (got, direct)


@pytest.mark.parametrize("disp_hyper", df.HYPERS)
@pytest.mark.parametrize("family", df.FAMILIES)
def test_folding_against_a_direct_evaluation(nf, family, disp_hyper):
    """two groups, a fixed and a flat coefficient, offsets, weights with a dropped row, a linear term and a constant"""
    g, X, w, off = _data(1 + df.HYPERS.index(disp_hyper) + 10 * df.FAMILIES.index(family))
    G = 2
    grp = np.array([0, -1, 1, -1])
    sig = np.array([1.0, 1.7, 1.0, math.inf])
    hyper = ["halfnormal", "lognormal"]
    loc, scl = np.array([0.0, -0.2]), np.array([0.8, 1.7])
    lin = 0.5 * g.standard_normal(P_)
    k = g.poisson(3.0, ROWS).astype(np.float64)
    k[1], k[2] = 11.0, 40.0  # row 2 has weight 0: its count must not lengthen the table
    ys = g.standard_normal((P_ + G + 1, N_))
    ys[-1] = np.array([-1.0, 0.3, 2.5, 0.0, 1.1])
    tgt = nf.DispersionGLMTarget(family, _t(X), counts=_t(k) if family == "negbin" else None, groups=torch.tensor(grp), n_groups=G, offset=_t(off),
                                 weights=_t(w), lin=_t(lin), const=0.25, param=NU if family == "student" else 0.0, fixed_sigma=_t(sig), hyper=hyper,
                                 hyper_loc=_t(loc), hyper_scale=_t(scl), disp_hyper=disp_hyper, disp_loc=0.3, disp_scale=1.4)
    beta, tau, lam = ys[:P_], ys[P_:P_ + G], ys[-1]
    eta = X @ beta + off[:, None]
    direct = 0.25 + _loglik(family, eta, lam, w, k) + lin @ beta + _prior(beta, tau, lam, grp, sig, hyper, loc, scl, disp_hyper, 0.3, 1.4)
    got = df.ref_of(tgt)(ys)[0]
    _close(got, direct)
    for n in range(N_):
        _check_score(tgt, ys[:, n:n + 1])
    d = P_ + G + 1
    assert tgt.d == d and tgt.p == P_ and tgt.G == G and tgt.family == family and tgt.rows == ROWS and tgt.disp_hyper == disp_hyper
    assert tgt.A.shape == (ROWS, d) and not bool(tgt.A[:, P_:].any()) and torch.equal(tgt.A[:, :P_], _t(X))
    assert tgt.c.kind == DGLM_KINDS[family] and tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr()
    assert tgt.c.s0 == ROWS and tgt.c.s1 == G and tgt.A.dtype == torch.float64 and tgt.p0.dtype == torch.float64
    q = df.split_p0(tgt.p0.numpy(), d, ROWS, G, family == "negbin")
    assert list(q["gptr"]) == [0, 1, 2] and list(q["gidx"][:2]) == [0, 2] and list(q["hk"]) == [1, 0, df.HYPERS.index(disp_hyper)]
    assert list(q["isd"]) == [0.0, 1.0 / 1.7, 0.0, 0.0]
    if family == "negbin":
        live = w > 0
        M = int(k[live].max())
        assert q["par"][2] == M - 1 == tgt.table_len and np.array_equal(q["cnt"], k)
        assert np.allclose(q["ctab"], [w[live & (k > m)].sum() for m in range(1, M)], rtol=1e-15, atol=0)
        assert q["ctab"][-1] > 0 and tgt.p0.numel() == 4 * d + 3 * ROWS + 5 + G + M - 1
    else:
        assert q["par"][2] == 0 and tgt.p0.numel() == 4 * d + 2 * ROWS + 5 + G
        assert abs(q["lin"][d - 1] - (-w.sum() + (0.0 if disp_hyper == "lognormal" else 1.0))) <= 1e-14 * w.sum()  # (the order of the sum)
    yt = _t(ys)
    assert torch.equal(tgt.coefficients(yt), yt[:P_]) and torch.allclose(tgt.scales(yt), torch.exp(yt[P_:P_ + G]))
    assert torch.equal(tgt.dispersion(yt), torch.exp(yt[-1]))


def test_negbin_tends_to_poisson_and_short_tables(nf):
    """max k = 0, 1 (empty tables) and 2 (one entry) against gammaln; at lambda = 30 the likelihood is the Poisson one to 1e-9"""
    g, X, w, off = _data(5)
    ys = g.standard_normal((P_ + 1, N_))
    for maxk, mt in ((0, 0), (1, 0), (2, 1)):
        k = g.integers(0, maxk + 1, ROWS).astype(np.float64)
        k[0] = maxk
        tgt = nf.DispersionGLMTarget("negbin", _t(X), counts=_t(k), offset=_t(off), weights=_t(w), disp_hyper="lognormal")
        assert tgt.table_len == mt and tgt.G == 0 and tgt.d == P_ + 1
        eta = X @ ys[:P_] + off[:, None]
        direct = _loglik("negbin", eta, ys[-1], w, k) + stats.norm.logpdf(ys[:P_], 0.0, 1.0).sum(0) + stats.norm.logpdf(ys[-1], 0.0, 1.0)
        _close(df.ref_of(tgt)(ys)[0], direct)
        _check_score(tgt, ys[:, :1])
    k = g.poisson(3.0, ROWS).astype(np.float64)
    tgt = nf.DispersionGLMTarget("negbin", _t(X), counts=_t(k), offset=_t(off), weights=_t(w), disp_hyper="lognormal", disp_loc=30.0)
    big = ys.copy()
    big[-1] = 30.0
    eta = X @ big[:P_] + off[:, None]
    pois = (w[:, None] * stats.poisson.logpmf(k[:, None], np.exp(eta))).sum(0) + stats.norm.logpdf(big[:P_], 0.0, 1.0).sum(0) + \
        stats.norm.logpdf(30.0, 30.0, 1.0)
    _close(df.ref_of(tgt)(big)[0], pois, rtol=1e-9)


def test_named_regressions_against_scipy(nf):
    g, X, w, off = _data(7)
    y = g.standard_normal(ROWS)
    ys = g.standard_normal((P_ + 1, N_))
    b, lam = ys[:P_], ys[-1]
    prior = stats.norm.logpdf(b, 0.0, 2.0).sum(0) + stats.halfcauchy.logpdf(np.exp(lam), scale=1.5) + lam
    res = y[:, None] - X @ b
    tg = nf.GaussianRegressionTarget(_t(X), _t(y), weights=_t(w), fixed_sigma=2.0, disp_scale=1.5)
    _close(df.ref_of(tg)(ys)[0], (w[:, None] * stats.norm.logpdf(res, 0.0, np.exp(lam)[None, :])).sum(0) + prior)
    ts = nf.StudentRegressionTarget(_t(X), _t(y), NU, weights=_t(w), fixed_sigma=2.0, disp_scale=1.5)
    _close(df.ref_of(ts)(ys)[0], (w[:, None] * stats.t.logpdf(res, NU, scale=np.exp(lam)[None, :])).sum(0) + prior)
    k = g.poisson(2.0, ROWS)
    expo = g.uniform(0.5, 2.0, ROWS)
    tn = nf.NegativeBinomialRegressionTarget(_t(X), torch.tensor(k), exposure=_t(expo), weights=_t(w), fixed_sigma=2.0, disp_scale=1.5)
    r = np.exp(lam)[None, :]
    mean = expo[:, None] * np.exp(X @ b)
    _close(df.ref_of(tn)(ys)[0], (w[:, None] * stats.nbinom.logpmf(k[:, None], r, r / (r + mean))).sum(0) + prior, rtol=1e-11)
    for t in (tg, ts, tn):
        assert t.d == P_ + 1 and t.G == 0 and isinstance(t, nf.DispersionGLMTarget)
        _check_score(t, ys[:, :1])
    # the linear mixed model y ~ x + (1 | level)
    L, px = 3, 2
    lev = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1])
    tm = nf.LinearMixedModelTarget(_t(X[:, :px]), _t(y), torch.tensor(lev), L, weights=_t(w), fixed_sigma=2.0, hyper="halfnormal", hyper_scale=0.9,
                                   disp_hyper="lognormal", disp_loc=-0.2, disp_scale=0.7)
    assert tm.d == px + L + 2 and tm.p == px + L and tm.G == 1 and tm.n_levels == L
    assert np.array_equal(tm.A.numpy(), np.concatenate([X[:, :px], np.eye(L)[lev], np.zeros((ROWS, 2))], 1))
    ym = g.standard_normal((tm.d, N_))
    b, a, tau, lam = ym[:px], ym[px:px + L], ym[px + L], ym[-1]
    mu = X[:, :px] @ b + a[lev]
    direct = (w[:, None] * stats.norm.logpdf(y[:, None], mu, np.exp(lam)[None, :])).sum(0) + stats.norm.logpdf(b, 0.0, 2.0).sum(0) + \
        stats.norm.logpdf(a, 0.0, np.exp(tau)).sum(0) + stats.halfnorm.logpdf(np.exp(tau), scale=0.9) + tau + stats.norm.logpdf(lam, -0.2, 0.7)
    _close(df.ref_of(tm)(ym)[0], direct)
    _check_score(tm, ym[:, :1])
    t32 = nf.GaussianRegressionTarget(_t(X).float(), _t(y).float())
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32 and t32.disp_hyper == "halfcauchy"


def test_float32_floor_follows_the_reference(nf):
    """the op-by-op float32 evaluation of disp_forms (what the GPU tests pass as floor=) stays within float32's reach of the float64 one"""
    for family in df.FAMILIES:
        tgt = df.build(nf, family, 5, 2, 33, torch.float32, "cpu")
        ys = df.sample_ys(5, 37, False)
        (l64, g64), (l32, g32) = df.ref_of(tgt)(ys), df.ref_of(tgt)(ys.astype(np.float32))
        assert l32.dtype == np.float32 and g32.dtype == np.float32
        assert np.abs(l32 - l64).max() <= 1e-4 * np.abs(l64).max() and np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max()


def test_constructors_refuse_bad_arguments(nf):
    E = nf.NFHipError
    g, X, w, off = _data(13)
    X, w, off = _t(X), _t(w), _t(off)
    k = torch.tensor(g.poisson(2.0, ROWS))
    grp = torch.tensor([0, 1, -1, 0])
    D = nf.DispersionGLMTarget
    bad = [
        lambda: D("poisson", X),                                               # not a dispersion family
        lambda: D("normal", X[0]),                                             # not a matrix
        lambda: D("normal", X, counts=k),                                      # counts only for negbin
        lambda: D("student", X, counts=k, param=3.0),
        lambda: D("negbin", X),                                                # counts required
        lambda: D("negbin", X, counts=k[:-1]),
        lambda: D("negbin", X, counts=k.double() + 0.5),                       # not integers
        lambda: D("negbin", X, counts=-k - 1),
        lambda: D("negbin", X, counts=torch.full((ROWS,), 4098)),              # beyond the table
        lambda: D("negbin", X, counts=torch.full((ROWS,), math.nan, dtype=torch.float64)),
        lambda: D("student", X, param=0.0),
        lambda: D("normal", X, groups=torch.tensor([0, 2, -1, 0]), n_groups=2),  # a group index out of range
        lambda: D("normal", X, groups=grp),                                    # groups without n_groups
        lambda: D("normal", X, groups=grp[:-1], n_groups=2),
        lambda: D("normal", X, groups=grp.double(), n_groups=2),
        lambda: D("normal", X, n_groups=-1),
        lambda: D("normal", X, n_groups=1.5),
        lambda: D("normal", X, fixed_sigma=0.0),
        lambda: D("normal", X, fixed_sigma=math.nan),
        lambda: D("normal", X, groups=grp, n_groups=2, hyper="gamma"),
        lambda: D("normal", X, groups=grp, n_groups=2, hyper=["halfnormal"]),
        lambda: D("normal", X, groups=grp, n_groups=2, hyper_scale=0.0),
        lambda: D("normal", X, groups=grp, n_groups=2, hyper_loc=math.nan),
        lambda: D("normal", X, disp_hyper="gamma"),
        lambda: D("normal", X, disp_hyper=["halfnormal"]),
        lambda: D("normal", X, disp_scale=0.0),
        lambda: D("normal", X, disp_scale=math.inf),
        lambda: D("normal", X, disp_loc=math.nan),
        lambda: D("normal", X, weights=-w),
        lambda: D("normal", X, offset=off[:-1]),
        lambda: D("normal", X, lin=off),                                       # lin has p entries
        lambda: D("normal", X, const=math.nan),
        lambda: D("normal", torch.ones(4, 250, dtype=torch.float64), groups=torch.zeros(250, dtype=torch.int64), n_groups=6),  # p + G + 1 = 257
        lambda: nf.GaussianRegressionTarget(X, off[:-1]),
        lambda: nf.StudentRegressionTarget(X, off, 0.0),
        lambda: nf.NegativeBinomialRegressionTarget(X, k, exposure=-w),
        lambda: nf.LinearMixedModelTarget(X, off, torch.tensor([0, 1, 2, 3, 0, 1, 2, 0, 1]), 3),   # a level out of range
        lambda: nf.LinearMixedModelTarget(X, off, torch.tensor([0, 1, 2]), 3),
        lambda: nf.LinearMixedModelTarget(X, off, torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2]), 0),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(E):
            make()
            pytest.fail(f"case {i} was accepted")
    D("normal", torch.ones(4, 250, dtype=torch.float64), groups=torch.zeros(250, dtype=torch.int64), n_groups=5)  # p + G + 1 = 256
    D("negbin", X, counts=torch.full((ROWS,), 4097))                                                             # the largest count: 4096 entries
    assert D("negbin", X, counts=torch.full((ROWS,), 4097)).table_len == 4096


def test_existing_constructors_keep_their_buffers(nf):
    """LinearRegressionTarget / RobustRegressionTarget / VaryingInterceptTarget are untouched: layouts and kinds as before"""
    g, X, w, off = _data(17)
    t = nf.LinearRegressionTarget(_t(X), _t(off), 0.7, weights=_t(w))
    assert t.c.kind == 13 and t.p0.numel() == P_ + 2 * ROWS + 2
    t = nf.RobustRegressionTarget(_t(X), _t(off), 4.0, 0.7)
    assert t.c.kind == 12 and t.p0.numel() == P_ + 2 * ROWS + 2
    t = nf.VaryingInterceptTarget("normal", _t(X), torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0]), 2)
    assert t.c.kind == 20 and t.p0.numel() == 4 * t.d + 2 * ROWS + 3 + 1


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    X = torch.randn(4, 3, generator=torch.Generator().manual_seed(0))
    td = nf.DispersionGLMTarget("student", X, param=4.0)
    tn = nf.NegativeBinomialRegressionTarget(X, torch.tensor([0, 3, 1, 2]))
    for t in (td, tn):
        assert t.d == 4 and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
        assert not isinstance(t, nf.GLMTarget) and not isinstance(t, nf.HierarchicalGLMTarget)
        check_target(t, torch.float32, "cpu", 4)
        for args in ((torch.float64, "cpu", 4), (torch.float32, "cuda:0", 4), (torch.float32, "cpu", 3)):
            with pytest.raises(nf.NFHipError):
                check_target(t, *args)

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d):
            self.kind, self.theta = kind, torch.zeros(1)
            self.dist = type("D", (), {"d": d})()

    for t in (td, tn):
        for kind in ("planar", "radial", "meanfield"):
            assert ob._builtin(F(kind, 4), t) is False   # the closure route, with the device score
        assert ob._builtin(F("hamiltonian", 8), t) is False
        for kind in ("realnvp", "nsf", "composite", "fullrank"):
            assert ob._builtin(F(kind, 4), t) is True    # the library route
        with pytest.raises(nf.NFHipError):
            ob._builtin(F("planar", 3), t)


# ---- resources ---------------------------------------------------------------------------------------------------------------------
# (prefix, ceiling in bytes, why): new tiled instantiations that carry scratch at __launch_bounds__(256).  None does.
KNOWN = []


def test_disp_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_target_disp_tiled<", 12), ("void k_target_disp<", 6)):  # DB in {1, 2, 4, 8} x 3 row functions; {float, double} x 3
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        for name, agpr, vgpr, sgpr, scratch, lds in hit:
            cap = max([c for pre, c, _ in KNOWN if name.startswith(pre)], default=0)
            assert scratch <= cap, (name, scratch)
            assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole register file
            assert lds <= 4096, (name, lds)   # static LDS only (the tile, the images and the partial sums are dynamic)
    # the shipped forms keep their instantiation counts: the fourth form added kernels, it changed none
    for prefix, count in (("void k_target_hier_tiled<", 20), ("void k_target_hier<", 10), ("void k_target_glm_tiled<", 20), ("void k_target_glm<", 10)):
        assert len([r for r in rows if r[0].startswith(prefix)]) == count, prefix
