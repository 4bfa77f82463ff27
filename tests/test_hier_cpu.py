"""CPU checks of the hierarchical GLM targets (NF_TARGET_HGLM_LOGIT .. NF_TARGET_HGLM_NORMAL, kinds 16..20): the constants,
nf_target_check's argument conventions as nf_target_logp reports them BEFORE any device work (a stand-in context is enough),
the refusals of the flows that evaluate their target in their own kernels, the host folding of HierarchicalGLMTarget and
VaryingInterceptTarget against the model written directly with scipy.stats (norm, halfnorm, halfcauchy and the family's
log-likelihood, with the change of variables sigma = exp(tau)), the score of tests/hier_forms.py against central differences,
the constructors' refusals, the routing of the Python mirror and the new kernels' resources."""
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

import hier_forms as hf
from __graft_entry__ import ROOT, build, load_package

HGLM_KINDS = {"logit": 16, "probit": 17, "poisson": 18, "student": 19, "normal": 20}


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
    for fam, v in HGLM_KINDS.items():
        name = "NF_TARGET_HGLM_" + fam.upper()
        assert defs[name] == getattr(nf._lib, name) == v == defs["NF_TARGET_GLM_" + fam.upper()] + 7
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    for absent in (7, 14):
        assert absent not in defs.values()
    from normalizingflows_jl_amd import flows

    assert flows._HGLM_KINDS == HGLM_KINDS and flows._HYPER_KINDS == {"lognormal": 0, "halfnormal": 1, "halfcauchy": 2}
    assert nf.load_library().nf_abi_version() == 4


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) for every violated convention of kinds 16..20 without touching the context (N = 0: nothing is launched,
    and a good target's answer is no error).  d > 256 is answered by the launcher, as for the siblings."""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=6, n=4, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)

    for kind in HGLM_KINDS.values():
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
            assert logp(Target(kind, p, p, 8.0, 6.0), dtype=dtype) == -1             # G = d: no coefficient left
            assert logp(Target(kind, p, p, 8.0, 7.0), dtype=dtype) == -1             # G > d
            assert logp(Target(kind, p, p, 8.0, math.inf), dtype=dtype) == -1
            assert logp(Target(kind, p, p, 8.0, 1.0), d=1, dtype=dtype) == -1        # d = 1 leaves room for no log-scale
            assert logp(Target(kind, p, p, 8.0, 0.0), n=0, dtype=dtype) >= 0         # G = 0: past the check
            assert logp(Target(kind, p, p, 8.0, 5.0), n=0, dtype=dtype) >= 0         # G = d - 1
            assert logp(Target(kind, p, p, 8.0, 0.0), d=1, n=0, dtype=dtype) >= 0
            assert logp(Target(kind, p, p, 2147483647.0, 2.0), n=0, dtype=dtype) >= 0
    assert logp(Target(7, p, p, 8.0, 2.0)) == -1 and logp(Target(14, p, p, 8.0, 2.0)) == -1 and logp(Target(21, p, p, 8.0, 2.0)) == -1


def _five(lib, ctx, p, val, desc, tgt):
    return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
            lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
            lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
            lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
            lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with
    a hierarchical kind as the target and as the Hamiltonian score -- the stand-in context is never used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    for tk in HGLM_KINDS.values():
        hg = Target(tk, p.value, p.value, 4.0, 1.0)
        for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1), ("planar", 1)):
            desc = FlowDesc()
            desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
            assert _five(lib, ctx, p, val, desc, hg) == [-2] * 5, (kind, tk)
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
        hd.score = C.cast(C.pointer(diag), C.c_void_p)  # a supported score, a hierarchical ELBO target
        assert _five(lib, ctx, p, val, hd, hg) == [-2] * 5, tk
        hd.score = C.cast(C.pointer(hg), C.c_void_p)    # a hierarchical score
        assert _five(lib, ctx, p, val, hd, diag) == [-2] * 5, tk


def test_realnvp_and_fullrank_get_past_every_refusal(nf):
    """RealNVP and full-rank descriptors of either element type with a hierarchical kind: the ELBO entry points get past every
    refusal that comes before device work and stop at the stand-in context's device ordinal (a positive HIP error code); the graph
    form is never an argument error (its NF_ERR_UNSUPPORTED comes after the device ordinal for RealNVP: test_gpu_hier.py)"""
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
            for tk in HGLM_KINDS.values():
                got = _five(lib, ctx, p, val, desc, Target(tk, p.value, p.value, 4.0, 2.0))
                assert all(c > 0 for c in got[:4]) and (got[4] > 0 or got[4] == -2), (kind, dtype, tk, got)


# ---- host folding ---------------------------------------------------------------------------------------------------------------
P_, ROWS, N_ = 5, 7, 5


def _data(seed=0):
    g = np.random.default_rng(seed)
    X = g.standard_normal((ROWS, P_)) / np.sqrt(P_)
    w = g.uniform(0.3, 2.5, ROWS)
    w[2] = 0.0  # one dropped row
    off = 0.4 * g.standard_normal(ROWS)
    return g, X, w, off


def _likelihood(family, eta, w, nu=3.5):
    if family == "logit":
        ll = stats.bernoulli.logpmf(1, sp.expit(eta))
    elif family == "probit":
        ll = stats.norm.logcdf(eta)
    elif family == "poisson":
        ll = -np.exp(eta)
    elif family == "student":
        ll = stats.t.logpdf(eta, nu) - (sp.gammaln(0.5 * (nu + 1)) - sp.gammaln(0.5 * nu) - 0.5 * np.log(nu * np.pi))
    else:
        ll = stats.norm.logpdf(eta) + 0.5 * np.log(2.0 * np.pi)
    return (w[:, None] * ll).sum(0)


def _textbook(family, X, w, off, lin, const, grp, sig, hyper, loc, scl, ys):
    """the joint log-density over (beta, tau) written with scipy.stats: sigma_g = exp(tau_g) has the named density, and the density
    over tau_g carries the Jacobian d sigma / d tau = sigma"""
    p, G = X.shape[1], len(hyper)
    beta, tau = ys[:p], ys[p:]
    out = const + _likelihood(family, X @ beta + off[:, None], w) + lin @ beta
    for j in range(p):
        if grp[j] >= 0:
            out = out + stats.norm.logpdf(beta[j], 0.0, np.exp(tau[grp[j]]))
        elif np.isfinite(sig[j]):
            out = out + stats.norm.logpdf(beta[j], 0.0, sig[j])
    for g in range(G):
        s = np.exp(tau[g])
        if hyper[g] == "lognormal":
            out = out + stats.norm.logpdf(tau[g], loc[g], scl[g])
        elif hyper[g] == "halfnormal":
            out = out + stats.halfnorm.logpdf(s, scale=scl[g]) + tau[g]
        else:
            out = out + stats.halfcauchy.logpdf(s, scale=scl[g]) + tau[g]
    return out


def _folded(tgt, ys):
    return hf.ref_of(tgt)(ys)


def _check_score(tgt, y0):
    sc = _folded(tgt, y0)[1][:, 0]
    for i in range(tgt.d):
        e = np.zeros_like(y0)
        e[i] = 1e-6
        fd = (_folded(tgt, y0 + e)[0][0] - _folded(tgt, y0 - e)[0][0]) / 2e-6
        assert abs(fd - sc[i]) <= 1e-7 * max(1.0, abs(sc[i])), (i, fd, sc[i])


@pytest.mark.parametrize("hyper", hf.HYPERS)
@pytest.mark.parametrize("family", hf.FAMILIES)
def test_folding_against_scipy_one_hyper_prior(nf, family, hyper):
    """every coefficient in one of two groups, both under the same hyper-prior form"""
    g, X, w, off = _data(1 + hf.HYPERS.index(hyper))
    G = 2
    grp = np.array([0, 1, 0, 0, 1])
    lin = 0.5 * g.standard_normal(P_)
    loc, scl = np.array([0.3, -0.2]), np.array([0.8, 1.7])
    ys = g.standard_normal((P_ + G, N_))
    tgt = nf.HierarchicalGLMTarget(family, _t(X), torch.tensor(grp), G, offset=_t(off), weights=_t(w), lin=_t(lin), const=0.25,
                                   param=3.5 if family == "student" else 0.0, hyper=hyper, hyper_loc=_t(loc), hyper_scale=_t(scl))
    direct = _textbook(family, X, w, off, lin, 0.25, grp, np.ones(P_), [hyper] * G, loc, scl, ys)
    got = _folded(tgt, ys)[0]
    assert got.shape == direct.shape == (N_,)
    assert (np.abs(got - direct) <= 1e-12 * np.maximum(1.0, np.abs(direct))).all(), (got, direct)
    _check_score(tgt, ys[:, :1])
    d = P_ + G
    assert tgt.d == d and tgt.p == P_ and tgt.G == G and tgt.family == family and tgt.rows == ROWS
    assert tgt.A.shape == (ROWS, d) and not bool(tgt.A[:, P_:].any()) and torch.equal(tgt.A[:, :P_], _t(X))
    assert tgt.A.dtype == torch.float64 and tgt.p0.dtype == torch.float64 and tgt.p0.shape == (4 * d + 2 * ROWS + 3 + G,)
    assert tgt.c.kind == HGLM_KINDS[family] and tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr()
    assert tgt.c.s0 == ROWS and tgt.c.s1 == G
    q = hf.split_p0(tgt.p0.numpy(), d, ROWS, G)
    assert list(q["gptr"]) == [0, 3, 5] and list(q["gidx"]) == [0, 2, 3, 1, 4]  # members in increasing feature index


@pytest.mark.parametrize("family", ["poisson", "normal"])
def test_folding_against_scipy_mixed_fixed_and_grouped(nf, family):
    """fixed-scale, flat and grouped coefficients, one hyper-prior of each form and a group without a member"""
    g, X, w, off = _data(7)
    G = 4
    grp = np.array([-1, 2, 0, -1, 2])
    sig = np.array([1.7, 1.0, 1.0, math.inf, 1.0])
    hyper = ["halfcauchy", "lognormal", "halfnormal", "lognormal"]  # groups 1 and 3 have no member
    loc, scl = np.array([0.0, 0.4, 0.0, -0.3]), np.array([2.5, 0.6, 0.9, 1.2])
    ys = g.standard_normal((P_ + G, N_))
    tgt = nf.HierarchicalGLMTarget(family, _t(X), torch.tensor(grp), G, offset=_t(off), weights=_t(w), fixed_sigma=_t(sig), hyper=hyper,
                                   hyper_loc=_t(loc), hyper_scale=_t(scl))
    direct = _textbook(family, X, w, off, np.zeros(P_), 0.0, grp, sig, hyper, loc, scl, ys)
    got = _folded(tgt, ys)[0]
    assert (np.abs(got - direct) <= 1e-12 * np.maximum(1.0, np.abs(direct))).all(), (got, direct)
    _check_score(tgt, ys[:, :1])
    q = hf.split_p0(tgt.p0.numpy(), P_ + G, ROWS, G)
    assert list(q["grp"]) == list(grp) and list(q["isd"]) == [1.0 / 1.7, 0.0, 0.0, 0.0, 0.0] and list(q["hk"]) == [2, 0, 1, 0]
    assert list(q["gptr"]) == [0, 1, 1, 3, 3] and list(q["gidx"][:3]) == [2, 1, 4]
    # defaults, scalars and Float32
    t32 = nf.HierarchicalGLMTarget(family, _t(X).float(), torch.tensor(grp), G)
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32 and t32.hyper == ["halfcauchy"] * 4


def test_no_group_is_the_glm_target(nf):
    """G = 0 with one common fixed sigma is GLMTarget(prior_sigma): the same density from the two folded buffers"""
    import glm_forms as gf

    g, X, w, off = _data(9)
    ys = g.standard_normal((P_, N_))
    none = torch.full((P_,), -1, dtype=torch.int64)
    for sigma in (1.7, math.inf):
        h = nf.HierarchicalGLMTarget("logit", _t(X), none, 0, offset=_t(off), weights=_t(w), const=0.5, fixed_sigma=sigma)
        t = nf.GLMTarget("logit", _t(X), offset=_t(off), weights=_t(w), const=0.5, prior_sigma=sigma)
        a, b = _folded(h, ys), gf.ref_of(t)(ys)
        assert h.d == P_ and h.G == 0 and h.c.s1 == 0.0
        assert np.allclose(a[0], b[0], rtol=1e-13, atol=0) and np.allclose(a[1], b[1], rtol=1e-13, atol=1e-15)


def test_varying_intercepts_against_scipy(nf):
    g, X, w, off = _data(11)
    L = 3
    lev = np.array([0, 2, 1, 1, 0, 2, 2])
    px = 2
    Xf = X[:, :px]
    k = g.poisson(2.0, ROWS).astype(np.float64)
    # Poisson counts: lin and const as PoissonRegressionTarget folds them, over A = [X | one-hot]
    A = np.concatenate([Xf, np.eye(L)[lev]], 1)
    lin = (w * k) @ A
    const = float((w * (k * off - sp.gammaln(k + 1.0))).sum())
    tgt = nf.VaryingInterceptTarget("poisson", _t(Xf), torch.tensor(lev), L, offset=_t(off), weights=_t(w), lin=_t(lin), const=const,
                                    fixed_sigma=2.0, hyper="halfnormal", hyper_scale=1.5)
    assert tgt.d == px + L + 1 and tgt.p == px + L and tgt.G == 1 and tgt.n_levels == L
    assert np.array_equal(tgt.A.numpy(), np.concatenate([A, np.zeros((ROWS, 1))], 1))
    ys = g.standard_normal((tgt.d, N_))
    b, a, tau = ys[:px], ys[px:px + L], ys[px + L]
    eta = Xf @ b + a[lev] + off[:, None]
    direct = (w[:, None] * stats.poisson.logpmf(k[:, None], np.exp(eta))).sum(0) + stats.norm.logpdf(b, 0.0, 2.0).sum(0) + \
        stats.norm.logpdf(a, 0.0, np.exp(tau)).sum(0) + stats.halfnorm.logpdf(np.exp(tau), scale=1.5) + tau
    got = _folded(tgt, ys)[0]
    assert (np.abs(got - direct) <= 1e-12 * np.maximum(1.0, np.abs(direct))).all(), (got, direct)
    assert torch.equal(tgt.coefficients(_t(ys)), _t(ys[:px + L])) and torch.allclose(tgt.scales(_t(ys)), _t(np.exp(ys[px + L:])))


def test_each_hyper_prior_integrates_to_one():
    """exp(h(tau - hm) + the folded normaliser + the Jacobian term) over tau, by the trapezoid rule on a wide grid"""
    tau = np.linspace(-40.0, 12.0, 520001)
    s = 1.7
    for kind, logc, jac in ((0, math.log(1.0 / 0.8) - 0.5 * math.log(2 * math.pi), 0.0), (1, 0.5 * math.log(2 / math.pi) - math.log(s), 1.0),
                            (2, math.log(2 / math.pi) - math.log(s), 1.0)):
        hm = 0.3 if kind == 0 else math.log(s)
        hv, _ = hf.hyper(kind, tau - hm, 1.0 / 0.8)
        f = np.exp(hv + logc + jac * tau)
        total = float(((f[1:] + f[:-1]) * 0.5 * np.diff(tau)).sum())
        assert abs(total - 1.0) <= (2e-5 if kind == 2 else 1e-9), (kind, total)  # the half-Cauchy's tail beyond e^12 holds 2 s / (pi e^12)


def test_constructors_refuse_bad_arguments(nf):
    E = nf.NFHipError
    _, X, w, off = _data(13)
    X, w, off = _t(X), _t(w), _t(off)
    grp = torch.tensor([0, 1, -1, 0, 1])
    H = nf.HierarchicalGLMTarget
    bad = [
        lambda: H("cloglog", X, grp, 2),
        lambda: H("logit", X[0], grp, 2),                                      # not a matrix
        lambda: H("logit", X, torch.tensor([0, 2, -1, 0, 1]), 2),              # a group index out of range
        lambda: H("logit", X, torch.tensor([0, -2, -1, 0, 1]), 2),
        lambda: H("logit", X, grp[:-1], 2),                                    # a wrong length
        lambda: H("logit", X, grp.double(), 2),                                # not an integer tensor
        lambda: H("logit", X, grp, -1),
        lambda: H("logit", X, grp, 2.5),
        lambda: H("logit", X, grp, 2, fixed_sigma=0.0),
        lambda: H("logit", X, grp, 2, fixed_sigma=-1.0),
        lambda: H("logit", X, grp, 2, fixed_sigma=math.nan),
        lambda: H("logit", X, grp, 2, fixed_sigma=_t([1.0, 1.0, 0.0, 1.0, 1.0])),
        lambda: H("logit", X, grp, 2, fixed_sigma=_t([1.0, 1.0])),
        lambda: H("logit", X, grp, 2, hyper="gamma"),                          # an unknown hyper-prior
        lambda: H("logit", X, grp, 2, hyper=["halfnormal"]),                   # one per group
        lambda: H("logit", X, grp, 2, hyper=["halfnormal", "wishart"]),
        lambda: H("logit", X, grp, 2, hyper_scale=0.0),
        lambda: H("logit", X, grp, 2, hyper_scale=math.inf),
        lambda: H("logit", X, grp, 2, hyper_loc=math.nan),
        lambda: H("logit", X, grp, 2, hyper_loc=_t([0.0, 0.0, 0.0])),
        lambda: H("logit", X, grp, 2, weights=-w),
        lambda: H("logit", X, grp, 2, offset=off[:-1]),
        lambda: H("logit", X, grp, 2, lin=off),                                # lin has p entries
        lambda: H("logit", X, grp, 2, const=math.nan),
        lambda: H("student", X, grp, 2, param=0.0),
        lambda: H("logit", torch.ones(4, 250, dtype=torch.float64), torch.zeros(250, dtype=torch.int64), 7),  # p + G = 257
        lambda: nf.VaryingInterceptTarget("logit", X, torch.tensor([0, 1, 2, 3, 0, 1, 2]), 3),                # a level out of range
        lambda: nf.VaryingInterceptTarget("logit", X, torch.tensor([0, 1, 2]), 3),
        lambda: nf.VaryingInterceptTarget("logit", X, torch.tensor([0, 1, 2, 0, 1, 2, 0]), 0),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(E):
            make()
            pytest.fail(f"case {i} was accepted")
    H("logit", torch.ones(4, 250, dtype=torch.float64), torch.zeros(250, dtype=torch.int64), 6)  # p + G = 256
    H("logit", X, grp, 5, weights=w, fixed_sigma=math.inf)                                       # groups without members: fine


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    X = torch.randn(4, 3, generator=torch.Generator().manual_seed(0))
    th = nf.HierarchicalGLMTarget("probit", X, torch.tensor([0, -1, 0]), 1)
    tv = nf.VaryingInterceptTarget("poisson", X[:, :1], torch.tensor([0, 1, 1, 0]), 2)
    for t in (th, tv):
        assert t.d == 4 and isinstance(t, nf.HierarchicalGLMTarget) and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
        assert not isinstance(t, nf.GLMTarget)
        check_target(t, torch.float32, "cpu", 4)
        for args in ((torch.float64, "cpu", 4), (torch.float32, "cuda:0", 4), (torch.float32, "cpu", 3)):
            with pytest.raises(nf.NFHipError):
                check_target(t, *args)

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d):
            self.kind, self.theta = kind, torch.zeros(1)
            self.dist = type("D", (), {"d": d})()

    for t in (th, tv):
        for kind in ("planar", "radial", "meanfield"):
            assert ob._builtin(F(kind, 4), t) is False   # the closure route, with the device score
        assert ob._builtin(F("hamiltonian", 8), t) is False
        for kind in ("realnvp", "nsf", "composite", "fullrank"):
            assert ob._builtin(F(kind, 4), t) is True    # the library route
        with pytest.raises(nf.NFHipError):
            ob._builtin(F("planar", 3), t)


# ---- resources ---------------------------------------------------------------------------------------------------------------------
def test_hier_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_target_hier_tiled<", 20), ("void k_target_hier<", 10)):  # DB in {1, 2, 4, 8} x 5 phi; {float, double} x 5 phi
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        for name, agpr, vgpr, sgpr, scratch, lds in hit:
            assert "k_target_glm" not in name and "k_target_linpred" not in name
            assert scratch == 0, (name, scratch)
            assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole register file
            assert lds <= 4096, (name, lds)   # static LDS only (the tile and the images are dynamic)
