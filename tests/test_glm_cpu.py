"""CPU checks of the generalised linear-predictor targets (NF_TARGET_GLM_LOGIT .. NF_TARGET_GLM_NORMAL, kinds 9..13): the
constants, nf_target_check's argument conventions as nf_target_logp reports them BEFORE any device work (a stand-in context
is enough), the refusals of the flows that evaluate their target in their own kernels, the host folding of every convenience
constructor against the model written directly with scipy.stats, the constructors' refusals, the routing of the Python mirror
and the new kernels' resources."""
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

import glm_forms as gf
from __graft_entry__ import ROOT, build, load_package

GLM_KINDS = {"logit": 9, "probit": 10, "poisson": 11, "student": 12, "normal": 13}


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def test_constants_match_the_header_and_kind_7_stays_absent(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M)}
    want = {"NF_TARGET_GLM_LOGIT": 9, "NF_TARGET_GLM_PROBIT": 10, "NF_TARGET_GLM_POISSON": 11, "NF_TARGET_GLM_STUDENT": 12,
            "NF_TARGET_GLM_NORMAL": 13}
    for name, v in want.items():
        assert defs[name] == getattr(nf._lib, name) == v
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    assert 7 not in defs.values()
    assert 7 not in [v for k, v in vars(nf._lib).items() if k.startswith("NF_TARGET_")]
    from normalizingflows_jl_amd import flows

    assert flows._GLM_KINDS == GLM_KINDS


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) for every violated convention of kinds 9..13 without touching the context; s1 = +inf (the flat prior)
    passes the check (N = 0: nothing is launched, and the answer is no argument error)."""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, n=4, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), 3, n, C.c_void_p(p), C.c_void_p(p), None)

    for kind in GLM_KINDS.values():
        for dtype in (0, 1):
            assert logp(Target(kind, 0, p, 8.0, 1.0), dtype=dtype) == -1            # p0 = NULL
            assert logp(Target(kind, p, 0, 8.0, 1.0), dtype=dtype) == -1            # p1 = NULL
            assert logp(Target(kind, p, p, 0.0, 1.0), dtype=dtype) == -1            # rows = 0
            assert logp(Target(kind, p, p, -3.0, 1.0), dtype=dtype) == -1           # negative rows
            assert logp(Target(kind, p, p, 2.5, 1.0), dtype=dtype) == -1            # rows not integral
            assert logp(Target(kind, p, p, 2147483648.0, 1.0), dtype=dtype) == -1   # rows = 2^31
            assert logp(Target(kind, p, p, math.nan, 1.0), dtype=dtype) == -1       # NaN rows
            assert logp(Target(kind, p, p, 8.0, 0.0), dtype=dtype) == -1            # prior sigma = 0
            assert logp(Target(kind, p, p, 8.0, -1.0), dtype=dtype) == -1           # negative
            assert logp(Target(kind, p, p, 8.0, math.nan), dtype=dtype) == -1       # NaN
            assert logp(Target(kind, p, p, 8.0, math.inf), n=0, dtype=dtype) >= 0   # flat prior: past the check
            assert logp(Target(kind, p, p, 8.0, 2.0), n=0, dtype=dtype) >= 0
    assert logp(Target(7, p, p, 8.0, 1.0)) == -1 and logp(Target(14, p, p, 8.0, 1.0)) == -1  # no such kinds


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with
    a GLM kind as the target and with a GLM kind as the Hamiltonian score -- the stand-in context is never used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)

    def five(desc, tgt):
        return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
                lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
                lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
                lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
                lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]

    diag = Target(0, p.value, p.value, 0.0, 0.0)
    for tk in GLM_KINDS.values():
        glm = Target(tk, p.value, p.value, 4.0, 1.0)
        for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1), ("planar", 1)):
            desc = FlowDesc()
            desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
            assert five(desc, glm) == [-2] * 5, (kind, tk)
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
        hd.score = C.cast(C.pointer(diag), C.c_void_p)  # a supported score, a GLM ELBO target
        assert five(hd, glm) == [-2] * 5, tk
        hd.score = C.cast(C.pointer(glm), C.c_void_p)   # a GLM score
        assert five(hd, diag) == [-2] * 5, tk


# ---- host folding ---------------------------------------------------------------------------------------------------------------
D, ROWS = 3, 7


def _data(seed=0):
    g = np.random.default_rng(seed)
    X = g.standard_normal((ROWS, D)) / np.sqrt(D)
    w = g.uniform(0.3, 2.5, ROWS)
    w[2] = 0.0  # one dropped row
    off = 0.4 * g.standard_normal(ROWS)
    ys = g.standard_normal((D, 5))
    return g, X, w, off, ys


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _prior(ys, sigma):
    return stats.norm.logpdf(ys, 0.0, sigma).sum(0)


def _folded(tgt, ys):
    A, p0 = gf.target_arrays(tgt)
    return gf.logp_score(tgt.family, ys, A, p0, tgt.prior_sigma)[0]


def _agree(tgt, ys, direct):
    got = _folded(tgt, ys)
    assert got.shape == direct.shape == (5,)
    assert (np.abs(got - direct) <= 1e-12 * np.abs(direct)).all(), (got, direct)
    assert tgt.A.dtype == torch.float64 and tgt.p0.dtype == torch.float64 and tgt.p0.shape == (D + 2 * ROWS + 2,)
    assert tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr() and tgt.c.s0 == ROWS and tgt.c.s1 == tgt.prior_sigma
    assert tgt.c.kind == GLM_KINDS[tgt.family]


def test_poisson_folding(nf):
    g, X, w, _, ys = _data(1)
    k = g.poisson(3.0, ROWS).astype(np.float64)
    expo = g.uniform(0.5, 3.0, ROWS)
    tgt = nf.PoissonRegressionTarget(_t(X), _t(k), exposure=_t(expo), weights=_t(w), prior_sigma=1.7)
    direct = (w[:, None] * stats.poisson.logpmf(k[:, None], expo[:, None] * np.exp(X @ ys))).sum(0) + _prior(ys, 1.7)
    _agree(tgt, ys, direct)
    assert tgt.family == "poisson"
    tgt_i = nf.PoissonRegressionTarget(_t(X), torch.tensor(k, dtype=torch.int64), exposure=_t(expo), weights=_t(w), prior_sigma=1.7)
    assert torch.equal(tgt_i.p0, tgt.p0)  # integer counts are the same data


def test_binomial_folding_and_the_bernoulli_case(nf):
    g, X, w, off, ys = _data(2)
    n = g.integers(1, 9, ROWS).astype(np.float64)
    k = np.array([g.integers(0, int(m) + 1) for m in n], dtype=np.float64)
    tgt = nf.BinomialRegressionTarget(_t(X), _t(k), _t(n), offset=_t(off), weights=_t(w), prior_sigma=2.0)
    eta = X @ ys + off[:, None]
    direct = (w[:, None] * stats.binom.logpmf(k[:, None], n[:, None], sp.expit(eta))).sum(0) + _prior(ys, 2.0)
    _agree(tgt, ys, direct)
    assert tgt.family == "logit"
    ones = np.ones(ROWS)
    kb = g.integers(0, 2, ROWS).astype(np.float64)
    tb = nf.BinomialRegressionTarget(_t(X), _t(kb), _t(ones), offset=_t(off), weights=_t(w), prior_sigma=2.0)
    bern = (w[:, None] * stats.bernoulli.logpmf(kb[:, None], sp.expit(eta))).sum(0) + _prior(ys, 2.0)
    _agree(tb, ys, bern)


def test_probit_folding(nf):
    g, X, w, off, ys = _data(3)
    lab = g.integers(0, 2, ROWS)
    tgt = nf.ProbitRegressionTarget(_t(X), torch.tensor(lab), offset=_t(off), weights=_t(w), prior_sigma=0.8)
    sign = 2.0 * lab - 1.0
    direct = (w[:, None] * stats.norm.logcdf(sign[:, None] * (X @ ys + off[:, None]))).sum(0) + _prior(ys, 0.8)
    _agree(tgt, ys, direct)
    same = nf.ProbitRegressionTarget(_t(X), _t(sign), offset=_t(off), weights=_t(w), prior_sigma=0.8)
    assert torch.equal(same.A, tgt.A) and torch.equal(same.p0, tgt.p0)  # {-1, +1} labels


def test_robust_folding(nf):
    g, X, w, _, ys = _data(4)
    yobs = g.standard_normal(ROWS) * 2.0
    tgt = nf.RobustRegressionTarget(_t(X), _t(yobs), 3.5, 0.7, weights=_t(w), prior_sigma=1.3)
    direct = (w[:, None] * stats.t.logpdf(yobs[:, None], 3.5, loc=X @ ys, scale=0.7)).sum(0) + _prior(ys, 1.3)
    _agree(tgt, ys, direct)
    assert tgt.param == 3.5 and float(tgt.p0[-2]) == 3.5


def test_linear_folding_and_the_flat_prior(nf):
    g, X, w, _, ys = _data(5)
    yobs = g.standard_normal(ROWS)
    tgt = nf.LinearRegressionTarget(_t(X), _t(yobs), 0.6, weights=_t(w), prior_sigma=1.1)
    like = (w[:, None] * stats.norm.logpdf(yobs[:, None], X @ ys, 0.6)).sum(0)
    _agree(tgt, ys, like + _prior(ys, 1.1))
    flat = nf.LinearRegressionTarget(_t(X), _t(yobs), 0.6, weights=_t(w), prior_sigma=math.inf)
    _agree(flat, ys, like)
    assert math.isinf(flat.c.s1)


def test_raw_form_defaults(nf):
    g, X, _, _, ys = _data(6)
    tgt = nf.GLMTarget("student", _t(X), param=4.0)
    assert torch.equal(tgt.p0, torch.cat([torch.zeros(D + ROWS), torch.ones(ROWS), torch.tensor([4.0, 0.0])]).double())
    direct = stats.t.logpdf(X @ ys, 4.0).sum(0) - ROWS * (sp.gammaln(2.5) - sp.gammaln(2.0) - 0.5 * np.log(4.0 * np.pi)) + _prior(ys, 1.0)
    _agree(tgt, ys, direct)
    t32 = nf.GLMTarget("normal", _t(X).float())
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32


def test_constructors_refuse_bad_arguments(nf):
    E = nf.NFHipError
    _, X, w, off, _ = _data(7)
    X, w, off = _t(X), _t(w), _t(off)
    k, n1, y = _t(np.arange(ROWS)), _t(np.full(ROWS, 9.0)), _t(np.linspace(-1, 1, ROWS))
    lab = torch.tensor([0, 1] * 3 + [1])
    bad = [
        lambda: nf.GLMTarget("cloglog", X),
        lambda: nf.GLMTarget("logit", X[0]),                                   # not a matrix
        lambda: nf.GLMTarget("logit", X.to(torch.float16)),
        lambda: nf.GLMTarget("logit", X, offset=off[:-1]),                     # shapes
        lambda: nf.GLMTarget("logit", X, weights=w[:-1]),
        lambda: nf.GLMTarget("logit", X, lin=off),                             # lin has d entries
        lambda: nf.GLMTarget("logit", X, offset=off.float()),                  # element types differ
        lambda: nf.GLMTarget("logit", X, weights=w.to("meta")),                # devices differ
        lambda: nf.GLMTarget("logit", X, weights=-w),
        lambda: nf.GLMTarget("logit", X, offset=off * math.nan),
        lambda: nf.GLMTarget("logit", X * math.inf),
        lambda: nf.GLMTarget("logit", X, const=math.nan),
        lambda: nf.GLMTarget("student", X, param=0.0),                         # nu <= 0
        lambda: nf.GLMTarget("student", X, param=-1.0),
        lambda: nf.GLMTarget("logit", X, prior_sigma=0.0),
        lambda: nf.GLMTarget("logit", X, prior_sigma=-math.inf),
        lambda: nf.GLMTarget("logit", X, prior_sigma=math.nan),
        lambda: nf.PoissonRegressionTarget(X, -k),                             # negative counts
        lambda: nf.PoissonRegressionTarget(X, k + 0.5),
        lambda: nf.PoissonRegressionTarget(X, k[:-1]),
        lambda: nf.PoissonRegressionTarget(X, k, exposure=w),                  # an exposure of 0
        lambda: nf.PoissonRegressionTarget(X, k, weights=-w),
        lambda: nf.PoissonRegressionTarget(X, k.float()),
        lambda: nf.BinomialRegressionTarget(X, n1 + 1.0, n1),                  # successes > trials
        lambda: nf.BinomialRegressionTarget(X, -k, n1),
        lambda: nf.BinomialRegressionTarget(X, k, n1, weights=-w),
        lambda: nf.BinomialRegressionTarget(X, k, n1[:-1]),
        lambda: nf.ProbitRegressionTarget(X, torch.tensor([0, 1, 2, 0, 1, 0, 1])),
        lambda: nf.ProbitRegressionTarget(X, torch.tensor([-1, 1, 0, 1, 1, 1, 1])),
        lambda: nf.ProbitRegressionTarget(X, lab, weights=-w),
        lambda: nf.ProbitRegressionTarget(X, lab, offset=off * math.inf),
        lambda: nf.RobustRegressionTarget(X, y, 0.0, 1.0),                     # nu <= 0
        lambda: nf.RobustRegressionTarget(X, y, -2.0, 1.0),
        lambda: nf.RobustRegressionTarget(X, y, 3.0, 0.0),                     # scale <= 0
        lambda: nf.RobustRegressionTarget(X, y, 3.0, -1.0),
        lambda: nf.RobustRegressionTarget(X, y, 3.0, 1.0, weights=-w),
        lambda: nf.RobustRegressionTarget(X, y * math.nan, 3.0, 1.0),
        lambda: nf.RobustRegressionTarget(X, y.float(), 3.0, 1.0),
        lambda: nf.LinearRegressionTarget(X, y, 0.0),
        lambda: nf.LinearRegressionTarget(X, y, 1.0, weights=-w),
        lambda: nf.LinearRegressionTarget(X, y[:-1], 1.0),
        lambda: nf.LinearRegressionTarget(X, y, 1.0, prior_sigma=0.0),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(E):
            make()
            pytest.fail(f"case {i} was accepted")
    nf.PoissonRegressionTarget(X, k, exposure=w + 0.1, weights=w, prior_sigma=math.inf)  # zero weights, a flat prior: fine


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    X = torch.randn(4, 3, generator=torch.Generator().manual_seed(0))
    tp = nf.PoissonRegressionTarget(X, torch.tensor([0, 2, 1, 5]))
    tg = nf.GLMTarget("probit", X)
    for t in (tp, tg):
        assert isinstance(t, nf.GLMTarget) and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
        check_target(t, torch.float32, "cpu", 3)
        for args in ((torch.float64, "cpu", 3), (torch.float32, "cuda:0", 3), (torch.float32, "cpu", 4)):
            with pytest.raises(nf.NFHipError):
                check_target(t, *args)

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d):
            self.kind, self.theta = kind, torch.zeros(1)
            self.dist = type("D", (), {"d": d})()

    for t in (tp, tg):
        for kind in ("planar", "radial", "meanfield"):
            assert ob._builtin(F(kind, 3), t) is False   # the closure route, with the device score
        assert ob._builtin(F("hamiltonian", 6), t) is False
        for kind in ("realnvp", "nsf", "composite"):
            assert ob._builtin(F(kind, 3), t) is True    # the library route
        with pytest.raises(nf.NFHipError):
            ob._builtin(F("planar", 4), t)


def test_glm_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = [r for r in kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build")) if "k_target_glm" in r[0]]
    tiled = [r for r in rows if "k_target_glm_tiled<" in r[0]]
    flat = [r for r in rows if "k_target_glm<" in r[0]]
    assert len(tiled) == 20 and len(flat) == 10, [r[0][:60] for r in rows]  # DB in {1, 2, 4, 8} x 5 phi; {float, double} x 5 phi
    for name, agpr, vgpr, sgpr, scratch, lds in rows:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole register file
        assert lds <= 4096, (name, lds)   # static LDS only (the tile and the images are dynamic)
