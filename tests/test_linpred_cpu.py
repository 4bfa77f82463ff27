"""CPU checks of the linear-predictor targets (NF_TARGET_DENSEGAUSS, NF_TARGET_LOGREG): the constants, the argument
conventions of nf_target_check as the C entry points report them BEFORE any device work (a stand-in context is enough),
the refusals for the flows whose kernels evaluate the target one feature at a time, the new kernels' resources, and the
host-side constructors."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from __graft_entry__ import ROOT, build, load_package


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def test_constants_match_the_header(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = dict(re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M))
    assert int(defs["NF_TARGET_DENSEGAUSS"]) == nf._lib.NF_TARGET_DENSEGAUSS == 5
    assert int(defs["NF_TARGET_LOGREG"]) == nf._lib.NF_TARGET_LOGREG == 6
    for name, v in defs.items():
        assert getattr(nf._lib, name) == int(v)


def test_target_logp_argument_errors_come_before_device_work(nf):
    """nf_target_logp answers NF_ERR_ARG (-1) for every violated argument convention of the two kinds without touching
    the context: a zeroed stand-in is enough."""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=3, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, 4, C.c_void_p(p), C.c_void_p(p), None)

    for dtype in (0, 1):
        assert logp(Target(5, p, 0, 0.0, 0.0), dtype=dtype) == -1      # DENSEGAUSS: p1 = NULL
        assert logp(Target(5, 0, p, 0.0, 0.0), dtype=dtype) == -1      # DENSEGAUSS: p0 = NULL
        assert logp(Target(6, 0, 0, 8.0, 1.0), dtype=dtype) == -1      # LOGREG: p1 = NULL
        assert logp(Target(6, 0, p, 0.0, 1.0), dtype=dtype) == -1      # s0 = 0 rows
        assert logp(Target(6, 0, p, 2.5, 1.0), dtype=dtype) == -1      # s0 not integral
        assert logp(Target(6, 0, p, -3.0, 1.0), dtype=dtype) == -1
        assert logp(Target(6, 0, p, 2147483648.0, 1.0), dtype=dtype) == -1
        assert logp(Target(6, 0, p, 8.0, 0.0), dtype=dtype) == -1      # prior sigma = 0
        assert logp(Target(6, 0, p, 8.0, -1.0), dtype=dtype) == -1
        assert logp(Target(7, p, p, 8.0, 1.0), dtype=dtype) == -1      # no such kind


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """Planar, radial, mean-field and Hamiltonian flows answer NF_ERR_UNSUPPORTED (-2) to the ELBO entry points with a
    linear-predictor target, and a Hamiltonian descriptor cannot take one as its score -- all before the context is used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1)):
        desc = FlowDesc()
        desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
        for tk in (5, 6):
            tgt = Target(tk, p.value, p.value, 4.0, 1.0)
            assert lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p) == -2
            assert lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)) == -2
            assert lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)) == -2
            assert lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None) == -2
            assert lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None) == -2
    score = Target(5, p.value, p.value, 0.0, 0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    hd = FlowDesc()
    hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
    hd.score = C.cast(C.pointer(score), C.c_void_p)
    assert lib.nf_elbo_value_and_grad(ctx, C.byref(hd), C.byref(diag), p, p, 8, 8, 1, 0, 0, p) == -2
    hd.score = C.cast(C.pointer(diag), C.c_void_p)  # a supported score, a linear-predictor ELBO target
    assert lib.nf_elbo_value_and_grad(ctx, C.byref(hd), C.byref(score), p, p, 8, 8, 1, 0, 0, p) == -2


def test_linpred_kernels_are_built_register_resident(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = [r for r in kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build")) if "k_target_linpred" in r[0]]
    tiled = [r for r in rows if "k_target_linpred_tiled<" in r[0]]
    flat = [r for r in rows if "k_target_linpred<" in r[0]]
    assert len(tiled) == 8 and len(flat) == 4, [r[0][:60] for r in rows]  # DB in {1, 2, 4, 8} x phi; {float, double} x phi
    for name, agpr, vgpr, sgpr, scratch, lds in rows:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole file


def test_mvnormal_target_factorisation(nf):
    g = torch.Generator().manual_seed(3)
    d = 7
    Q, _ = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))
    lam = 0.5 + 1.5 * torch.rand(d, generator=g, dtype=torch.float64)
    Sigma = (Q * lam) @ Q.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    mu = torch.randn(d, generator=g, dtype=torch.float64)
    t = nf.MvNormalTarget(mu, Sigma)
    Wi = torch.linalg.inv(t.W)
    assert float((Wi @ Wi.T - Sigma).abs().max()) <= 1e-12
    assert float(torch.triu(t.W, 1).abs().max()) == 0.0  # lower triangular, stored dense with its zeros
    assert abs(t.c.s0 - (-0.5 * float(torch.logdet(Sigma)))) <= 1e-12
    assert t.c.kind == 5 and t.c.p0 == t.mu.data_ptr() and t.c.p1 == t.W.data_ptr()
    t32 = nf.MvNormalTarget(mu.float(), Sigma.float())
    assert t32.W.dtype == torch.float32 and t32.mu.dtype == torch.float32


def test_constructors_refuse_bad_arguments(nf):
    E = nf.NFHipError
    mu = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(E):
        nf.MvNormalTarget(mu, torch.tensor([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64))  # indefinite
    with pytest.raises(E):
        nf.MvNormalTarget(mu, torch.tensor([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64))  # not symmetric
    with pytest.raises(E):
        nf.MvNormalTarget(mu, torch.eye(3, dtype=torch.float32))  # element types differ
    with pytest.raises(E):
        nf.MvNormalTarget(mu, torch.eye(4, dtype=torch.float64))  # dimensions differ
    X = torch.randn(5, 3, generator=torch.Generator().manual_seed(0))
    with pytest.raises(E):
        nf.LogisticRegressionTarget(X, torch.tensor([0, 1, 2, 0, 1]))
    with pytest.raises(E):
        nf.LogisticRegressionTarget(X, torch.tensor([-1, 1, 0, 1, 1]))  # a mixture of the two label sets
    with pytest.raises(E):
        nf.LogisticRegressionTarget(X, torch.tensor([1, 1, 0, 1]))
    for bad in (0.0, -1.0):
        with pytest.raises(E):
            nf.LogisticRegressionTarget(X, torch.tensor([1, 1, 0, 1, 0]), prior_sigma=bad)
    with pytest.raises(E):
        nf.LogisticRegressionTarget(X, torch.tensor([1, 1, 0, 1, 0]), shift=torch.zeros(3, dtype=torch.float64))
    t = nf.LogisticRegressionTarget(X, torch.tensor([1, 1, 0, 1, 0]), prior_sigma=2.0)
    sign = torch.tensor([1.0, 1.0, -1.0, 1.0, -1.0])
    assert torch.equal(t.A, X * sign[:, None]) and t.c.kind == 6 and t.c.s0 == 5.0 and t.c.s1 == 2.0 and not t.c.p0
    assert torch.equal(nf.LogisticRegressionTarget(X, sign).A, t.A)


def test_check_compatible_refuses_type_device_and_dimension_mismatch(nf):
    E = nf.NFHipError
    from normalizingflows_jl_amd.flows import check_target

    tg = nf.MvNormalTarget(torch.zeros(3), torch.eye(3))
    tl = nf.LogisticRegressionTarget(torch.ones(4, 3), torch.tensor([1, -1, 1, 1]))
    for t in (tg, tl):
        check_target(t, torch.float32, "cpu", 3)
        with pytest.raises(E):
            check_target(t, torch.float64, "cpu", 3)
        with pytest.raises(E):
            check_target(t, torch.float32, "cuda:0", 3)
        with pytest.raises(E):
            check_target(t, torch.float32, "cpu", 4)


def test_builtin_routing_sends_simple_flows_to_the_closure_branch(nf):
    from normalizingflows_jl_amd import objectives as ob

    assert nf.MvNormalTarget in ob._BUILTIN and nf.LogisticRegressionTarget in ob._BUILTIN

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d):
            self.kind, self.theta = kind, torch.zeros(1)
            self.dist = type("D", (), {"d": d})()

    tg = nf.MvNormalTarget(torch.zeros(3), torch.eye(3))
    for kind in ("planar", "radial", "meanfield"):
        assert ob._builtin(F(kind, 3), tg) is False
    assert ob._builtin(F("hamiltonian", 6), tg) is False
    for kind in ("realnvp", "nsf", "composite"):
        assert ob._builtin(F(kind, 3), tg) is True
    with pytest.raises(nf.NFHipError):
        ob._builtin(F("planar", 4), tg)  # the mismatch is reported on either route
