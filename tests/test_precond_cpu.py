"""CPU checks of the preconditioned coupling flow (NF_KIND_PRECOND: Shift o Scale(LowerTriangular) o couplings): the numpy
reference tests/precond_ref.py against central differences (the oracle has no such kind), the library's host side with a
stand-in context (every refusal below comes before any device work), the Python mirror and the new kernel's resources -- no
GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fullrank_cases as fc
import nf_oracle as o
import parity as P
import precond_ref as pr
from __graft_entry__ import build, load_package
from test_fullrank_cpu import _elbo_entry_points, _standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF_ERR_ARG, NF_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
FD_SPECS = [o.FlowSpec("realnvp", 5, 1, (8, 8)), o.FlowSpec("nsf", 5, 1, (8, 8), 4, 30.0)]


@pytest.mark.parametrize("spec", FD_SPECS, ids=lambda s: s.kind)
def test_reference_gradient_against_central_differences(spec):
    d, n = spec.d, 6
    theta, x = pr.inputs(spec, n, True, nan_upper=False)
    theta = theta + np.concatenate([np.zeros(pr.head(d)), 0.05 * np.random.default_rng(3).standard_normal(o.param_count(spec))])
    up = pr.upper_mask(spec)
    for name in ("diaggauss", "glm_poisson"):
        ref = fc.numpy_target(name, d, True)
        _, g = pr.neg_elbo_value_and_grad(spec, theta, x, ref)
        fd = np.zeros_like(theta)
        h = 1e-6
        for p in np.flatnonzero(~up):
            tp, tm = theta.copy(), theta.copy()
            tp[p] += h
            tm[p] -= h
            fd[p] = (pr.neg_elbo_value_and_grad(spec, tp, x, ref)[0] - pr.neg_elbo_value_and_grad(spec, tm, x, ref)[0]) / (2 * h)
        err = P.gradient(f"precond reference {spec.kind} d={d} {name}: gradient vs central differences", g, fd, 1e-6)
        print(f"precond reference {spec.kind} d={d} {name}: gradient vs central differences {err:.2e}")
        assert (g[up] == 0.0).all()


@pytest.mark.parametrize("spec", FD_SPECS, ids=lambda s: s.kind)
def test_reference_pullback_and_inverse(spec):
    d, n = spec.d, 6
    theta, x = pr.inputs(spec, n, True)  # NaN above the diagonal: never read
    rng = np.random.default_rng(1)
    ybar, lbar = rng.standard_normal((d, n)), rng.standard_normal(n)

    def f(xx):
        y, ladj = pr.fwd(spec, theta, xx)
        return (ybar * y).sum() + (lbar * ladj).sum()

    y, ladj, tape = pr.fwd(spec, theta, x, keep=True)
    xbar, g = pr.bwd(spec, theta, tape, ybar, lbar)
    assert np.isfinite(y).all() and np.isfinite(g[~pr.upper_mask(spec)]).all()
    h = 1e-6
    for (i, j) in ((0, 0), (2, 3), (4, 5)):
        xp, xm = x.copy(), x.copy()
        xp[i, j] += h
        xm[i, j] -= h
        assert abs((f(xp) - f(xm)) / (2 * h) - xbar[i, j]) <= 1e-6 * max(1.0, abs(xbar[i, j]))
    xr, li = pr.inv(spec, theta, y)
    assert np.abs(xr - x).max() <= 1e-9 and np.abs(li + ladj).max() <= 1e-9
    # layer by layer: Scale after the couplings, then Shift
    u, l = x, np.zeros(n)
    for i in range(2 + 2 * spec.nlayers - 1, -1, -1):
        u, li_ = pr.layer(spec, theta, i, u)
        l = l + li_
    assert np.abs(u - y).max() <= 1e-12 and np.abs(l - ladj).max() <= 1e-12


def test_identity_preconditioner_is_the_inner_flow():
    spec = FD_SPECS[0]
    d, n = spec.d, 7
    ti = o.init_params(spec, np.random.default_rng(7))
    x = np.random.default_rng(2).standard_normal((d, n))
    theta = np.concatenate([np.zeros(d), np.eye(d).reshape(-1), ti])
    y, ladj = pr.fwd(spec, theta, x)
    y0, l0 = o.flow_fwd(spec, ti, x)
    assert np.array_equal(y, y0) and np.array_equal(ladj, l0)


# ---- host side of the library ------------------------------------------------------------------------------------------------------
def _inner(nf, kind, d, dtype=0, hdims=(32, 32), nlayers=1, K=8):
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    g = FlowDesc()
    g.kind, g.dtype, g.d, g.nlayers = NF_KIND[kind], dtype, d, nlayers
    if kind in ("realnvp", "nsf"):
        g.n_hidden = len(hdims)
        for i, h in enumerate(hdims):
            g.hdims[i] = h
    if kind == "nsf":
        g.K, g.B = K, 30.0
    return g


def _precond(nf, inner, d=None, dtype=None, nsegments=1, nlayers=1):
    """(descriptor, keep-alive)"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    segs = (FlowDesc * max(nsegments, 1))()
    for i in range(max(nsegments, 1)):
        C.memmove(C.addressof(segs[i]), C.addressof(inner), C.sizeof(FlowDesc))
    desc = FlowDesc()
    desc.kind, desc.nlayers, desc.nsegments = NF_KIND["preconditioned"], nlayers, nsegments
    desc.d = inner.d if d is None else d
    desc.dtype = inner.dtype if dtype is None else dtype
    desc.segments = C.cast(segs, C.c_void_p)
    return desc, segs


def test_kind_constant_matches_the_header(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = dict(re.findall(r"^#define (NF_KIND_\w+) (\d+)", hdr, re.M))
    assert int(defs["NF_KIND_PRECOND"]) == nf._lib.NF_KIND["preconditioned"] == 8


def test_counts_and_layout(nf):
    lib = nf.load_library()
    ctx, keep = _standin()
    for dtype in (0, 1):
        for kind, d, hd, nl in (("realnvp", 5, (32, 32), 2), ("nsf", 32, (32, 32), 1), ("realnvp", 70, (32, 32), 1),
                                ("realnvp", 256, (128, 100), 1), ("nsf", 6, (64, 64), 1)):
            inner = _inner(nf, kind, d, dtype, hd, nl)
            desc, segs = _precond(nf, inner)
            p_in, l_in = int(lib.nf_param_count(C.byref(inner))), int(lib.nf_layer_count(C.byref(inner)))
            assert p_in == o.param_count(o.FlowSpec(kind, d, nl, hd, 8 if kind == "nsf" else 0, 30.0 if kind == "nsf" else 0.0))
            assert int(lib.nf_param_count(C.byref(desc))) == d + d * d + p_in
            assert int(lib.nf_layer_count(C.byref(desc))) == 2 + l_in == 2 + 2 * nl
            # the tape holds the full-rank layer's input next to the couplings' own tape
            assert int(lib.nf_tape_bytes(ctx, C.byref(desc), 100)) >= int(lib.nf_tape_bytes(ctx, C.byref(inner), 100)) + 100 * d * (8 if dtype else 4)
            assert int(lib.nf_workspace_bytes(ctx, C.byref(desc), 100)) > int(lib.nf_workspace_bytes(ctx, C.byref(inner), 100)) > 0
            assert int(lib.nf_comm_bucket_count(ctx, C.byref(desc))) == 0  # one message, whatever the inner flow


def test_check_desc_outcomes(nf):
    from normalizingflows_jl_amd._lib import NF_KIND, Base, FlowDesc

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def code(desc):
        a, b = int(lib.nf_tape_bytes(ctx, C.byref(desc), 10)), lib.nf_flow_fwd(ctx, C.byref(desc), p, p, 8, p, p)
        c = int(lib.nf_workspace_bytes(ctx, C.byref(desc), 10))
        assert a == b == c, (a, b, c)
        return a

    for dtype in (0, 1):
        ok = _inner(nf, "realnvp", 5, dtype)
        assert int(lib.nf_tape_bytes(ctx, C.byref(_precond(nf, ok)[0]), 10)) > 0
        # inner kinds other than the two coupling families
        for kind in ("planar", "radial", "meanfield", "fullrank"):
            assert code(_precond(nf, _inner(nf, kind, 5, dtype))[0]) == NF_ERR_ARG, kind
        comp = FlowDesc()
        comp.kind, comp.dtype, comp.d, comp.nlayers, comp.nsegments = NF_KIND["composite"], dtype, 5, 1, 1
        seg = (FlowDesc * 1)()
        C.memmove(C.addressof(seg[0]), C.addressof(ok), C.sizeof(FlowDesc))
        comp.segments = C.cast(seg, C.c_void_p)
        assert code(_precond(nf, comp)[0]) == NF_ERR_ARG
        nested, keep2 = _precond(nf, ok)
        assert code(_precond(nf, nested)[0]) == NF_ERR_ARG
        # mismatches, an inner base, the segment count, nlayers
        assert code(_precond(nf, ok, d=6)[0]) == NF_ERR_ARG
        assert code(_precond(nf, ok, dtype=1 - dtype)[0]) == NF_ERR_ARG
        based = _inner(nf, "realnvp", 5, dtype)
        base = Base(1, p.value, p.value, 0.0)
        based.base = C.addressof(base)
        assert code(_precond(nf, based)[0]) == NF_ERR_ARG
        assert code(_precond(nf, ok, nsegments=2)[0]) == NF_ERR_ARG
        assert code(_precond(nf, ok, nsegments=0)[0]) == NF_ERR_ARG
        assert code(_precond(nf, ok, nlayers=2)[0]) == NF_ERR_ARG
        none = _precond(nf, ok)[0]
        none.segments = None
        assert code(none) == NF_ERR_ARG
        # the envelope
        assert code(_precond(nf, _inner(nf, "realnvp", 257, dtype))[0]) == NF_ERR_UNSUPPORTED
        assert int(lib.nf_tape_bytes(ctx, C.byref(_precond(nf, _inner(nf, "realnvp", 256, dtype, (128, 100)))[0]), 10)) > 0
        # a preconditioned flow is no segment of a composition, in either position
        pre, keep3 = _precond(nf, ok)
        for order in ((pre, _inner(nf, "planar", 5, dtype, nlayers=2)), (_inner(nf, "planar", 5, dtype, nlayers=2), pre)):
            segs = (FlowDesc * 2)()
            for g, src in zip(segs, order):
                C.memmove(C.addressof(g), C.addressof(src), C.sizeof(FlowDesc))
            comp2 = FlowDesc()
            comp2.kind, comp2.dtype, comp2.d, comp2.nlayers, comp2.nsegments = NF_KIND["composite"], dtype, 5, 1, 2
            comp2.segments = C.cast(segs, C.c_void_p)
            assert code(comp2) == NF_ERR_ARG


def test_refusals_come_before_device_work(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    for dtype in (0, 1):
        for inner in (_inner(nf, "realnvp", 5, dtype), _inner(nf, "nsf", 32, dtype)):
            desc, segs = _precond(nf, inner)
            assert lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(diag), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
            assert lib.nf_loglikelihood_value_and_grad(ctx, C.byref(desc), p, p, 8, 8, p) == NF_ERR_UNSUPPORTED
            assert lib.nf_loglikelihood_step(ctx, C.byref(desc), p, p, p, p, 8, 8, 0, 1e-3, 0.9, 0.999, 1e-8, None, None) == NF_ERR_UNSUPPORTED
            assert lib.nf_loglikelihood_step_enqueue(ctx, C.byref(desc), p, p, p, p, 8, 8, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
            # served: these pass every check and stop at the stand-in context's device ordinal
            assert lib.nf_loglikelihood(ctx, C.byref(desc), p, p, 8, None, C.byref(val)) > 0
            assert all(c > 0 for c in _elbo_entry_points(lib, ctx, desc, diag, p, val))
            assert lib.nf_flow_inv(ctx, C.byref(desc), p, p, 8, p, p) > 0
            assert lib.nf_layer_apply(ctx, C.byref(desc), 2, 0, p, p, 8, p, p) > 0
            assert lib.nf_layer_apply(ctx, C.byref(desc), 4, 0, p, p, 8, p, p) == NF_ERR_ARG  # 2 + 2 layers


def test_targets_are_refused_as_for_the_inner_flow(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    mix = Target(8, p.value, p.value, 3.0, 0.0)
    kinds = [0, 1, 2, 5, 6, 8, 9, 10, 11, 12, 13]
    for dtype in (0, 1):
        for k in kinds:  # every target the inner flow is served with, at d = 5
            tgt = Target(k, p.value, p.value, 4.0, 0.0 if k == 8 else 1.0)
            inner = _inner(nf, "realnvp", 5, dtype)
            a = _elbo_entry_points(lib, ctx, inner, tgt, p, val)
            b = _elbo_entry_points(lib, ctx, _precond(nf, inner)[0], tgt, p, val)
            assert [c > 0 for c in a] == [c > 0 for c in b] and all(c > 0 for c in b), (dtype, k, a, b)
    # the mixture beyond the tiled kernel's d = 64: refused in Float32 on the matrix-pipe path, served in Float64 and at d = 64
    wide32, wide64 = _inner(nf, "realnvp", 70, 0), _inner(nf, "realnvp", 70, 1)
    assert _elbo_entry_points(lib, ctx, wide32, mix, p, val) == [NF_ERR_UNSUPPORTED] * 4
    assert _elbo_entry_points(lib, ctx, _precond(nf, wide32)[0], mix, p, val) == [NF_ERR_UNSUPPORTED] * 4
    assert all(c > 0 for c in _elbo_entry_points(lib, ctx, _precond(nf, wide64)[0], mix, p, val))
    assert all(c > 0 for c in _elbo_entry_points(lib, ctx, _precond(nf, _inner(nf, "realnvp", 64, 0, (64, 64)))[0], mix, p, val))


# ---- the Python mirror -------------------------------------------------------------------------------------------------------------
def test_python_mirror_on_the_cpu(nf):
    import torch

    from normalizingflows_jl_amd.objectives import _builtin

    d = 4
    for dt in (torch.float32, torch.float64):
        rn = nf.realnvp(nf.MvNormal(d), [8, 8], 1, paramtype=dt, device="cpu")
        flow = nf.preconditioned(rn)
        assert flow.kind == "preconditioned" and flow.P == d + d * d + rn.P and flow.theta.dtype == dt
        th = flow.theta.numpy()
        assert (th[:d] == 0).all() and (th[d:d + d * d].reshape(d, d) == np.eye(d)).all()
        assert (th[d + d * d:] == rn.theta.numpy()).all()
        # mu= / L=: column-major, the upper triangle kept as given
        Lm = torch.arange(1.0, d * d + 1, dtype=dt).reshape(d, d)
        f2 = nf.preconditioned(rn, mu=torch.arange(d, dtype=dt), L=Lm)
        t2 = f2.theta.numpy()
        assert (t2[:d] == np.arange(d)).all() and t2[d + 1] == Lm[1, 0] and t2[d + d] == Lm[0, 1]
        # init= copies a full-rank flow's bits, NaN above the diagonal included
        fr_flow = nf.fullrank(nf.MvNormal(d), paramtype=dt, device="cpu")
        t = fr_flow.theta.clone()
        t[:d] = torch.tensor([3.0, -2.0, 1.0, 0.5], dtype=dt)
        t[d + d] = float("nan")  # (row 0, column 1)
        fr_flow.theta = t
        f3 = nf.preconditioned(rn, init=fr_flow)
        assert f3.theta[: d + d * d].numpy().tobytes() == t.numpy().tobytes()
        assert (f3.theta[d + d * d:] == rn.theta).all()
        # with_theta / destructure keep the family
        theta, re = f3.destructure()
        f4 = re(theta * 2)
        assert f4.kind == "preconditioned" and f4.inner is rn and f4.P == f3.P and f4.desc.nsegments == 1
        # _builtin answers as for the inner flow
        mu, Sig = torch.zeros(d, dtype=dt), torch.eye(d, dtype=dt) * 2.0
        gauss = nf.MvNormalTarget(mu, Sig)
        glm = nf.GLMTarget("logit", torch.ones(3, d, dtype=dt))
        mix = nf.MixtureTarget(torch.tensor([0.5, 0.5], dtype=dt), torch.zeros(2, d, dtype=dt), torch.stack([Sig, Sig]))
        diag = nf.DiagGaussTarget(mu, torch.ones(d, dtype=dt))
        for tgt in (gauss, glm, mix, diag):
            assert _builtin(flow, tgt) is _builtin(rn, tgt) is True
        assert _builtin(flow, lambda y: y.sum(0)) is False
        # what the constructor refuses
        pl = nf.planarflow(nf.MvNormal(d), 2, paramtype=dt, device="cpu")
        for bad in (pl, fr_flow, flow, nf.create_flow([rn, pl], nf.MvNormal(d))):
            with pytest.raises(nf.NFHipError):
                nf.preconditioned(bad)
        with pytest.raises(nf.NFHipError):
            nf.preconditioned(rn, init=nf.fullrank(nf.MvNormal(d + 1), paramtype=dt, device="cpu"))
        other = torch.float64 if dt == torch.float32 else torch.float32
        with pytest.raises(nf.NFHipError):
            nf.preconditioned(rn, init=nf.fullrank(nf.MvNormal(d), paramtype=other, device="cpu"))
        with pytest.raises(nf.NFHipError):
            nf.preconditioned(rn, init=fr_flow, mu=torch.zeros(d, dtype=dt))
        with pytest.raises(nf.NFHipError):
            nf.preconditioned(rn, L=torch.eye(d + 1, dtype=dt))
        # no membership in a composition
        with pytest.raises(nf.NFHipError):
            nf.create_flow([flow, pl], nf.MvNormal(d))
        with pytest.raises(nf.NFHipError):
            nf.create_flow([pl, flow], nf.MvNormal(d))
    # Float32 beyond the tiled mixture kernel: the closure route, as for the inner flow; Float64 is served
    d = 70
    Sig = torch.eye(d)
    mix = nf.MixtureTarget(torch.tensor([0.5, 0.5]), torch.zeros(2, d), torch.stack([Sig, Sig]))
    assert _builtin(nf.preconditioned(nf.realnvp(nf.MvNormal(d), [32, 32], 1, paramtype=torch.float32, device="cpu")), mix) is False
    mix64 = nf.MixtureTarget(torch.tensor([0.5, 0.5], dtype=torch.float64), torch.zeros(2, d, dtype=torch.float64), torch.stack([Sig, Sig]).double())
    assert _builtin(nf.preconditioned(nf.realnvp(nf.MvNormal(d), [32, 32], 1, paramtype=torch.float64, device="cpu")), mix64) is True


# ---- the new kernel is register-resident and fits the LDS ----------------------------------------------------------------------
def test_new_kernel_uses_no_scratch_and_fits_the_lds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    hit = [r for r in rows if r[0].startswith("void k_fr_bwd_x<")]
    assert len(hit) == 4, [r[0][:60] for r in hit]
    assert all(r[4] == 0 for r in hit), [(r[0][:60], r[4]) for r in hit]
    # the dynamic LDS request of the launcher: two tiles and a matrix-block image per wave, at DB = 1, 2, 4, 8
    for db in (1, 2, 4, 8):
        assert (2 * 32 * db * 33 + 4 * 32 * 33) * 4 + 64 < 160 * 1024
    # the existing kernels are all still there, scratch-free
    for prefix, count in (("void k_fr_gemm<", 4), ("void k_fr_bwd<", 4)):
        old = [r for r in rows if r[0].startswith(prefix)]
        assert len(old) == count and all(r[4] == 0 for r in old)
