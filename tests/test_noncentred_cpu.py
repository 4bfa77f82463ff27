"""CPU checks of the non-centred flow (NF_KIND_NONCENTRED: the non-centring layer of the hierarchical targets over a RealNVP, NSF
or full-rank flow): the numpy reference tests/noncentred_ref.py against central differences (the oracle has no such kind), the
library's host side with a stand-in context (every refusal below comes before any device work), the Python mirror and the new
kernels' resources -- no GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import nf_oracle as o
import noncentred_cases as nc
import noncentred_ref as ncr
import parity as P
from __graft_entry__ import build, load_package
from test_fullrank_cpu import _elbo_entry_points, _standin
from test_precond_cpu import _inner, _precond

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF_ERR_ARG, NF_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def _fd_spec(shape, kind, frozen):
    form, p, G = nc.SHAPES[shape]
    d = nc.dim(shape)
    inner = {"realnvp": o.FlowSpec("realnvp", d, 1, (8, 8)), "nsf": o.FlowSpec("nsf", d, 1, (8, 8), 4, 30.0),
             "fullrank": ncr.fullrank_spec(d)}[kind]
    return ncr.Spec(inner, ncr.groups(p, G), G, frozen)


@pytest.mark.parametrize("frozen", [False, True], ids=["trained", "frozen"])
@pytest.mark.parametrize("shape", ["small", "disp"])
@pytest.mark.parametrize("kind", ["realnvp", "nsf", "fullrank"])
def test_reference_gradient_against_central_differences(nf, kind, shape, frozen):
    import torch

    spec = _fd_spec(shape, kind, frozen)
    n = 6
    theta, x = ncr.inputs(spec, n, True)
    rng = np.random.default_rng(3)
    theta = theta + np.concatenate([np.zeros(spec.p), 0.05 * rng.standard_normal(ncr.inner_params(spec.inner))])
    if kind == "fullrank":  # the reference keeps zeros above the diagonal: differentiate what it reads
        import fullrank_cases as fc

        theta = np.concatenate([theta[:spec.p], fc.zero_upper(theta[spec.p:], spec.d)])
        skip = np.concatenate([np.zeros(spec.p, dtype=bool), fc.upper_mask(spec.d)])
    else:
        skip = np.zeros(theta.size, dtype=bool)
    _, ref = nc.make_target(nf, shape, torch.float64, "cpu")
    _, g = ncr.neg_elbo_value_and_grad(spec, theta, x, ref)
    fixed = ncr.fixed_mask(spec)
    fd = np.zeros_like(theta)
    h = 1e-6
    for q in np.flatnonzero(~skip):
        if frozen and q < spec.p:
            continue
        tp, tm = theta.copy(), theta.copy()
        tp[q] += h
        tm[q] -= h
        fd[q] = (ncr.neg_elbo_value_and_grad(spec, tp, x, ref)[0] - ncr.neg_elbo_value_and_grad(spec, tm, x, ref)[0]) / (2 * h)
    key = f"noncentred reference {kind} {shape} {'frozen' if frozen else 'trained'}: gradient vs central differences"
    err = P.gradient(key, g, fd, 1e-6)
    print(f"{key} {err:.2e}")
    assert (g[fixed] == 0.0).all() and np.abs(fd[fixed]).max() == 0.0  # a coefficient without a group: lam is not read
    if frozen:
        assert (g[:spec.p] == 0.0).all()
    else:
        assert np.abs(g[:spec.p][~fixed[:spec.p]]).min() > 0.0


@pytest.mark.parametrize("shape", ["small", "disp", "nogroup"])
def test_reference_pullback_inverse_and_layers(shape):
    spec = nc.spec_of(shape, "realnvp")
    d, n = spec.d, 6
    theta, x = ncr.inputs(spec, n, True, nan_fixed=True)  # NaN where lam is never read
    rng = np.random.default_rng(1)
    ybar, lbar = rng.standard_normal((d, n)), rng.standard_normal(n)

    def f(xx):
        y, ladj = ncr.fwd(spec, theta, xx)
        return (ybar * y).sum() + (lbar * ladj).sum()

    y, ladj, tape = ncr.fwd(spec, theta, x, keep=True)
    xbar, g = ncr.bwd(spec, theta, tape, ybar, lbar)
    assert np.isfinite(y).all() and np.isfinite(g).all() and (g[ncr.fixed_mask(spec)] == 0.0).all()
    h = 1e-6
    for (i, j) in ((0, 0), (d - 2, 3), (d - 1, 5)):
        xp, xm = x.copy(), x.copy()
        xp[i, j] += h
        xm[i, j] -= h
        assert abs((f(xp) - f(xm)) / (2 * h) - xbar[i, j]) <= 1e-6 * max(1.0, abs(xbar[i, j]))
    xr, li = ncr.inv(spec, theta, y)
    assert np.abs(xr - x).max() <= 1e-9 and np.abs(li + ladj).max() <= 1e-9
    # layer by layer: the inner flow's layers (the last-listed first), then S, the last layer
    u, l = x, np.zeros(n)
    for i in list(range(ncr.layer_count(spec) - 2, -1, -1)) + [ncr.layer_count(spec) - 1]:
        u, li_ = ncr.layer(spec, theta, i, u)
        l = l + li_
    assert np.abs(u - y).max() <= 1e-12 and np.abs(l - ladj).max() <= 1e-12
    # ladj is the log-determinant of S's Jacobian
    lam, ti = ncr.split(spec, theta)
    z = x[:, :1]
    J = np.zeros((d, d))
    for k in range(d):
        zp, zm = z.copy(), z.copy()
        zp[k] += h
        zm[k] -= h
        J[:, k] = ((ncr.s_fwd(spec, lam, zp)[0] - ncr.s_fwd(spec, lam, zm)[0]) / (2 * h))[:, 0]
    assert abs(np.linalg.slogdet(J)[1] - ncr.s_fwd(spec, lam, z)[1][0]) <= 1e-7


def test_lam_zero_is_the_inner_flow():
    for kind in ("realnvp", "fullrank"):
        spec = nc.spec_of("small", kind)
        theta, x = ncr.inputs(spec, 7, True, lam=0.0)
        y, ladj = ncr.fwd(spec, theta, x)
        y0, l0, _ = ncr.inner_fwd(spec.inner, theta[spec.p:], x)
        assert np.array_equal(y, y0) and np.array_equal(ladj, l0)


# ---- host side of the library ------------------------------------------------------------------------------------------------------
def _target(kind=16, d=5, G=2, rows=4.0):
    """(nf_target, keep-alive): host fields only -- nothing dereferences the buffers before the device is set"""
    from normalizingflows_jl_amd._lib import Target

    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    tgt = Target(kind, p.value, p.value, rows, float(G))
    tgt._keep = buf
    return tgt, buf


def _noncentred(nf, inner, tgt, d=None, dtype=None, nsegments=1, K=0):
    """(descriptor, keep-alive)"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    segs = (FlowDesc * max(nsegments, 1))()
    for i in range(max(nsegments, 1)):
        C.memmove(C.addressof(segs[i]), C.addressof(inner), C.sizeof(FlowDesc))
    desc = FlowDesc()
    desc.kind, desc.nlayers, desc.nsegments, desc.K = NF_KIND["noncentred"], 1, nsegments, K
    desc.d = inner.d if d is None else d
    desc.dtype = inner.dtype if dtype is None else dtype
    desc.segments = C.cast(segs, C.c_void_p)
    desc.score = C.addressof(tgt) if tgt is not None else None
    desc._keep = (segs, tgt)  # the descriptor holds plain addresses
    return desc, segs


def test_kind_constant_abi_and_symbols_are_unchanged(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = dict(re.findall(r"^#define (NF_KIND_\w+) (\d+)", hdr, re.M))
    assert int(defs["NF_KIND_NONCENTRED"]) == nf._lib.NF_KIND["noncentred"] == 10
    assert 9 not in nf._lib.NF_KIND.values() and "9" not in defs.values()
    assert nf.load_library().nf_abi_version() == 4 and int(re.search(r"#define NF_ABI_VERSION (\d+)", hdr).group(1)) == 4
    declared = set(re.findall(r"\b(nf_[a-z0-9_]+)\s*\(", hdr))
    assert set(nf.SYMBOLS) <= declared and len(nf.SYMBOLS) == 49


def test_counts_agree_with_the_reference(nf):
    lib = nf.load_library()
    ctx, keep = _standin()
    for dtype in (0, 1):
        for shape, kind, hd in (("small", "realnvp", (32, 32)), ("disp", "nsf", (32, 32)), ("wide", "realnvp", (32, 32)),
                                ("pair", "realnvp", (64, 64)), ("wide", "fullrank", ()), ("nogroup", "realnvp", (32, 32))):
            form, p, G = nc.SHAPES[shape]
            d = nc.dim(shape)
            inner = _inner(nf, kind, d, dtype, hd, 1)
            tgt, tk = _target(29 if form == "disp" else 16, d, G)
            desc, segs = _noncentred(nf, inner, tgt)
            g = ncr.fullrank_spec(d) if kind == "fullrank" else o.FlowSpec(kind, d, 1, hd, 8 if kind == "nsf" else 0, 30.0 if kind == "nsf" else 0.0)
            spec = ncr.Spec(g, ncr.groups(p, G), G)
            assert int(lib.nf_param_count(C.byref(desc))) == ncr.param_count(spec) == p + int(lib.nf_param_count(C.byref(inner)))
            assert int(lib.nf_layer_count(C.byref(desc))) == ncr.layer_count(spec) == 1 + int(lib.nf_layer_count(C.byref(inner)))
            # the tape holds S's input next to the inner flow's own tape
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

    tgt, tk = _target(16, 5, 2)
    for dtype in (0, 1):
        ok = _inner(nf, "realnvp", 5, dtype)
        for kind in ("realnvp", "nsf", "fullrank"):
            for K in (0, 1):
                assert int(lib.nf_tape_bytes(ctx, C.byref(_noncentred(nf, _inner(nf, kind, 5, dtype), tgt, K=K)[0]), 10)) > 0, kind
        for K in (-1, 2, 8):
            assert code(_noncentred(nf, ok, tgt, K=K)[0]) == NF_ERR_ARG, K
        # the segment count, NULL segments, NULL score
        assert code(_noncentred(nf, ok, tgt, nsegments=2)[0]) == NF_ERR_ARG
        assert code(_noncentred(nf, ok, tgt, nsegments=0)[0]) == NF_ERR_ARG
        none = _noncentred(nf, ok, tgt)[0]
        none.segments = None
        assert code(none) == NF_ERR_ARG
        assert code(_noncentred(nf, ok, None)[0]) == NF_ERR_ARG
        # inner kinds other than RealNVP / NSF / full-rank
        for kind in ("planar", "radial", "meanfield"):
            assert code(_noncentred(nf, _inner(nf, kind, 5, dtype, nlayers=2), tgt)[0]) == NF_ERR_ARG, kind
        comp = FlowDesc()
        comp.kind, comp.dtype, comp.d, comp.nlayers, comp.nsegments = NF_KIND["composite"], dtype, 5, 1, 1
        seg = (FlowDesc * 1)()
        C.memmove(C.addressof(seg[0]), C.addressof(ok), C.sizeof(FlowDesc))
        comp.segments = C.cast(seg, C.c_void_p)
        assert code(_noncentred(nf, comp, tgt)[0]) == NF_ERR_ARG
        nested, keep2 = _noncentred(nf, ok, tgt)
        assert code(_noncentred(nf, nested, tgt)[0]) == NF_ERR_ARG
        pre, keep3 = _precond(nf, ok)
        assert code(_noncentred(nf, pre, tgt)[0]) == NF_ERR_ARG
        # the inner flow's d, dtype, base
        assert code(_noncentred(nf, ok, tgt, d=6)[0]) == NF_ERR_ARG
        assert code(_noncentred(nf, ok, tgt, dtype=1 - dtype)[0]) == NF_ERR_ARG
        based = _inner(nf, "realnvp", 5, dtype)
        base = Base(1, p.value, p.value, 0.0)
        based.base = C.addressof(base)
        assert code(_noncentred(nf, based, tgt)[0]) == NF_ERR_ARG
        # score kinds outside 16..20 and 29..31
        for k in (0, 2, 5, 6, 8, 9, 13, 14, 15, 21, 22, 26, 27, 28, 32):
            assert code(_noncentred(nf, ok, _target(k, 5, 2)[0])[0]) == NF_ERR_ARG, k
        for k in (16, 17, 18, 19, 20, 29, 30, 31):
            assert int(lib.nf_tape_bytes(ctx, C.byref(_noncentred(nf, ok, _target(k, 5, 2)[0])[0]), 10)) > 0, k
        # a score that fails its own check at this d: G beyond d - 1 (d - 2 for the dispersion form), a fractional G, no rows, no buffer
        for bad in (_target(16, 5, 5), _target(29, 5, 4), _target(16, 5, 1.5), _target(16, 5, 2, rows=0.0), _target(16, 5, -1)):
            assert code(_noncentred(nf, ok, bad[0])[0]) == NF_ERR_ARG
        nobuf, tk2 = _target(16, 5, 2)
        nobuf.p0 = None
        assert code(_noncentred(nf, ok, nobuf)[0]) == NF_ERR_ARG
        assert int(lib.nf_tape_bytes(ctx, C.byref(_noncentred(nf, ok, _target(16, 5, 4)[0])[0]), 10)) > 0  # G = d - 1: p = 1
        # what the inner flow refuses
        assert code(_noncentred(nf, _inner(nf, "fullrank", 257, dtype), _target(16, 257, 2)[0])[0]) == NF_ERR_UNSUPPORTED
        assert code(_noncentred(nf, _inner(nf, "realnvp", 257, dtype), _target(16, 257, 2)[0])[0]) == NF_ERR_UNSUPPORTED
        # kind 9 stays unassigned
        nine = _inner(nf, "realnvp", 5, dtype)
        nine.kind = 9
        assert code(nine) == NF_ERR_ARG
        nine2 = _noncentred(nf, ok, tgt)[0]
        nine2.kind = 9
        assert code(nine2) == NF_ERR_ARG
        # a non-centred flow is no segment of a composition, in either position, and no inner flow of a preconditioned one
        ncd, keep4 = _noncentred(nf, ok, tgt)
        for order in ((ncd, _inner(nf, "planar", 5, dtype, nlayers=2)), (_inner(nf, "planar", 5, dtype, nlayers=2), ncd)):
            segs = (FlowDesc * 2)()
            for g, src in zip(segs, order):
                C.memmove(C.addressof(g), C.addressof(src), C.sizeof(FlowDesc))
            comp2 = FlowDesc()
            comp2.kind, comp2.dtype, comp2.d, comp2.nlayers, comp2.nsegments = NF_KIND["composite"], dtype, 5, 1, 2
            comp2.segments = C.cast(segs, C.c_void_p)
            assert code(comp2) == NF_ERR_ARG
        pre2, keep6 = _precond(nf, ncd)
        assert code(pre2) == NF_ERR_ARG
        # the layer's own descriptor (no segments) exists only inside the library
        alone, keep5 = _noncentred(nf, ok, tgt, nsegments=0)
        alone.segments = None
        assert code(alone) == NF_ERR_ARG


def test_refusals_come_before_device_work(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    score, tk = _target(16, 5, 2)
    score32, tk32 = _target(30, 32, 3)
    for dtype in (0, 1):
        for inner, tgt in ((_inner(nf, "realnvp", 5, dtype), score), (_inner(nf, "nsf", 32, dtype), score32), (_inner(nf, "fullrank", 5, dtype), score)):
            desc, segs = _noncentred(nf, inner, tgt)
            assert lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(diag), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
            assert lib.nf_loglikelihood_value_and_grad(ctx, C.byref(desc), p, p, 8, 8, p) == NF_ERR_UNSUPPORTED
            assert lib.nf_loglikelihood_step(ctx, C.byref(desc), p, p, p, p, 8, 8, 0, 1e-3, 0.9, 0.999, 1e-8, None, None) == NF_ERR_UNSUPPORTED
            assert lib.nf_loglikelihood_step_enqueue(ctx, C.byref(desc), p, p, p, p, 8, 8, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
            # served: these pass every check and stop at the stand-in context's device ordinal -- with the layer's own target and
            # with any other the inner flow is served with
            assert lib.nf_loglikelihood(ctx, C.byref(desc), p, p, 8, None, C.byref(val)) > 0
            assert all(c > 0 for c in _elbo_entry_points(lib, ctx, desc, diag, p, val))
            assert all(c > 0 for c in _elbo_entry_points(lib, ctx, desc, tgt, p, val))
            assert lib.nf_flow_inv(ctx, C.byref(desc), p, p, 8, p, p) > 0
            assert lib.nf_flow_rand(ctx, C.byref(desc), p, 8, 1, 0, 0, p) > 0
            nl = int(lib.nf_layer_count(C.byref(desc)))
            assert lib.nf_layer_apply(ctx, C.byref(desc), nl - 1, 0, p, p, 8, p, p) > 0
            assert lib.nf_layer_apply(ctx, C.byref(desc), nl, 0, p, p, 8, p, p) == NF_ERR_ARG


def test_targets_are_refused_as_for_the_inner_flow(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    mix = Target(8, p.value, p.value, 3.0, 0.0)
    score, tk = _target(16, 70, 10)
    wide32, wide64 = _inner(nf, "realnvp", 70, 0), _inner(nf, "realnvp", 70, 1)
    assert _elbo_entry_points(lib, ctx, _noncentred(nf, wide32, score)[0], mix, p, val) == [NF_ERR_UNSUPPORTED] * 4
    assert _elbo_entry_points(lib, ctx, _noncentred(nf, _inner(nf, "fullrank", 70, 0), score)[0], mix, p, val) == [NF_ERR_UNSUPPORTED] * 4
    assert all(c > 0 for c in _elbo_entry_points(lib, ctx, _noncentred(nf, wide64, score)[0], mix, p, val))


# ---- the Python mirror -------------------------------------------------------------------------------------------------------------
def test_python_mirror_on_the_cpu(nf):
    import torch

    from normalizingflows_jl_amd.objectives import _builtin

    for dt in (torch.float32, torch.float64):
        for shape in ("small", "disp"):
            form, p, G = nc.SHAPES[shape]
            d = nc.dim(shape)
            tgt, _ = nc.make_target(nf, shape, dt, "cpu")
            rn = nf.realnvp(nf.MvNormal(d), [8, 8], 1, paramtype=dt, device="cpu")
            flow = nf.noncentred(rn, tgt)
            assert flow.kind == "noncentred" and flow.P == p + rn.P and flow.theta.dtype == dt and flow.score is tgt
            assert flow.desc.kind == 10 and flow.desc.K == 0 and flow.desc.nsegments == 1 and flow.desc.score == C.addressof(tgt.c)
            assert (flow.lam == 1).all() and torch.equal(flow.inner.theta, rn.theta)
            # lam and inner are views of theta
            flow.theta[0] = 3.0
            flow.theta[p] = -2.0
            assert flow.lam[0] == 3.0 and flow.inner.theta[0] == -2.0 and flow.inner.kind == "realnvp"
            # lam= as a vector, learn=False
            lam = torch.arange(p, dtype=dt) * 0.25
            f2 = nf.noncentred(rn, tgt, lam=lam, learn=False)
            assert torch.equal(f2.lam, lam) and f2.desc.K == 1
            assert (nf.noncentred(rn, tgt, lam=0.0).lam == 0).all()
            # with_theta / destructure keep the family, the target and the frozen flag
            theta, re_ = f2.destructure()
            f3 = re_(theta * 2)
            assert f3.kind == "noncentred" and f3.P == f2.P and f3.desc.K == 1 and f3.score is tgt and torch.equal(f3.lam, lam * 2)
            # every inner family
            for inner in (nf.nsf(nf.MvNormal(d), [8, 8], 4, 30.0, 1, paramtype=dt, device="cpu"), nf.fullrank(nf.MvNormal(d), paramtype=dt, device="cpu")):
                assert nf.noncentred(inner, tgt).P == p + inner.P
            # _builtin answers as for the inner flow
            diag = nf.DiagGaussTarget(torch.zeros(d, dtype=dt), torch.ones(d, dtype=dt))
            for t in (tgt, diag):
                assert _builtin(flow, t) is _builtin(rn, t) is True
            assert _builtin(flow, lambda y: y.sum(0)) is False
            # what the constructor refuses
            pl = nf.planarflow(nf.MvNormal(d), 2, paramtype=dt, device="cpu")
            for bad in (pl, flow, nf.preconditioned(rn), nf.create_flow([rn, pl], nf.MvNormal(d)), None):
                with pytest.raises(nf.NFHipError):
                    nf.noncentred(bad, tgt)
            for bad in (diag, nf.GLMTarget("logit", torch.ones(3, d, dtype=dt)), None):
                with pytest.raises(nf.NFHipError):
                    nf.noncentred(rn, bad)
            with pytest.raises(nf.NFHipError):
                nf.noncentred(rn, tgt, lam=torch.zeros(p + 1, dtype=dt))
            with pytest.raises(nf.NFHipError):  # the target's dimension
                nf.noncentred(nf.realnvp(nf.MvNormal(d + 1), [8, 8], 1, paramtype=dt, device="cpu"), tgt)
            other = torch.float64 if dt == torch.float32 else torch.float32
            with pytest.raises(nf.NFHipError):  # the target's element type
                nf.noncentred(nf.realnvp(nf.MvNormal(d), [8, 8], 1, paramtype=other, device="cpu"), tgt)
            # no membership in a composition, no preconditioning
            for order in ([flow, pl], [pl, flow]):
                with pytest.raises(nf.NFHipError):
                    nf.create_flow(order, nf.MvNormal(d))
            with pytest.raises(nf.NFHipError):
                nf.preconditioned(flow)


# ---- the new kernels are register-resident and fit the LDS ------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_fit_the_lds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    for prefix, count in (("void k_nc_fwd_tiled<", 2), ("void k_nc_bwd_tiled<", 8), ("void k_nc_apply_flat<", 4), ("void k_nc_pull_flat<", 4),
                          ("void k_nc_grad_flat<", 4)):
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        assert all(r[4] == 0 and r[5] == 0 for r in hit), [(r[0][:60], r[4], r[5]) for r in hit]
    # the dynamic LDS requests of the two tiled launchers at the widest p: below the 64 KiB no attribute is needed for
    assert 255 * 33 * 4 < 64 * 1024
