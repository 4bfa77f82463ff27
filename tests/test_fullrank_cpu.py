"""CPU checks of the full-rank Gaussian family (NF_KIND_FULLRANK, Shift o Scale(LowerTriangular)): the numpy reference
tests/fullrank_ref.py against finite differences and closed forms, the library's host side with a stand-in context (every
refusal below comes before any device work), the Python mirror, the new kernels' scratch, and the conditioning of the inputs
test_gpu_fullrank.py runs -- no GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fullrank_cases as fc
import fullrank_ref as fr
import parity as P
from __graft_entry__ import build, load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF_ERR_ARG, NF_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(1, 3), (4, 7), (9, 5)])
def test_reference_gradient_against_central_differences(d, n):
    theta, x = fc.inputs(d, n, True, nan_upper=False)
    for name in ("diaggauss", "mvnormal", "glm_logit"):
        ref = fc.numpy_target(name, d, True)
        _, g = fr.neg_elbo_value_and_grad(theta, x, ref)
        low = ~fc.upper_mask(d)
        fd = np.zeros_like(theta)
        h = 1e-6
        for p in np.flatnonzero(low):
            tp, tm = theta.copy(), theta.copy()
            tp[p] += h
            tm[p] -= h
            fd[p] = (fr.neg_elbo_value_and_grad(tp, x, ref)[0] - fr.neg_elbo_value_and_grad(tm, x, ref)[0]) / (2 * h)
        err = np.abs(g - fd).max() / np.abs(fd).max()
        print(f"fullrank reference d={d} {name}: gradient vs central differences {err:.2e}")
        assert err <= 1e-6
        assert (g[fc.upper_mask(d)] == 0.0).all()


def test_reference_pullback_against_central_differences():
    d, n = 5, 6
    theta, x = fc.inputs(d, n, True, nan_upper=False)
    rng = np.random.default_rng(1)
    ybar, lbar = rng.standard_normal((d, n)), rng.standard_normal(n)

    def f(th, xx):
        y, ladj = fr.fwd(th, xx)
        return (ybar * y).sum() + (lbar * ladj).sum()

    xbar, g = fr.bwd(theta, x, ybar, lbar)
    h = 1e-6
    for p in np.flatnonzero(~fc.upper_mask(d)):
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        assert abs((f(tp, x) - f(tm, x)) / (2 * h) - g[p]) <= 1e-6 * max(1.0, abs(g[p]))
    xp, xm = x.copy(), x.copy()
    xp[2, 3] += h
    xm[2, 3] -= h
    assert abs((f(theta, xp) - f(theta, xm)) / (2 * h) - xbar[2, 3]) <= 1e-6


@pytest.mark.parametrize("d", [1, 5, 33])
def test_ladj_is_the_jacobians_slogdet_and_the_inverse_inverts(d):
    theta, x = fc.inputs(d, 4, True)  # NaN above the diagonal: never read
    y, ladj = fr.fwd(theta, x)
    _, L = fr.split(theta, d)
    assert np.isfinite(y).all()
    assert np.allclose(ladj, np.linalg.slogdet(L)[1], rtol=1e-13, atol=1e-13)  # dy/dx = L
    assert np.linalg.det(L) < 0  # one diagonal entry is negative: |.| matters
    xr, li = fr.inv(theta, y)
    assert np.abs(xr - x).max() <= 1e-12 and np.allclose(li, -ladj, rtol=0, atol=1e-14)


def test_elbo_of_the_exact_posterior_is_zero_for_every_sample():
    """test/objectives.jl:15-18 with a full covariance: q = p gives elbo_j = 0 for every draw"""
    d, n = 6, 50
    m, Sigma = fc.gauss_arrays(d)
    Lc = np.linalg.cholesky(Sigma)
    W = np.linalg.solve(Lc, np.eye(d))
    theta = fr.join(m, Lc)
    x = np.random.default_rng(2).standard_normal((d, n))
    e = fr.elbos(theta, x, lambda y: fc.gauss_logp_score(y, m, W, -np.log(np.diag(Lc)).sum()))
    assert np.abs(e).max() <= 1e-12


# ---- host side of the library ------------------------------------------------------------------------------------------------------
def _standin():
    """A zeroed context whose device ordinal does not exist: an entry point that passes its argument and capability checks
    fails at hipSetDevice with a HIP error (> 0) and touches nothing -- with or without a GPU in the machine."""
    buf = (C.c_char * 4096)()
    C.cast(buf, C.POINTER(C.c_int32))[0] = 1 << 20
    return C.cast(buf, C.c_void_p), buf


def _desc(nf, d, dtype=0, nlayers=1):
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    desc = FlowDesc()
    desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND["fullrank"], dtype, d, nlayers
    return desc


def test_kind_constant_matches_the_header(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = dict(re.findall(r"^#define (NF_KIND_\w+) (\d+)", hdr, re.M))
    assert int(defs["NF_KIND_FULLRANK"]) == nf._lib.NF_KIND["fullrank"] == 7
    assert nf.load_library().nf_abi_version() == 4


def test_counts_and_envelope(nf):
    lib = nf.load_library()
    ctx, keep = _standin()
    for dtype in (0, 1):
        for d in (1, 5, 256):
            desc = _desc(nf, d, dtype)
            assert int(lib.nf_param_count(C.byref(desc))) == d + d * d
            assert int(lib.nf_layer_count(C.byref(desc))) == 2
            assert int(lib.nf_workspace_bytes(ctx, C.byref(desc), 100)) > 0
            assert int(lib.nf_tape_bytes(ctx, C.byref(desc), 100)) >= 100 * d * (8 if dtype else 4)
        assert int(lib.nf_tape_bytes(ctx, C.byref(_desc(nf, 257, dtype)), 100)) == NF_ERR_UNSUPPORTED
        assert int(lib.nf_workspace_bytes(ctx, C.byref(_desc(nf, 257, dtype)), 100)) == NF_ERR_UNSUPPORTED
        assert int(lib.nf_tape_bytes(ctx, C.byref(_desc(nf, 4, dtype, nlayers=2)), 100)) == NF_ERR_ARG
        assert int(lib.nf_tape_bytes(ctx, C.byref(_desc(nf, 0, dtype)), 100)) == NF_ERR_ARG


def _elbo_entry_points(lib, ctx, desc, tgt, p, val):
    return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
            lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
            lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
            lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None)]


def test_every_target_kind_is_accepted(nf):
    """all 13 built-in kinds at a valid d, both element types: the four ELBO entry points get past every refusal (and stop at
    the stand-in context's device ordinal)"""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    kinds = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]
    assert len(kinds) == 13
    for dtype in (0, 1):
        for k in kinds:
            d = 2 if k in (3, 4) else 5
            tgt = Target(k, p.value, p.value, 4.0, 0.0 if k == 8 else 1.0)
            codes = _elbo_entry_points(lib, ctx, _desc(nf, d, dtype), tgt, p, val)
            assert all(c > 0 for c in codes), (dtype, k, codes)


def test_refusals_come_before_device_work(nf):
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    ctx, keep = _standin()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    for dtype in (0, 1):
        desc = _desc(nf, 5, dtype)
        # forward KL: value, value and gradient, the step and its graph form
        assert lib.nf_loglikelihood(ctx, C.byref(desc), p, p, 8, None, C.byref(val)) == NF_ERR_UNSUPPORTED
        assert lib.nf_loglikelihood_value_and_grad(ctx, C.byref(desc), p, p, 8, 8, p) == NF_ERR_UNSUPPORTED
        assert lib.nf_loglikelihood_step(ctx, C.byref(desc), p, p, p, p, 8, 8, 0, 1e-3, 0.9, 0.999, 1e-8, None, None) == NF_ERR_UNSUPPORTED
        assert lib.nf_loglikelihood_step_enqueue(ctx, C.byref(desc), p, p, p, p, 8, 8, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
        # the graph-replay ELBO step
        assert lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(diag), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
        # membership in a composition, in either position
        for order in (("planar", "fullrank"), ("fullrank", "planar")):
            segs = (FlowDesc * 2)()
            for g, kind in zip(segs, order):
                g.kind, g.dtype, g.d, g.nlayers = NF_KIND[kind], dtype, 5, 2 if kind == "planar" else 1
            comp = FlowDesc()
            comp.kind, comp.dtype, comp.d, comp.nlayers, comp.nsegments = NF_KIND["composite"], dtype, 5, 1, 2
            comp.segments = C.cast(segs, C.c_void_p)
            assert int(lib.nf_tape_bytes(ctx, C.byref(comp), 10)) == NF_ERR_UNSUPPORTED, order
            assert lib.nf_flow_fwd(ctx, C.byref(comp), p, p, 8, p, p) == NF_ERR_UNSUPPORTED, order
        # beyond the envelope: every entry point, before any launch
        wide = _desc(nf, 257, dtype)
        assert _elbo_entry_points(lib, ctx, wide, diag, p, val) == [NF_ERR_UNSUPPORTED] * 4
        assert lib.nf_flow_fwd(ctx, C.byref(wide), p, p, 8, p, p) == NF_ERR_UNSUPPORTED
    # the mixture in Float32 beyond the tiled kernel's d = 64 (as for the coupling flows); Float64 and d = 64 are served
    mix = Target(8, p.value, p.value, 3.0, 0.0)
    assert _elbo_entry_points(lib, ctx, _desc(nf, 70, 0), mix, p, val) == [NF_ERR_UNSUPPORTED] * 4
    assert lib.nf_elbo_step_enqueue(ctx, C.byref(_desc(nf, 70, 0)), C.byref(mix), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None) == NF_ERR_UNSUPPORTED
    assert all(c > 0 for c in _elbo_entry_points(lib, ctx, _desc(nf, 64, 0), mix, p, val))
    assert all(c > 0 for c in _elbo_entry_points(lib, ctx, _desc(nf, 70, 1), mix, p, val))


# ---- the Python mirror -------------------------------------------------------------------------------------------------------------
def test_python_mirror_on_the_cpu(nf):
    import torch

    d = 4
    for dt in (torch.float32, torch.float64):
        flow = nf.fullrank(nf.MvNormal(d), paramtype=dt, device="cpu")
        assert flow.kind == "fullrank" and flow.P == d + d * d and flow.theta.dtype == dt
        th = flow.theta.numpy()
        assert (th[:d] == 0).all() and (th[d:].reshape(d, d) == np.eye(d)).all()
        mu, Sig = torch.zeros(d, dtype=dt), torch.eye(d, dtype=dt) * 2.0
        from normalizingflows_jl_amd.objectives import _builtin

        gauss = nf.MvNormalTarget(mu, Sig)
        glm = nf.GLMTarget("logit", torch.ones(3, d, dtype=dt))
        mix = nf.MixtureTarget(torch.tensor([0.5, 0.5], dtype=dt), torch.zeros(2, d, dtype=dt), torch.stack([Sig, Sig]))
        diag = nf.DiagGaussTarget(mu, torch.ones(d, dtype=dt))
        for tgt in (gauss, glm, mix, diag):
            assert _builtin(flow, tgt) is True
        # the other kinds answer as before
        mf = nf.meanfield(nf.MvNormal(d), paramtype=dt, device="cpu")
        pl = nf.planarflow(nf.MvNormal(d), 2, paramtype=dt, device="cpu")
        rn = nf.realnvp(nf.MvNormal(d), [8, 8], 1, paramtype=dt, device="cpu")
        for tgt in (gauss, glm, mix):
            assert _builtin(mf, tgt) is False and _builtin(pl, tgt) is False and _builtin(rn, tgt) is True
        assert _builtin(mf, diag) is True and _builtin(flow, lambda y: y.sum(0)) is False
        with pytest.raises(nf.NFHipError):
            nf.create_flow([flow, pl], nf.MvNormal(d))
    # Float32 beyond the tiled mixture kernel: the closure route, as for the coupling flows
    d = 70
    Sig = torch.eye(d)
    mix = nf.MixtureTarget(torch.tensor([0.5, 0.5]), torch.zeros(2, d), torch.stack([Sig, Sig]))
    from normalizingflows_jl_amd.objectives import _builtin

    assert _builtin(nf.fullrank(nf.MvNormal(d), paramtype=torch.float32, device="cpu"), mix) is False
    mix64 = nf.MixtureTarget(torch.tensor([0.5, 0.5], dtype=torch.float64), torch.zeros(2, d, dtype=torch.float64), torch.stack([Sig, Sig]).double())
    assert _builtin(nf.fullrank(nf.MvNormal(d), paramtype=torch.float64, device="cpu"), mix64) is True


# ---- the new kernels are register-resident ---------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_fr_gemm<", 4), ("void k_fr_bwd<", 4), ("k_fr_tri_inverse(", 1), ("void k_fr_shift<", 2),
                          ("void k_fr_apply_flat<", 1), ("void k_fr_grad_flat<", 1)):
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        assert all(r[4] == 0 for r in hit), [(r[0][:60], r[4]) for r in hit]


# ---- the GPU cases' inputs are well conditioned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", fc.SHAPES + [(fc.GRID_STRIDE_D, fc.GRID_STRIDE_N)])
def test_float32_floor_is_far_inside_the_tolerances(d, n):
    """For every GPU case, the float32 evaluation of the reference is within 0.5 x the stated tolerance for y, 0.05 x for loss
    and gradient, and its own round trip is within 2e-7: the plain tolerances hold outright for a correct kernel, and the
    `floor=` clause of tests/parity.py cannot hide a wrong one."""
    theta, x = fc.inputs(d, n, False)
    _, L = fr.split(theta, d)
    assert np.linalg.cond(L) <= 1.9
    t32, x32 = theta.astype(np.float32), x.astype(np.float32)
    y, ladj = fr.fwd(theta, x)
    y32, l32 = fr.fwd(t32, x32)
    ry = (np.abs(y32 - y) / (P.Y_ATOL + P.Y_RTOL * np.abs(y))).max()
    rl = (np.abs(l32 - ladj) / (P.Y_ATOL + P.Y_RTOL * np.abs(ladj))).max()
    xr32, _ = fr.inv(t32, y32)
    rt = np.linalg.norm(xr32.astype(np.float64) - x) / np.linalg.norm(x)
    print(f"fullrank floor d={d} N={n}: y {ry:.3f}x ladj {rl:.3f}x round trip {rt:.2e}")
    assert ry <= 0.5 and rl <= 0.5 and rt <= 2e-7
    for name in fc.target_names(d, False):
        ref = fc.numpy_target(name, d, False)
        l_ref, g_ref = fr.neg_elbo_value_and_grad(theta, x, ref)
        l_32, g_32 = fr.neg_elbo_value_and_grad(t32, x32, ref)
        rloss = abs(l_32 - l_ref) / abs(l_ref) / P.LOSS_RTOL
        rgrad = np.abs(g_32 - g_ref).max() / np.abs(g_ref).max() / P.GRAD_RTOL
        print(f"fullrank floor d={d} N={n} {name}: loss {rloss:.4f}x gradient {rgrad:.4f}x")
        assert rloss <= 0.05 and rgrad <= 0.05, (name, rloss, rgrad)
