"""GPU parity of the non-centred flow (NF_KIND_NONCENTRED: y = S(T(x)), S the non-centring layer of a hierarchical target, T a
RealNVP, NSF or full-rank flow) against the numpy reference tests/noncentred_ref.py (validated against central differences in
test_noncentred_cpu.py), at the criteria of tests/parity.py.  The cases are the smallest that reach every path: the small
hierarchical and dispersion shapes, the wide one (three feature blocks), d = 64 under the pair kernel, every inner family on
the tiled kernels, the general kernels in Float32, Float64, a partly filled last tile and a single sample.  On the parent
commit kind 10 is NF_ERR_ARG and every test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

import noncentred_cases as nc
import noncentred_ref as ncr
import parity as P
from __graft_entry__ import load_package
from test_gpu_fullrank import bits, host, tag, vec
from test_gpu_linpred import new_ctx, tdt, to_dev, vp

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
# name -> (shape, inner flow, N)
CASES = {
    "small-realnvp": ("small", "realnvp", 33),    # LDS-resident RealNVP [32, 32]: the activation stash; the second tile holds one sample
    "disp-realnvp": ("disp", "realnvp", 33),      # d = p + G + 1
    "small-nsf": ("small", "nsf", 33),            # spline couplings, K = 8, hidden 32: the spline tape
    "small-fullrank": ("small", "fullrank", 33),  # the tiled full-rank family, one feature block
    "wide-realnvp": ("wide", "realnvp", 40),      # d = 70: the weight-streaming RealNVP, three feature blocks
    "wide-fullrank": ("wide", "fullrank", 40),    # DB = 4
    "pair": ("pair", "realnvp64", 40),            # d = 64 under RealNVP [64, 64]: the pair kernel's path
    "flat32": ("disp", "nsf64", 33),              # Float32 on the general kernels: the standard layout
    "single": ("small", "realnvp", 1),            # a single sample
}
TILED = ["small-realnvp", "disp-realnvp", "small-nsf", "small-fullrank", "wide-realnvp", "wide-fullrank", "pair"]
F64_CASES = ["small-realnvp", "disp-realnvp", "wide-fullrank"]  # Float64 RealNVP (both forms) and Float64 fullrank


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def inner_spec(kind, d):
    if kind == "nsf64":
        import nf_oracle as o

        return o.FlowSpec("nsf", d, 1, (64, 64), 8, 30.0)
    return nc.inner_spec(kind, d)


def make_inner(nf, g, f64):
    q0 = nf.MvNormal(g.d)
    if g.kind == "realnvp":
        return nf.realnvp(q0, g.hdims, g.nlayers, paramtype=tdt(f64))
    if g.kind == "nsf":
        return nf.nsf(q0, g.hdims, g.K, g.B, g.nlayers, paramtype=tdt(f64))
    return nf.fullrank(q0, paramtype=tdt(f64))


_TARGETS, _CASES = {}, {}


def target(nf, shape, f64):
    """(device target, ref) -- one per (shape, element type)"""
    if (shape, f64) not in _TARGETS:
        _TARGETS[(shape, f64)] = nc.make_target(nf, shape, tdt(f64), "cuda")
    return _TARGETS[(shape, f64)]


def case(nf, name, f64, lam=None, nan_fixed=False, frozen=False):
    """(spec, n, theta, x, flow, xs, tgt, ref) -- computed once per key and left unchanged"""
    key = (name, f64, lam, nan_fixed, frozen)
    if key not in _CASES:
        shape, kind, n = CASES[name]
        form, p, G = nc.SHAPES[shape]
        spec = ncr.Spec(inner_spec(kind, nc.dim(shape)), ncr.groups(p, G), G, frozen)
        theta, x = ncr.inputs(spec, n, f64, lam=lam, nan_fixed=nan_fixed)
        tgt, ref = target(nf, shape, f64)
        flow = nf.noncentred(make_inner(nf, spec.inner, f64), tgt, learn=not frozen)
        assert flow.P == theta.size == ncr.param_count(spec)
        _CASES[key] = (spec, n, theta, x, flow.with_theta(vec(theta, f64)), to_dev(x, f64), tgt, ref)
    return _CASES[key]


def cases(names32, with_f64=True):
    out = [(n, False) for n in names32] + ([(n, True) for n in F64_CASES] if with_f64 else [])
    return pytest.mark.parametrize("name,f64", out, ids=[f"{n}-{tag(f)}" for n, f in out])


def f32(*a):
    return tuple(v.astype(np.float32) for v in a)


# ---- 1. forward, inverse, layers, rand, logpdf -------------------------------------------------------------------------------------
@cases(TILED + ["flat32", "single"])
def test_forward_inverse_layers_rand_logpdf(nf, name, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, name, f64)
    key = f"noncentred {name} {tag(f64)}"
    y, ladj = nf.with_logabsdet_jacobian(flow.transform, xs)
    torch.cuda.synchronize()
    y_ref, l_ref = ncr.fwd(spec, theta, x)
    assert np.isfinite(host(y)).all() and np.isfinite(host(ladj)).all(), key
    t32, x32 = f32(theta, x)
    if f64:
        P.elementwise(key + ": y", y, y_ref, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": ladj", ladj, l_ref, P.F64_RTOL, 1e-12)
    else:
        y32, l32 = ncr.fwd(spec, t32, x32)
        P.elementwise(key + ": y", y, y_ref, floor=y32)
        P.elementwise(key + ": ladj", ladj, l_ref, floor=l32)
    # round trip, norm-wise at the inner kind's tolerance, and ladj_inv = -ladj
    rt = P.INV_RTOL.get(spec.inner.kind, 1e-6)
    xr, lr = nf.with_logabsdet_jacobian(nf.inverse(flow.transform), y)
    if f64:
        P.isapprox(key + ": round trip x", xr, x, P.F64_GRAD)
        P.isapprox(key + ": round trip ladj", lr, -host(ladj), P.F64_GRAD)
    else:
        xr32, lr32 = ncr.inv(spec, t32, y32)
        P.isapprox(key + ": round trip x", xr, x, rt, floor_err=P.relerr(xr32, x))
        P.isapprox(key + ": round trip ladj", lr, -host(ladj), rt, floor_err=P.relerr(lr32, -l32.astype(np.float64)))
    # the inverse against the reference's, at the flow's own outputs (as the device holds them)
    yh = host(y)
    x_ref, li_ref = ncr.inv(spec, theta, yh)
    if f64:
        P.isapprox(key + ": inverse x", xr, x_ref, P.F64_GRAD)
        P.elementwise(key + ": inverse ladj", lr, li_ref, P.F64_RTOL, 1e-12)
    else:
        xi32, li32 = ncr.inv(spec, t32, yh.astype(np.float32))
        P.isapprox(key + ": inverse x", xr, x_ref, rt, floor_err=P.relerr(xi32, x_ref))
        P.elementwise(key + ": inverse ladj", lr, li_ref, floor=li32)
    # single bijectors: the inner flow's first layer, and S, the last one, in both directions
    last = ncr.layer_count(spec) - 1
    for i in (0, last):
        yi, li = nf.with_logabsdet_jacobian(nf.layer(flow, i), xs)
        yi_ref, li_ref = ncr.layer(spec, theta, i, x)
        if f64:
            P.elementwise(f"{key}: layer {i} y", yi, yi_ref, P.F64_RTOL, 1e-12)
            P.elementwise(f"{key}: layer {i} ladj", li, li_ref, P.F64_RTOL, 1e-12)
        else:
            yi32, li32 = ncr.layer(spec, t32, i, x32)
            P.elementwise(f"{key}: layer {i} y", yi, yi_ref, floor=yi32)
            P.elementwise(f"{key}: layer {i} ladj", li, li_ref, floor=li32)
    zs, ls = nf.with_logabsdet_jacobian(nf.inverse(nf.layer(flow, last)), yi)
    torch.cuda.synchronize()
    assert bits(ls) == bits(-li), key  # tau passes through: the same terms, the same order, the other sign
    P.isapprox(key + ": S round trip", zs, x, P.F64_GRAD if f64 else 1e-6)
    with pytest.raises(nf.NFHipError):
        nf.with_logabsdet_jacobian(nf.layer(flow, last + 1), xs)
    # rand: the forward of the base draws, bit for bit
    ys = nf.rand(flow, n, nf.PhiloxRNG(9))
    xd = nf.device_specific_rand(nf.PhiloxRNG(9), flow.dist, n, dtype=tdt(f64))
    yd, _ = nf.with_logabsdet_jacobian(flow.transform, xd)
    torch.cuda.synchronize()
    assert bits(ys) == bits(yd) and np.isfinite(host(ys)).all(), key
    # logpdf(flow, y)
    lp = nf.logpdf(flow, y)
    lp_ref = ncr.logpdf(spec, theta, yh)
    if f64:
        P.elementwise(key + ": logpdf", lp, lp_ref, P.F64_RTOL, 1e-12)
    else:
        P.elementwise(key + ": logpdf", lp, lp_ref, floor=ncr.logpdf(spec, t32, yh.astype(np.float32)))


# ---- 2. the tape pair ----------------------------------------------------------------------------------------------------------------
@cases(TILED + ["flat32", "single"])
def test_tape_pullback(nf, name, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, name, f64)
    d = spec.d
    key = f"noncentred pullback {name} {tag(f64)}"
    rng = np.random.default_rng(8)
    ybar64, lbar64 = ncr.rounded(rng.standard_normal((d, n)), f64), ncr.rounded(rng.standard_normal(n), f64)
    ybar, lbar = to_dev(ybar64, f64), vec(lbar64, f64)
    (y, ladj), pullback = nf.rrule_with_logabsdet_jacobian(flow.transform, xs)
    xbar, g = pullback(ybar, lbar)
    torch.cuda.synchronize()
    _, _, tape = ncr.fwd(spec, theta, x, keep=True)
    xbar_ref, g_ref = ncr.bwd(spec, theta, tape, ybar64, lbar64)
    if spec.inner.kind == "fullrank":  # the reference's zeros above the diagonal (the device's too: exactly)
        import fullrank_cases as fc

        up = np.concatenate([np.zeros(spec.p, dtype=bool), fc.upper_mask(d)])
        assert bool((g[torch.tensor(up, device="cuda")] == 0.0).all()), key
    if f64:
        P.gradient(key + ": xbar", xbar, xbar_ref, P.F64_GRAD)
        P.gradient(key + ": gtheta", g, g_ref, P.F64_GRAD)
    else:
        t32, x32, yb32, lb32 = f32(theta, x, ybar64, lbar64)
        _, _, tape32 = ncr.fwd(spec, t32, x32, keep=True)
        xb32, g32 = ncr.bwd(spec, t32, tape32, yb32, lb32)
        P.gradient(key + ": xbar", xbar, xbar_ref, floor=xb32)
        P.gradient(key + ": gtheta", g, g_ref, floor=g32)
        P.gradient(key + ": glam", g[:spec.p], g_ref[:spec.p], floor=g32[:spec.p])
    fixed = torch.tensor(ncr.fixed_mask(spec), device="cuda")
    assert bool((g[fixed] == 0.0).all()), key  # exactly 0.0 where lam is not read
    # a second pullback from the same tape: the same bits
    xbar2, g2 = pullback(ybar, lbar)
    assert bits(xbar2) == bits(xbar) and bits(g2) == bits(g), key


# ---- 3. ELBO value and gradient: caller's draws and in-library draws; nf_elbo_batch -------------------------------------------------
def check_vg(key, spec, theta, x, ref, f64, loss, grad):
    l_ref, g_ref = ncr.neg_elbo_value_and_grad(spec, theta, x, ref)
    assert np.isfinite(loss) and np.isfinite(host(grad)).all(), key
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": gradient", grad, g_ref, P.F64_GRAD)
    else:
        l32, g32 = ncr.neg_elbo_value_and_grad(spec, *f32(theta, x), ref)
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": gradient", grad, g_ref, floor=g32)
        P.gradient(key + ": glam", grad[:spec.p], g_ref[:spec.p], floor=g32[:spec.p])
    assert bool((grad[torch.tensor(ncr.fixed_mask(spec), device="cuda")] == 0.0).all()), key


@cases(TILED + ["flat32", "single"])
def test_elbo_value_and_gradient(nf, name, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, name, f64)
    key = f"noncentred vg {name} {tag(f64)}"
    loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    torch.cuda.synchronize()
    check_vg(key + " xs", spec, theta, x, ref, f64, loss, grad)
    # per-sample terms and the value-only entry points
    e = nf.batched_elbos(flow, tgt, xs)
    e_ref = ncr.elbos(spec, theta, x, ref)
    if f64:
        P.elementwise(key + ": elbo terms", e, e_ref, P.F64_RTOL, 1e-12)
    else:
        P.elementwise(key + ": elbo terms", e, e_ref, floor=ncr.elbos(spec, *f32(theta, x), ref))
    P.scalar(key + ": elbo_batch", nf.elbo_batch(flow, tgt, xs), float(host(e).mean()), P.F64_RTOL if f64 else P.LOSS_RTOL)
    # in-library draws: the reference on the same draws
    seed = 41
    l_rng, g_rng = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
    xd = nf.device_specific_rand(nf.PhiloxRNG(seed), flow.dist, n, dtype=tdt(f64))
    torch.cuda.synchronize()
    check_vg(key + " rng", spec, theta, host(xd), ref, f64, l_rng, g_rng)
    # two calls: the same bits
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
    assert l2 == l_rng and bits(g2) == bits(g_rng), key


def test_a_target_other_than_the_layers_own(nf):
    """S reads its groups from the flow's target; the ELBO target of the entry points may be any other the inner flow is served with"""
    from test_gpu_fullrank import device_target

    spec, n, theta, x, flow, xs, _, _ = case(nf, "small-realnvp", False)
    tgt, ref = device_target(nf, "diaggauss", spec.d, False)
    loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    check_vg("noncentred vg small-realnvp diaggauss", spec, theta, x, ref, False, loss, grad)


def test_under_a_stash_budget_that_splits_the_bare_flows_step(nf):
    """d = 64, RealNVP [64, 64], 200 samples under a 384 KiB budget: the bare flow's step runs two chunks of its activation stash
    (128 + 72 samples); the non-centred step keeps the chain's output instead and its reverse pass recomputes -- the same numbers"""
    lib = nf.load_library()
    spec, _, theta, _, flow, _, tgt, ref = case(nf, "pair", False)
    n = 200
    x = ncr.rounded(np.random.default_rng(12).standard_normal((spec.d, n)), False)
    xs = to_dev(x, False)
    whole = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    ctx = flow.ctx
    nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, 3 << 17))
    try:
        loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
        torch.cuda.synchronize()
    finally:
        nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, -1))
    check_vg("noncentred vg pair under a two-chunk stash budget", spec, theta, x, ref, False, loss, grad)
    check_vg("noncentred vg pair N=200", spec, theta, x, ref, False, *whole)


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------
@cases(["small-realnvp", "wide-fullrank"])
def test_two_shards_sum_to_the_whole_batch(nf, name, f64):
    spec, n, theta, x, flow, _, tgt, _ = case(nf, name, f64)
    key = f"noncentred shards {name} {tag(f64)}"
    seed = 43
    l_all, g_all = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
    n_a = (2 * n) // 3
    l_a, g_a = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n_a, rng=nf.PhiloxRNG(seed), n_global=n)
    l_b, g_b = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n - n_a, rng=nf.PhiloxRNG(seed, sample_offset=n_a), n_global=n)
    P.scalar(key + ": loss", l_a + l_b, l_all, P.F64_RTOL if f64 else P.LOSS_RTOL)
    P.gradient(key + ": gradient", g_a + g_b, host(g_all), P.F64_GRAD if f64 else P.GRAD_RTOL)


# ---- 5. the step -------------------------------------------------------------------------------------------------------------------
@cases(["small-realnvp", "small-nsf", "wide-fullrank"], with_f64=False)
def test_elbo_step_equals_the_split_calls(nf, name, f64):
    """two nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit in theta, m, v; a second
    run of the step gives identical theta, m, v; the graph form refuses and touches nothing"""
    lib = nf.load_library()
    spec, n, theta, x, flow, _, tgt, _ = case(nf, name, f64, nan_fixed=False)
    seed, dt = 77, 1 if f64 else 0
    ctx_a, ctx_b, ctx_c = new_ctx(nf), new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert code == -2 and torch.equal(th, flow.theta) and int(counter[0]) == 0
    with pytest.raises(nf.NFHipError):
        nf._lib.check(code)
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    th_c, m_c, v_c = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, dtype=tdt(f64), device="cuda"), torch.empty(1, dtype=tdt(f64), device="cuda")
    fixed = torch.tensor(ncr.fixed_mask(spec), device="cuda")
    for step in range(2):
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS,
                                       C.byref(loss), C.byref(gnorm)))
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, dt, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        nf._lib.check(lib.nf_elbo_step(ctx_c.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_c), vp(m_c), vp(v_c), n, seed, step, LR, B1, B2, EPS,
                                       None, None))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert torch.equal(th, th_c) and torch.equal(m, m_c) and torch.equal(v, v_c), step
        assert loss.value == float(out[flow.P]) and gnorm.value == float(gn), step
        assert np.isfinite(loss.value)
        # Adam leaves the lam of a coefficient without a group alone
        assert torch.equal(th[fixed], flow.theta[fixed]) and bool((m[fixed] == 0.0).all()) and bool((v[fixed] == 0.0).all()), step
    assert not torch.equal(th, flow.theta)
    for c in (ctx_a, ctx_b, ctx_c):
        c.close()


# ---- 6. the exact checks -----------------------------------------------------------------------------------------------------------
@cases(TILED + ["flat32"])
def test_lam_zero_gives_the_inner_flows_own_bits(nf, name, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, name, f64, lam=0.0)
    inner = flow.inner.with_theta(flow.theta[spec.p:].clone())
    y, ladj = nf.with_logabsdet_jacobian(flow.transform, xs)
    y0, l0 = nf.with_logabsdet_jacobian(inner.transform, xs)
    torch.cuda.synchronize()
    assert bits(y) == bits(y0) and bits(ladj) == bits(l0), name
    # ... and through the tiled training sequence: the loss and the inner flow's gradient are the bare flow's
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(3))
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, inner, tgt, n, rng=nf.PhiloxRNG(3))
    P.scalar(f"noncentred lam=0 {name} {tag(f64)}: loss vs the inner flow's", l1, l2, P.F64_RTOL if f64 else P.LOSS_RTOL)
    P.gradient(f"noncentred lam=0 {name} {tag(f64)}: inner gradient vs the inner flow's", g1[spec.p:], host(g2), P.F64_GRAD if f64 else P.GRAD_RTOL)


@cases(TILED + ["flat32"])
def test_nan_in_an_unread_lam_changes_no_bit(nf, name, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, name, f64)
    _, _, theta_n, _, flow_n, _, _, _ = case(nf, name, f64, nan_fixed=True)
    fixed = ncr.fixed_mask(spec)
    assert fixed[:spec.p].any() and np.isnan(theta_n[fixed]).all() and np.array_equal(theta_n[~fixed], theta[~fixed])
    rng = np.random.default_rng(8)
    ybar, lbar = to_dev(rng.standard_normal((spec.d, n)), f64), vec(rng.standard_normal(n), f64)
    res = []
    for f in (flow, flow_n):
        y, ladj = nf.with_logabsdet_jacobian(f.transform, xs)
        xr, lr = nf.with_logabsdet_jacobian(nf.inverse(f.transform), y)
        (_, _), pullback = nf.rrule_with_logabsdet_jacobian(f.transform, xs)
        xbar, g = pullback(ybar, lbar)
        loss, grad = nf.value_and_gradient(nf.elbo_batch, f, tgt, n, rng=nf.PhiloxRNG(5))
        torch.cuda.synchronize()
        res.append((bits(y), bits(ladj), bits(xr), bits(lr), bits(xbar), bits(g), loss, bits(grad)))
        ft = torch.tensor(fixed, device="cuda")
        assert bool((g[ft] == 0.0).all()) and bool((grad[ft] == 0.0).all()) and np.isfinite(loss), name
    assert res[0] == res[1], name


@cases(TILED + ["flat32"])
def test_a_frozen_lam_has_exactly_zero_gradient(nf, name, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, name, f64)
    spec_f, _, _, _, flow_f, _, _, _ = case(nf, name, f64, frozen=True)
    assert flow_f.desc.K == 1 and torch.equal(flow_f.theta, flow.theta)
    p = spec.p
    loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(5))
    loss_f, grad_f = nf.value_and_gradient(nf.elbo_batch, flow_f, tgt, n, rng=nf.PhiloxRNG(5))
    assert bool((grad_f[:p] == 0.0).all()) and not bool((grad[:p] == 0.0).all()), name
    assert loss_f == loss and bits(grad_f[p:]) == bits(grad[p:]), name  # everything else: the same bits
    rng = np.random.default_rng(8)
    ybar, lbar = to_dev(rng.standard_normal((spec.d, n)), f64), vec(rng.standard_normal(n), f64)
    (_, _), pullback = nf.rrule_with_logabsdet_jacobian(flow_f.transform, xs)
    xbar, g = pullback(ybar, lbar)
    assert bool((g[:p] == 0.0).all()) and np.isfinite(host(xbar)).all(), name


# ---- 7. training -------------------------------------------------------------------------------------------------------------------
def test_training_reduces_the_loss(nf):
    spec, n, theta, x, flow0, xs, tgt, ref = case(nf, "small-realnvp", False)
    flow = nf.noncentred(flow0.inner.with_theta(flow0.theta[spec.p:].clone()), tgt)
    trained, stats, _ = nf.train_flow(nf.elbo_batch, flow, tgt, 1024, max_iters=50, optimiser=nf.Adam(1e-2))
    losses = [s["loss"] for s in stats]
    print(f"noncentred training: loss {losses[0]:.4f} -> {losses[-1]:.4f}; lam {trained.lam.tolist()}")
    assert trained.kind == "noncentred" and len(stats) == 50 and all(np.isfinite(l) for l in losses)
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    fixed = torch.tensor(ncr.fixed_mask(spec)[:spec.p], device="cuda")
    assert bool((trained.lam[fixed] == 1.0).all()) and not bool((trained.lam[~fixed] == 1.0).any())


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_refusals_raise(nf, f64):
    spec, n, theta, x, flow, xs, tgt, ref = case(nf, "small-realnvp", f64)
    with pytest.raises(nf.NFHipError):
        nf.loglikelihood_value_and_gradient(flow, xs)
    with pytest.raises(nf.NFHipError):
        nf.train_flow(nf.loglikelihood, flow, xs, max_iters=1)
    with pytest.raises(nf.NFHipError):
        nf.create_flow([flow, nf.planarflow(nf.MvNormal(spec.d), 2, paramtype=tdt(f64))], nf.MvNormal(spec.d))
    assert np.isfinite(nf.loglikelihood(None, flow, xs))  # the value is served
