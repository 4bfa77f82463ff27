"""GPU parity of the full-rank Gaussian family (NF_KIND_FULLRANK: y = mu + L x, L lower triangular) against the numpy
reference tests/fullrank_ref.py, on the inputs of tests/fullrank_cases.py (whose conditioning test_fullrank_cpu.py checks:
the float32 floor is far inside every tolerance used here).  The strict upper triangle of theta's matrix is NaN in every
test but the Adam one: it is never read."""
import ctypes as C

import numpy as np
import pytest
import torch

import fullrank_cases as fc
import fullrank_ref as fr
import glm_forms as gf
import nf_oracle as o
import parity as P
from __graft_entry__ import load_package
from test_gpu_linpred import gauss_logp_score, new_ctx, tdt, to_dev, vp
from test_mixture_cpu import cast_pack, mixture_logp_score, random_mixture, target_pack

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
F64 = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def grid_stride_shape():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return fc.GRID_STRIDE_D, 32 * cus + 33


def all_shapes():
    return fc.SHAPES + ["grid-stride"]


def shape_of(s):
    return grid_stride_shape() if s == "grid-stride" else s


SHAPE = pytest.mark.parametrize("shape", all_shapes(), ids=lambda s: s if isinstance(s, str) else f"d{s[0]}-N{s[1]}")


def vec(a, f64):
    return torch.tensor(np.asarray(a), dtype=tdt(f64), device="cuda")


def make_flow(nf, theta, d, f64):
    flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64))
    flow.theta = vec(theta, f64)
    return flow


def host(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    """a tensor's bytes (NaN-safe equality)"""
    return t.detach().cpu().contiguous().numpy().tobytes()


_CASES = {}


def case(nf, shape, f64, nan_upper=True):
    """(d, n, theta, x, flow, xs) -- computed once per (shape, element type) and left unchanged"""
    d, n = shape_of(shape)
    key = (d, n, f64, nan_upper)
    if key not in _CASES:
        theta, x = fc.inputs(d, n, f64, nan_upper=nan_upper)
        _CASES[key] = (d, n, theta, x, make_flow(nf, theta, d, f64), to_dev(x, f64))
    return _CASES[key]


# ---- device targets with the closed forms of the values they hold --------------------------------------------------------------
_TARGETS = {}


def device_target(nf, name, d, f64):
    """(target, ref): ref(y) -> (log p, score) in y's dtype, from the device target's own (rounded) arrays"""
    key = (name, d, f64)
    if key in _TARGETS:
        return _TARGETS[key]
    if name == "diaggauss":
        mu, var = fc.diag_arrays(d)
        tgt = nf.DiagGaussTarget(vec(mu, f64), vec(var, f64))
        m, v = host(tgt.mu), host(tgt.var)
        ref = lambda y: (o.target_logp(("diaggauss", m.astype(y.dtype), v.astype(y.dtype)), y),
                         o.target_grad(("diaggauss", m.astype(y.dtype), v.astype(y.dtype)), y))
    elif name == "funnel":
        tgt = nf.FunnelTarget(d, 0.0, 3.0)
        ref = lambda y: (o.target_logp(("funnel", 0.0, 3.0), y), o.target_grad(("funnel", 0.0, 3.0), y))
    elif name == "mvnormal":
        mu, Sigma = fc.gauss_arrays(d)
        tgt = nf.MvNormalTarget(vec(mu, f64), vec(Sigma, f64))
        W, m = host(tgt.W), host(tgt.mu)
        ref = lambda y: gauss_logp_score(y, m.astype(y.dtype), W.astype(y.dtype), tgt.logdet_w)
    elif name.startswith("glm_"):
        A, wt = fc.glm_arrays(name[4:], d)
        tgt = nf.GLMTarget(name[4:], vec(A, f64), None, vec(wt, f64), None, prior_sigma=2.0)
        ref = gf.ref_of(tgt)
    else:
        assert name == "mixture3", name
        pi, mus, Sig = random_mixture(d, 3)
        tgt = nf.MixtureTarget(vec(pi, f64), vec(mus, f64), vec(Sig, f64))
        pack = target_pack(tgt)
        ref = lambda y: mixture_logp_score(y, *cast_pack(pack, y.dtype))
    _TARGETS[key] = (tgt, ref)
    return _TARGETS[key]


# ---- 1. forward, inverse, round trip, layers -------------------------------------------------------------------------------------
@F64
@SHAPE
def test_forward_inverse_round_trip_and_layers(nf, shape, f64):
    d, n, theta, x, flow, xs = case(nf, shape, f64)
    key = f"fullrank d={d} N={n} {tag(f64)}"
    y, ladj = nf.with_logabsdet_jacobian(flow.transform, xs)
    torch.cuda.synchronize()
    y_ref, l_ref = fr.fwd(theta, x)
    assert np.isfinite(host(y)).all() and np.isfinite(host(ladj)).all(), key
    if f64:
        P.elementwise(key + ": y", y, y_ref, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": ladj", ladj, l_ref, P.F64_RTOL, 1e-12)
    else:
        y32, l32 = fr.fwd(theta.astype(np.float32), x.astype(np.float32))
        P.elementwise(key + ": y", y, y_ref, floor=y32)
        P.elementwise(key + ": ladj", ladj, l_ref, floor=l32)
    # inverse on data of its own
    ys64 = fc.rounded(0.7 * np.random.default_rng(6).standard_normal((d, n)), f64)
    xi, li = nf.with_logabsdet_jacobian(nf.inverse(flow.transform), to_dev(ys64, f64))
    xi_ref, li_ref = fr.inv(theta, ys64)
    if f64:
        P.elementwise(key + ": inverse x", xi, xi_ref, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": inverse ladj", li, li_ref, P.F64_RTOL, 1e-12)
    else:
        xi32, li32 = fr.inv(theta.astype(np.float32), ys64.astype(np.float32))
        P.elementwise(key + ": inverse x", xi, xi_ref, floor=xi32)
        P.elementwise(key + ": inverse ladj", li, li_ref, floor=li32)
    # round trip, norm-wise at the mean-field family's tolerance, and ladj_inv = -ladj
    xr, lr = nf.with_logabsdet_jacobian(nf.inverse(flow.transform), y)
    P.isapprox(key + ": round trip x", xr, x, P.F64_GRAD if f64 else P.INV_RTOL["meanfield"])
    P.isapprox(key + ": round trip ladj", lr, -host(ladj), P.F64_GRAD if f64 else P.INV_RTOL["meanfield"])
    # layer by layer (flat order: 0 = Shift, applied last; 1 = Scale): y bit for bit, the log-dets add up
    h, l1 = nf.with_logabsdet_jacobian(nf.layer(flow, 1), xs)
    y2, l0 = nf.with_logabsdet_jacobian(nf.layer(flow, 0), h)
    torch.cuda.synchronize()
    assert bits(y2) == bits(y), key
    assert bits(l1) == bits(ladj) and float(l0.abs().max()) == 0.0, key
    # and back through the inverted layers
    h2, _ = nf.with_logabsdet_jacobian(nf.inverse(nf.layer(flow, 0)), y)
    x2, _ = nf.with_logabsdet_jacobian(nf.inverse(nf.layer(flow, 1)), h2)
    assert bits(x2) == bits(xr), key


# ---- 2. value and gradient on supplied draws -------------------------------------------------------------------------------------
def check_value_and_gradient(nf, key, d, theta, x, flow, xs, tgt, ref, f64):
    loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    torch.cuda.synchronize()
    l_ref, g_ref = fr.neg_elbo_value_and_grad(theta, x, ref)
    assert np.isfinite(loss) and np.isfinite(host(grad)).all(), key
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": gradient", grad, g_ref, P.F64_GRAD)
    else:
        l32, g32 = fr.neg_elbo_value_and_grad(theta.astype(np.float32), x.astype(np.float32), ref)
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": gradient", grad, g_ref, floor=g32)
    up = torch.tensor(fc.upper_mask(d), device="cuda")
    assert bool((grad[up] == 0.0).all()), key  # exactly 0.0 above the diagonal
    # the same bits with zeros in place of the NaNs
    flow0 = make_flow(nf, fc.zero_upper(theta, d), d, f64)
    loss0, grad0 = nf.value_and_gradient(nf.elbo_batch, flow0, tgt, xs)
    assert loss0 == loss and bits(grad0) == bits(grad), key
    # the value-only entry point agrees with the step's loss
    val = nf.elbo_batch(flow, tgt, xs)
    P.scalar(key + ": elbo_batch vs -loss", val, -loss, P.F64_RTOL if f64 else 1e-6)
    return loss, grad


@F64
@SHAPE
def test_value_and_gradient_on_supplied_draws(nf, shape, f64):
    d, n, theta, x, flow, xs = case(nf, shape, f64)
    for name in fc.target_names(d, f64):
        tgt, ref = device_target(nf, name, d, f64)
        check_value_and_gradient(nf, f"fullrank vg d={d} N={n} {name} {tag(f64)}", d, theta, x, flow, xs, tgt, ref, f64)


def test_float64_mixture_beyond_the_tiled_kernel_is_served(nf):
    """d = 70 > NF_MIXTURE_TILED_MAXD: Float64 goes through the flat launchers; Float32 is refused as for the coupling flows"""
    d, n, theta, x, flow, xs = case(nf, (70, 40), True)
    tgt, ref = device_target(nf, "mixture3", d, True)
    check_value_and_gradient(nf, "fullrank vg d=70 N=40 mixture3 f64", d, theta, x, flow, xs, tgt, ref, True)
    d, n, theta, x, flow32, xs32 = case(nf, (70, 40), False)
    tgt32, _ = device_target(nf, "mixture3", d, False)
    out = torch.zeros(flow32.P + 1, device="cuda")
    ctx = flow32.ctx
    code = ctx.lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow32.desc), C.byref(tgt32.c), vp(flow32.theta), None, n, n, 1, 0, 0, vp(out))
    torch.cuda.synchronize()
    assert code == -2 and float(out.abs().max()) == 0.0
    from normalizingflows_jl_amd.objectives import _builtin

    assert _builtin(flow32, tgt32) is False and _builtin(flow, tgt) is True


# ---- 3. the tape pullback ------------------------------------------------------------------------------------------------------------
@F64
@SHAPE
def test_tape_pullback(nf, shape, f64):
    d, n, theta, x, flow, xs = case(nf, shape, f64)
    key = f"fullrank pullback d={d} N={n} {tag(f64)}"
    rng = np.random.default_rng(8)
    ybar64, lbar64 = fc.rounded(rng.standard_normal((d, n)), f64), fc.rounded(rng.standard_normal(n), f64)
    ybar, lbar = to_dev(ybar64, f64), vec(lbar64, f64)
    ybar_before, lbar_before = bits(ybar), bits(lbar)
    (y, ladj), pullback = nf.rrule_with_logabsdet_jacobian(flow.transform, xs)
    xbar, g = pullback(ybar, lbar)
    torch.cuda.synchronize()
    xbar_ref, g_ref = fr.bwd(theta, x, ybar64, lbar64)
    if f64:
        P.gradient(key + ": xbar", xbar, xbar_ref, P.F64_GRAD)
        P.gradient(key + ": gtheta", g, g_ref, P.F64_GRAD)
    else:
        xb32, g32 = fr.bwd(theta.astype(np.float32), x.astype(np.float32), ybar64.astype(np.float32), lbar64.astype(np.float32))
        P.gradient(key + ": xbar", xbar, xbar_ref, floor=xb32)
        P.gradient(key + ": gtheta", g, g_ref, floor=g32)
    up = torch.tensor(fc.upper_mask(d), device="cuda")
    assert bool((g[up] == 0.0).all()), key
    # a second pullback from the same tape, and nf_flow_bwd from x alone: the same bits; the caller's cotangents untouched
    xbar2, g2 = pullback(ybar, lbar)
    assert bits(xbar2) == bits(xbar) and bits(g2) == bits(g), key
    xbar3, g3 = nf.new_batch(d, n, tdt(f64), "cuda"), torch.empty(flow.P, dtype=tdt(f64), device="cuda")
    ctx = flow.ctx
    nf._lib.check(ctx.lib.nf_flow_bwd(ctx.ptr, C.byref(flow.desc), vp(flow.theta), vp(xs), vp(y), vp(ybar), vp(lbar), n, vp(xbar3), vp(g3)))
    torch.cuda.synchronize()
    assert bits(xbar3) == bits(xbar) and bits(g3) == bits(g), key
    assert bits(ybar) == ybar_before and bits(lbar) == lbar_before, key


# ---- 4 - 6. in-library draws, shards, reproducibility -----------------------------------------------------------------------------
DRAW_SHAPES = [(5, 70), (33, 65), (256, 96)]


@F64
@pytest.mark.parametrize("shape", DRAW_SHAPES, ids=lambda s: f"d{s[0]}-N{s[1]}")
def test_in_library_draws_shards_and_reproducibility(nf, shape, f64):
    d, n, theta, x, flow, _ = case(nf, shape, f64)
    key = f"fullrank draws d={d} N={n} {tag(f64)}"
    seed = 41
    for name in ("diaggauss", "glm_logit"):
        tgt, _ = device_target(nf, name, d, f64)
        l_rng, g_rng = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
        xs = nf.device_specific_rand(nf.PhiloxRNG(seed), flow.dist, n, dtype=tdt(f64))
        l_xs, g_xs = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
        assert bits(g_rng) == bits(g_xs), (key, name)
        assert abs(l_rng - l_xs) <= (1e-13 if f64 else 1e-6) * abs(l_xs), (key, name, l_rng, l_xs)
        v_rng = nf.elbo_batch(nf.PhiloxRNG(seed), flow, tgt, n)
        P.scalar(f"{key} {name}: elbo_batch(rng) vs -loss", v_rng, -l_rng, P.F64_RTOL if f64 else 1e-6)
        # a second call: the same bits
        l_again, g_again = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
        assert l_again == l_rng and bits(g_again) == bits(g_rng), (key, name)
        # shards of 2/3 and 1/3 of the batch add up to the whole
        n_a = (2 * n) // 3
        l_a, g_a = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n_a, rng=nf.PhiloxRNG(seed), n_global=n)
        l_b, g_b = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n - n_a, rng=nf.PhiloxRNG(seed, sample_offset=n_a), n_global=n)
        if f64:
            P.scalar(f"{key} {name}: shards' loss", l_a + l_b, l_rng, P.F64_RTOL)
            P.gradient(f"{key} {name}: shards' gradient", g_a + g_b, host(g_rng), P.F64_GRAD)
        else:
            P.scalar(f"{key} {name}: shards' loss", l_a + l_b, l_rng)
            P.gradient(f"{key} {name}: shards' gradient", g_a + g_b, host(g_rng))


# ---- 7. the step --------------------------------------------------------------------------------------------------------------------
@F64
@pytest.mark.parametrize("shape,name", [((5, 70), "glm_poisson"), ((33, 65), "mvnormal"), ((70, 40), "diaggauss")],
                         ids=["d5-poisson", "d33-mvnormal", "d70-diaggauss"])
def test_elbo_step_equals_the_split_calls(nf, shape, name, f64):
    """three nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit in theta, m, v;
    the upper triangle of theta (zeros here) is still exactly zero; the graph form refuses and touches nothing."""
    lib = nf.load_library()
    d, n, theta, x, flow, _ = case(nf, shape, f64, nan_upper=False)
    tgt, _ = device_target(nf, name, d, f64)
    seed, dt = 77, 1 if f64 else 0
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert code == -2 and torch.equal(th, flow.theta) and int(counter[0]) == 0
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, dtype=tdt(f64), device="cuda"), torch.empty(1, dtype=tdt(f64), device="cuda")
    up = torch.tensor(fc.upper_mask(d), device="cuda")
    for step in range(3):
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS,
                                       C.byref(loss), C.byref(gnorm)))
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, dt, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert loss.value == float(out[flow.P]) and gnorm.value == float(gn), step
        assert np.isfinite(loss.value)
        assert bool((th[up] == 0.0).all()) and bool((m[up] == 0.0).all()) and bool((v[up] == 0.0).all()), step
    assert not torch.equal(th, flow.theta)
    ctx_a.close()
    ctx_b.close()


# ---- 8. rand --------------------------------------------------------------------------------------------------------------------------
@F64
@pytest.mark.parametrize("shape", [(5, 70), (70, 40)], ids=lambda s: f"d{s[0]}-N{s[1]}")
def test_rand_is_the_forward_of_the_base_draws(nf, shape, f64):
    d, n, theta, x, flow, _ = case(nf, shape, f64)
    ys = nf.rand(flow, n, nf.PhiloxRNG(9))
    xs = nf.device_specific_rand(nf.PhiloxRNG(9), flow.dist, n, dtype=tdt(f64))
    y, _ = nf.with_logabsdet_jacobian(flow.transform, xs)
    torch.cuda.synchronize()
    assert bits(ys) == bits(y) and np.isfinite(host(ys)).all()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
@F64
def test_refusals_raise(nf, f64):
    d, n, theta, x, flow, xs = case(nf, (5, 70), f64)
    with pytest.raises(nf.NFHipError):
        nf.loglikelihood(None, flow, xs)
    with pytest.raises(nf.NFHipError):
        nf.loglikelihood_value_and_gradient(flow, xs)
    with pytest.raises(nf.NFHipError):
        nf.create_flow([flow, nf.planarflow(nf.MvNormal(d), 2, paramtype=tdt(f64))], nf.MvNormal(d))
    with pytest.raises(nf.NFHipError):
        nf.train_flow(nf.loglikelihood, flow, xs, max_iters=1)


# ---- a general base goes through the wrappers ------------------------------------------------------------------------------------
@F64
def test_general_base_goes_through_the_existing_wrappers(nf, f64):
    d, n, theta, x, _, _ = case(nf, (5, 70), f64)
    rng = np.random.default_rng(12)
    bm, bv = fc.rounded(0.3 * rng.standard_normal(d), f64), fc.rounded(rng.uniform(0.5, 1.5, d), f64)
    flow = nf.fullrank(nf.MvNormal(vec(bm, f64), vec(bv, f64)), paramtype=tdt(f64))
    flow.theta = vec(theta, f64)
    tgt, ref = device_target(nf, "mvnormal", d, f64)
    xg = fc.rounded(bm[:, None] + np.sqrt(bv)[:, None] * x, f64)
    loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xg, f64))
    # the reference: the standard-base loss plus mean(log q0(x) - log N(x; 0, I)); the gradient does not see the base
    l_std, g_ref = fr.neg_elbo_value_and_grad(theta, xg, ref)
    logq = -0.5 * (d * fr.L2PI + np.log(bv).sum()) - 0.5 * (((xg - bm[:, None]) ** 2) / bv[:, None]).sum(0)
    l_ref = l_std + (logq - fr.std_normal_logpdf(xg)).mean()
    P.scalar(f"fullrank diagonal base {tag(f64)}: loss", loss, l_ref, P.F64_RTOL if f64 else P.LOSS_RTOL)
    P.gradient(f"fullrank diagonal base {tag(f64)}: gradient", grad, g_ref, P.F64_GRAD if f64 else P.GRAD_RTOL)


# ---- 10. training, with the reference's own criteria (test/interface.jl:27-50) -------------------------------------------------
@F64
def test_training_recovers_a_dense_gaussian(nf, f64):
    d = 4
    m = np.array([3.0, -2.0, 1.0, 0.5])
    A = 0.5 * np.random.default_rng(3).standard_normal((d, d))
    Sigma = A @ A.T + np.eye(d)
    tgt = nf.MvNormalTarget(vec(m, f64), vec(Sigma, f64))
    flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64))
    before = nf.elbo_batch(nf.PhiloxRNG(99), flow, tgt, 4096)
    trained, stats, _ = nf.train_flow(nf.elbo_batch, flow, tgt, 64, max_iters=3000, optimiser=nf.Adam(0.01))
    after = nf.elbo_batch(nf.PhiloxRNG(99), trained, tgt, 4096)
    mu, L = fr.split(host(trained.theta), d)
    err_mu, err_L = np.abs(mu - m).max(), np.abs(L - np.linalg.cholesky(Sigma)).max()
    print(f"fullrank training {tag(f64)}: |mu - m| {err_mu:.3f} |L - chol| {err_L:.3f} elbo {before:.3f} -> {after:.4f}")
    P.record(f"fullrank training {tag(f64)}: max |mu - m|", err_mu)
    P.record(f"fullrank training {tag(f64)}: max |L - chol Sigma|", err_L)
    P.record(f"fullrank training {tag(f64)}: elbo after", after)
    assert len(stats) == 3000 and all(np.isfinite(s["loss"]) for s in stats)
    assert err_mu <= 0.2 and err_L <= 0.2
    assert after > before and after > -1.0
    up = fc.upper_mask(d)
    assert (host(trained.theta)[up] == 0.0).all()  # Adam left the upper triangle where it was
