"""GPU tests of the generalised linear-predictor targets (NF_TARGET_GLM_LOGIT / PROBIT / POISSON / STUDENT / NORMAL; GLMTarget and
the regression constructors over it): nf_target_logp (flat kernel, both element types), the tails of every row function, the
cross-checks against the centred kernels, RealNVP / NSF flows (the tiled MFMA kernel; the flat one on the Float64 and the
composition path), nf_elbo_step, the refusals, the closure route, train_flow and determinism.

Reference values are the numpy closed forms of tests/glm_forms.py evaluated on the target's own `A` and `p0` (scipy's log_ndtr
in float64); whole-flow references compose them with oracle.nf_oracle as neg_elbo_value_and_grad does.  Tolerances are
tests/parity.py's; every Float32 check passes `floor=`: the same form evaluated op by op in numpy float32.

Inputs: A standard normal / sqrt(d), offsets 0.5 randn, weights uniform in [0.3, 2.5] with every fifth row's weight 0 (rows > 1),
lin 0.5 randn, a constant, prior sigma 2, nu = 3 for the Student family."""
import ctypes as C

import numpy as np
import pytest

import glm_forms as gf
import nf_oracle as o
import parity as P
from __graft_entry__ import load_package
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, make_gauss, make_logreg, new_ctx, prof_counts,
                              sample_ys, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ONE_LINPRED_LAUNCH = {"target_linpred": 1, "target": 0}


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def dev(a, f64):
    return torch.tensor(np.asarray(a), dtype=tdt(f64), device="cuda")


def glm_arrays(family, d, rows, seed=5):
    """the random row data of one target, float64"""
    rng = np.random.default_rng(seed + 7 * d + rows + 131 * gf.FAMILIES.index(family))
    A = rng.standard_normal((rows, d)) / np.sqrt(d)
    off = 0.5 * rng.standard_normal(rows)
    wt = rng.uniform(0.3, 2.5, rows)
    if rows > 1:
        wt[2::5] = 0.0
    lin = 0.5 * rng.standard_normal(d)
    return A, off, wt, lin


def build_glm(nf, family, f64, A, off, wt, lin, const=0.7, prior_sigma=2.0):
    tgt = nf.GLMTarget(family, dev(A, f64), None if off is None else dev(off, f64), None if wt is None else dev(wt, f64),
                       None if lin is None else dev(lin, f64), const=const, param=3.0 if family == "student" else 0.0, prior_sigma=prior_sigma)
    return tgt, gf.ref_of(tgt)


def make_glm(nf, family, d, rows, f64, seed=5):
    return build_glm(nf, family, f64, *glm_arrays(family, d, rows, seed))


def device_logp(nf, tgt, ys, f64):
    lp, sc = nf.target_logp(tgt, to_dev(ys, f64), with_grad=True)
    torch.cuda.synchronize()
    return lp.double().cpu().numpy(), sc.double().cpu().numpy()


# ---- 1. nf_target_logp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [2, 5, 64])
@pytest.mark.parametrize("family", gf.FAMILIES)
def test_target_logp(nf, family, d, f64):
    """value and score at rows = 1, 33 (one row past a 16- and a 32-row block), 133 (several passes, ragged tail) and N = 1, 37;
    the value is the same whether or not the score is asked for (check_logp)"""
    for rows in (1, 33, 133):
        tgt, ref = make_glm(nf, family, d, rows, f64)
        for n in (1, 37):
            check_logp(nf, f"glm logp {family} d={d} rows={rows} N={n} {tag(f64)}", tgt, ref, sample_ys(d, n, f64), f64)


# ---- 2. tails ------------------------------------------------------------------------------------------------------------------
TAILS = {"probit": (-30.0, 30.0), "logit": (-40.0, 40.0), "poisson": (-30.0, 8.0), "student": (-1e3, 1e3)}


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", list(TAILS))
def test_tails_stay_finite_and_accurate(nf, family, f64):
    """the predictors A y + off mapped affinely onto [lo, hi] (A scaled, one common offset): both ends are reached"""
    d, rows, n = 5, 33, 37
    lo, hi = TAILS[family]
    ys = sample_ys(d, n, f64)
    A, _, wt, lin = glm_arrays(family, d, rows)
    r = A @ ys
    s = (hi - lo) / (r.max() - r.min())
    tgt, ref = build_glm(nf, family, f64, s * A, np.full(rows, lo - s * r.min()), wt, lin)
    Ad, p0 = gf.target_arrays(tgt)
    u = Ad @ ys + gf.split_p0(p0, d, rows)[1][:, None]
    assert abs(u.min() - lo) <= 1e-3 * abs(lo) and abs(u.max() - hi) <= 1e-3 * abs(hi), (u.min(), u.max())
    check_logp(nf, f"glm tails {family} u in [{lo:g}, {hi:g}] {tag(f64)}", tgt, ref, ys, f64)


# ---- 3. cross-checks between kernels ---------------------------------------------------------------------------------------------
def agree(key, got, want, f64, ref64=None, ref32=None):
    """two device results: 1e-10 in Float64; in Float32 the first against the float64 closed form of the second, with its floor"""
    for name, g, w, r64, r32 in zip(("logp", "score"), got, want, ref64 or (None, None), ref32 or (None, None)):
        assert np.isfinite(g).all(), (key, name)
        if f64:
            P.elementwise(f"{key}: {name}", g, w, P.F64_RTOL, 1e-12)
        else:
            P.elementwise(f"{key}: {name}", g, r64, floor=r32)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_normal_family_reproduces_the_dense_gaussian(nf, f64):
    """NORMAL with A = W, off = -W mu, unit weights, a flat prior and const = -d/2 log(2 pi) + log|det W| is MvNormal(mu, Sigma)"""
    d, n = 5, 37
    mv, mv_ref, _ = make_gauss(nf, d, f64)
    W, mu = mv.W.double().cpu().numpy(), mv.mu.double().cpu().numpy()
    tgt, _ = build_glm(nf, "normal", f64, W, -W @ mu, None, None, const=-0.5 * d * gf.L2PI + mv.logdet_w, prior_sigma=np.inf)
    ys = sample_ys(d, n, f64)
    agree(f"glm normal vs densegauss {tag(f64)}", device_logp(nf, tgt, ys, f64), device_logp(nf, mv, ys, f64), f64, mv_ref(ys),
          mv_ref(ys.astype(np.float32)))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_logit_family_reproduces_logistic_regression(nf, f64):
    d, rows, n = 5, 33, 37
    lr, lr_ref = make_logreg(nf, d, rows, f64)
    tgt = nf.GLMTarget("logit", lr.A, prior_sigma=2.0)
    ys = sample_ys(d, n, f64)
    agree(f"glm logit vs logreg {tag(f64)}", device_logp(nf, tgt, ys, f64), device_logp(nf, lr, ys, f64), f64, lr_ref(ys),
          lr_ref(ys.astype(np.float32)))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_a_row_of_weight_two_is_the_row_written_twice(nf, f64):
    d, rows, n = 5, 33, 37
    A, off, wt, lin = glm_arrays("probit", d, rows)
    wt[3] = 2.0
    once, _ = build_glm(nf, "probit", f64, A, off, wt, lin)
    wt2 = np.append(wt, 1.0)
    wt2[3] = 1.0
    twice, ref2 = build_glm(nf, "probit", f64, np.vstack([A, A[3:4]]), np.append(off, off[3]), wt2, lin)
    ys = sample_ys(d, n, f64)
    agree(f"glm weight 2 vs the row twice {tag(f64)}", device_logp(nf, once, ys, f64), device_logp(nf, twice, ys, f64), f64, ref2(ys),
          ref2(ys.astype(np.float32)))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_zero_weight_row_with_an_overflowing_predictor_is_dropped_exactly(nf, f64):
    """a POISSON row whose predictor is 1e4 + x . y (exp overflows in either element type) under weight 0: value and score are those
    of the target without the row -- exactly in Float64 -- through nf_target_logp and, in Float32, through a flow's tiled kernel"""
    d, rows, n = 5, 33, 37
    A, off, wt, lin = glm_arrays("poisson", d, rows)
    plain, ref = build_glm(nf, "poisson", f64, A, off, wt, lin)
    masked, _ = build_glm(nf, "poisson", f64, np.vstack([A, np.ones((1, d))]), np.append(off, 1e4), np.append(wt, 0.0), lin)
    ys = sample_ys(d, n, f64)
    got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    if f64:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        return
    agree("glm zero-weight overflowing row f32", got, want, False, ref(ys), ref(ys.astype(np.float32)))
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(d, 48, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    P.scalar("glm zero-weight overflowing row f32, tiled: loss", l1, l2)
    P.gradient("glm zero-weight overflowing row f32, tiled: grad", g1, g2)


# ---- 4. through flows ------------------------------------------------------------------------------------------------------------
FLOW_CASES = {
    # name: (kind, d, hdims, nblocks, K, B, f64, family, rows)
    "realnvp_d5_poisson": ("realnvp", 5, (32, 32), 2, 0, 0.0, False, "poisson", 33),
    "nsf_d6_probit": ("nsf", 6, (32, 32), 2, 8, 5.0, False, "probit", 33),
    "realnvp_d40_student": ("realnvp", 40, (64, 64), 2, 0, 0.0, False, "student", 133),       # G over two accumulator blocks
    "realnvp_d70_wide_normal": ("realnvp", 70, (128, 100), 2, 0, 0.0, False, "normal", 133),  # a weight-streaming shape
    "realnvp_d5_f64_logit": ("realnvp", 5, (32, 32), 2, 0, 0.0, True, "logit", 33),           # flat kernel, Float64 coupling path
    "realnvp_d150_wide_probit": ("realnvp", 150, (128, 100), 2, 0, 0.0, False, "probit", 133),  # two feature chunks per row block
}
N_FLOW = 48


def make_flow_case(nf, name):
    kind, d, hd, nl, K, B, f64, family, rows = FLOW_CASES[name]
    spec = o.FlowSpec(kind, d, nl, hd, K, B)
    th = o.init_params(spec, np.random.default_rng(3))
    if not f64:
        th = th.astype(np.float32).astype(np.float64)
    flow = nf.Flow(kind, nf.MvNormal(d), nl, hd, K, B, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))
    tgt, ref = make_glm(nf, family, d, rows, f64)
    return spec, th, flow, tgt, ref, f64


def check_value_and_gradient(nf, key, flow, tgt, xs, f64, l_ref, g_ref, l32=None, g32=None):
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)))
    assert counts == ONE_LINPRED_LAUNCH, counts
    print(f"{key}: loss {loss!r} oracle {l_ref!r}; grad err / |g|inf {np.abs(g.double().cpu().numpy() - g_ref).max() / np.abs(g_ref).max():.3e}")
    assert np.isfinite(l_ref) and np.isfinite(g_ref).all()
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        P.record(key + ": loss, float32 oracle [rel err]", abs(float(l32) - l_ref) / abs(l_ref))
        P.scalar(key + ": loss", loss, l_ref)
        P.gradient(key + ": grad", g, g_ref, floor=g32)


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_coupling_flow(nf, name):
    """value_and_gradient(elbo_batch, flow, target, xs) at N = 48 (a ragged second tile) against the composed oracle; exactly one
    "target_linpred" launch and no "target" launch"""
    spec, th, flow, tgt, ref, f64 = make_flow_case(nf, name)
    xs = o.base_sample(spec.d, N_FLOW, 77, 0, 0)
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    l32, g32 = (None, None) if f64 else composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
    check_value_and_gradient(nf, f"glm flow {name} N={N_FLOW}", flow, tgt, xs, f64, l_ref, g_ref, l32, g32)


def comp_neg_elbo(specs, theta, ref, xs):
    """oracle.comp_neg_elbo_value_and_grad with the target's closed form"""
    n = xs.shape[1]
    sl = o._comp_slices(specs)
    ys, ladj, inputs = o.comp_fwd(specs, theta, xs, keep=True)
    lp, sc = ref(ys)
    loss = -(lp - o.std_normal_logpdf(xs) + ladj).mean()
    gbar = (-sc / n).astype(xs.dtype)
    lbar = np.full(n, -1.0 / n, dtype=xs.dtype)
    grad = np.zeros_like(theta)
    for s in range(len(specs)):
        th = theta[sl[s][0]:sl[s][1]]
        _, _, states = o.flow_fwd(specs[s], th, inputs[s], keep=True)
        gbar, g = o.flow_bwd(specs[s], th, states, gbar, lbar)
        grad[sl[s][0]:sl[s][1]] = g
    return loss, grad


def test_value_and_gradient_through_a_composition(nf):
    """create_flow((planar, realnvp), q0) on a Poisson target: the composition's generic sequence launches the target kernel once"""
    d = 6
    rng = np.random.default_rng(4)
    specs = [o.FlowSpec("planar", d, 3, ()), o.FlowSpec("realnvp", d, 2, (32, 32))]
    ths = [(0.3 * o.init_params(specs[0], rng)).astype(np.float32).astype(np.float64), o.init_params(specs[1], rng).astype(np.float32).astype(np.float64)]
    th = np.concatenate(ths)
    q0 = nf.MvNormal(d)
    segs = [nf.Flow(sp.kind, q0, sp.nlayers, sp.hdims, dtype=torch.float32, device="cuda", theta=torch.tensor(t, dtype=torch.float32, device="cuda"))
            for sp, t in zip(specs, ths)]
    flow = nf.create_flow(segs, q0)
    tgt, ref = make_glm(nf, "poisson", d, 33, False)
    xs = o.base_sample(d, N_FLOW, 77, 0, 0)
    l_ref, g_ref = comp_neg_elbo(specs, th, ref, xs)
    l32, g32 = comp_neg_elbo(specs, P.f32(th), ref, P.f32(xs))
    check_value_and_gradient(nf, f"glm flow composition planar+realnvp d6 poisson N={N_FLOW}", flow, tgt, xs, False, l_ref, g_ref, l32, g32)


# ---- 5. the step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["realnvp_d5_poisson", "nsf_d6_probit"])
def test_elbo_step_equals_the_split_calls_and_the_graph_form_refuses(nf, name):
    """two consecutive nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit;
    nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED and leaves theta and the counter alone."""
    lib = nf.load_library()
    _, _, flow, tgt, _, _ = make_flow_case(nf, name)
    n, seed = 97, 77
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert code == NF_ERR_UNSUPPORTED and torch.equal(th, flow.theta) and int(counter[0]) == 0
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    for step in range(2):
        loss, gnorm = C.c_double(0), C.c_double(0)
        _, counts = prof_counts(nf, ctx_a, lambda: nf._lib.check(lib.nf_elbo_step(
            ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS, C.byref(loss), C.byref(gnorm))))
        assert counts == ONE_LINPRED_LAUNCH, counts
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert loss.value == float(out[flow.P]) and gnorm.value == float(gn), (step, loss.value, float(out[flow.P]), gnorm.value, float(gn))
        assert np.isfinite(loss.value) and abs(loss.value) > 0.1
    assert not torch.equal(th, flow.theta)
    ctx_a.close()
    ctx_b.close()


# ---- 6. refusals and the closure route ---------------------------------------------------------------------------------------------
def test_flows_with_in_kernel_targets_refuse_and_touch_nothing(nf):
    lib = nf.load_library()
    ctx = new_ctx(nf)
    cases = [(nf.planarflow(nf.MvNormal(3), 4, paramtype=torch.float32, seed=1), False, "poisson"),
             (nf.radialflow(nf.MvNormal(3), 4, paramtype=torch.float32, seed=1), False, "probit"),
             (nf.meanfield(nf.MvNormal(3), paramtype=torch.float64), True, "student")]
    for flow, f64, family in cases:
        tgt = make_glm(nf, family, 3, 7, f64)[0]
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        out = torch.full((flow.P + 1,), 7.0, dtype=tdt(f64), device="cuda")
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        val = C.c_double(123.0)
        xs = to_dev(o.base_sample(3, 16, 5, 0, 0), f64)
        assert lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), None, 16, 16, 1, 0, 0, vp(out)) == NF_ERR_UNSUPPORTED
        assert lib.nf_elbo_batch(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(xs), 16, None, C.byref(val)) == NF_ERR_UNSUPPORTED
        assert lib.nf_elbo_batch_rng(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), 16, 1, 0, 0, C.byref(val)) == NF_ERR_UNSUPPORTED
        assert lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), 16, 1, 0, LR, B1, B2, EPS, None, None) == NF_ERR_UNSUPPORTED
        assert lib.nf_elbo_step_enqueue(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), 16, 1, vp(counter), LR, B1, B2, EPS,
                                        None) == NF_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert val.value == 123.0 and bool((out == 7.0).all()) and torch.equal(th, flow.theta) and not bool(m.any()) and not bool(v.any())
        assert int(counter[0]) == 0
    ctx.close()


def test_planar_float64_on_a_poisson_target_takes_the_closure_route(nf):
    d, nl, n = 2, 10, 37
    flow = nf.planarflow(nf.MvNormal(d), nl, paramtype=torch.float64, seed=3)
    flow = flow.with_theta(flow.theta * 0.3)
    rng = np.random.default_rng(8)
    X = rng.standard_normal((33, d)) / np.sqrt(d)
    tgt = nf.PoissonRegressionTarget(dev(X, True), dev(rng.poisson(2.0, 33), True), exposure=dev(rng.uniform(0.5, 2.0, 33), True),
                                     weights=dev(np.where(np.arange(33) % 5 == 2, 0.0, rng.uniform(0.3, 2.5, 33)), True), prior_sigma=2.0)
    ref = gf.ref_of(tgt)
    xs = o.base_sample(d, n, 77, 0, 0)
    spec, th = o.FlowSpec("planar", d, nl), flow.theta.cpu().numpy()
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, True)))
    assert counts == ONE_LINPRED_LAUNCH, counts  # the device score, through the target's autograd node
    P.scalar("glm closure route planar d2x10 f64 poisson: loss", loss, l_ref, P.F64_RTOL)
    P.gradient("glm closure route planar d2x10 f64 poisson: grad", g, g_ref, P.F64_GRAD)


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------
def test_train_flow_on_poisson_regression_equals_the_split_loop(nf):
    """train_flow(elbo_batch, realnvp, PoissonRegressionTarget, 64), five iterations, runs nf_elbo_step per iteration: theta, the
    Adam state and the recorded losses are those of `optimize` over value_and_gradient + update bit for bit."""
    from normalizingflows_jl_amd import objectives as ob

    d, rows, n = 5, 33, 64
    rng = np.random.default_rng(12)
    X = rng.standard_normal((rows, d)) / np.sqrt(d)
    tgt = nf.PoissonRegressionTarget(dev(X, False), dev(rng.poisson(2.0, rows), False), exposure=dev(rng.uniform(0.5, 2.0, rows), False))
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(9), None, {})
    fa, sa, sta = nf.train_flow(nf.PhiloxRNG(9), nf.elbo_batch, flow, tgt, n, max_iters=5, optimiser=nf.Adam(2e-3))
    theta0, re = flow.destructure()
    rng_b = nf.PhiloxRNG(9)
    tb, sb, stb = nf.optimize(lambda th: nf.value_and_gradient(nf.elbo_batch, re(th), tgt, n, rng_b), theta0, re, max_iters=5,
                              optimiser=nf.Adam(2e-3))
    assert torch.equal(fa.theta, tb) and torch.equal(sta.m, stb.m) and torch.equal(sta.v, stb.v) and sta.t == stb.t == 5
    assert not torch.equal(fa.theta, flow.theta)
    print("glm train_flow losses", [a["loss"] for a in sa], "split loop", [b["loss"] for b in sb])
    assert [a["loss"] for a in sa] == [b["loss"] for b in sb] and len(sa) == 5 and all(np.isfinite(a["loss"]) for a in sa)


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------------
def test_the_tiled_kernel_is_bitwise_reproducible(nf):
    """the same value_and_gradient call twice (d = 40: two accumulator blocks; rows = 133: every wave takes row blocks, combined
    in wave order)"""
    _, _, flow, tgt, _, _ = make_flow_case(nf, "realnvp_d40_student")
    xs = to_dev(o.base_sample(40, 97, 77, 0, 0), False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e1 = nf.batched_elbos(flow, tgt, xs).clone()
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e2 = nf.batched_elbos(flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)
