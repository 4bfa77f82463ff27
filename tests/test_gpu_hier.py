"""GPU tests of the hierarchical GLM targets (NF_TARGET_HGLM_LOGIT / PROBIT / POISSON / STUDENT / NORMAL; HierarchicalGLMTarget and
VaryingInterceptTarget): nf_target_logp (flat kernel, both element types), the cross-check against the GLM kernels at G = 0,
the exact drop of a zero-weight row, RealNVP / NSF / full-rank flows and a composition (the tiled MFMA kernel; the flat one on the
Float64 and the composition path), nf_elbo_step, the closure route, determinism and eight schools end to end.

Reference values are the numpy closed forms of tests/hier_forms.py evaluated on the target's own `A` and `p0`; whole-flow references
compose them with oracle.nf_oracle as neg_elbo_value_and_grad does.  Tolerances are tests/parity.py's; every Float32 check passes
`floor=`: the same form evaluated op by op in numpy float32.

Inputs (hier_forms.arrays): test_gpu_glm.glm_arrays' row data over the coefficients (every fifth weight 0), grp random in
{-1 .. G-1} with the last group left without a member, one flat coefficient, the three hyper-prior forms in turn; y standard normal.
No test feeds an out-of-range index: the kernels' bounds are a property of the code, to be read rather than provoked."""
import ctypes as C

import numpy as np
import pytest

import fullrank_ref as fr
import glm_forms as gf
import hier_forms as hf
import nf_oracle as o
import parity as P
from __graft_entry__ import load_package
from test_gpu_glm import agree, build_glm, comp_neg_elbo, device_logp, glm_arrays
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, new_ctx, prof_counts, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ONE_LINPRED_LAUNCH = {"target_linpred": 1, "target": 0}
TAU_MAX = 4.0  # exp(-2 tau) <= 3e3: no single sample carries the loss


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def make_hier(nf, family, d, G, rows, f64, seed=5):
    tgt = hf.build(nf, family, d, G, rows, tdt(f64), "cuda", seed)
    return tgt, hf.ref_of(tgt)


# ---- 1. nf_target_logp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", hf.SHAPES, ids=lambda s: "d%d_G%d" % s)
@pytest.mark.parametrize("family", hf.FAMILIES)
def test_target_logp(nf, family, shape, f64):
    """value and score at rows = 1, 33, 133 and N = 1, 37; (35, 2) puts the log-scales in another 32-feature block and another
    16-lane round than their members; the value is the same whether or not the score is asked for (check_logp)"""
    d, G = shape
    for rows in hf.ROWS:
        tgt, ref = make_hier(nf, family, d, G, rows, f64)
        q = hf.split_p0(hf.target_arrays(tgt)[1], d, rows, G)
        if G >= 2:
            assert q["gptr"][G] == q["gptr"][G - 1], "the last group has no member"
        if d - G > 1:
            assert q["isd"][0] == 0.0 and (q["grp"] < 0).any()
        for n in hf.NS:
            check_logp(nf, f"hier logp {family} d={d} G={G} rows={rows} N={n} {tag(f64)}", tgt, ref, hf.sample_ys(d, n, f64), f64)
    if G == 8:
        assert set(tgt.hyper) == set(hf.HYPERS)


# ---- 2. G = 0 is the GLM target ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("sigma", [2.0, np.inf], ids=["sigma2", "flat"])
def test_no_group_reproduces_the_glm_kernels(nf, sigma, f64):
    d, rows, n = 5, 33, 37
    A, off, wt, lin = glm_arrays("probit", d, rows)
    glm, ref = build_glm(nf, "probit", f64, A, off, wt, lin, prior_sigma=sigma)
    dv = lambda a: torch.tensor(np.asarray(a), dtype=tdt(f64), device="cuda")
    hier = nf.HierarchicalGLMTarget("probit", dv(A), torch.full((d,), -1, device="cuda"), 0, dv(off), dv(wt), dv(lin), const=0.7, fixed_sigma=sigma)
    assert hier.d == d and hier.G == 0
    ys = hf.sample_ys(d, n, f64)
    agree(f"hier G=0 vs glm sigma={sigma} {tag(f64)}", device_logp(nf, hier, ys, f64), device_logp(nf, glm, ys, f64), f64, ref(ys),
          ref(ys.astype(np.float32)))


# ---- 3. a zero-weight row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_zero_weight_row_with_an_overflowing_predictor_is_dropped_exactly(nf, f64):
    """a POISSON row whose predictor is 1e4 + x . beta under weight 0: value and score are those of the target without the row --
    exactly in Float64 -- through nf_target_logp and, in Float32, through a flow's tiled kernel"""
    d, G, rows, n = 5, 2, 33, 37
    a = hf.arrays("poisson", d, G, rows)
    dv = lambda v: torch.tensor(np.asarray(v), dtype=tdt(f64), device="cuda")

    def mk(A, off, wt):
        return nf.HierarchicalGLMTarget("poisson", dv(A), torch.tensor(a["grp"], device="cuda"), G, dv(off), dv(wt), dv(a["lin"]), const=0.7,
                                        fixed_sigma=a["sig"].tolist(), hyper=a["hyper"], hyper_loc=a["loc"].tolist(), hyper_scale=a["scl"].tolist())

    plain = mk(a["A"], a["off"], a["wt"])
    masked = mk(np.vstack([a["A"], np.ones((1, d - G))]), np.append(a["off"], 1e4), np.append(a["wt"], 0.0))
    ref = hf.ref_of(plain)
    ys = hf.sample_ys(d, n, f64)
    got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    if f64:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        return
    agree("hier zero-weight overflowing row f32", got, want, False, ref(ys), ref(ys.astype(np.float32)))
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    flow = flow.with_theta(flow.theta * 0.3)
    xs = to_dev(o.base_sample(d, 48, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    P.scalar("hier zero-weight overflowing row f32, tiled: loss", l1, l2)
    P.gradient("hier zero-weight overflowing row f32, tiled: grad", g1, g2)


# ---- 4. through flows ------------------------------------------------------------------------------------------------------------
FLOW_CASES = {
    # name: (kind, d, G, hdims, nblocks, K, B, f64, family, rows)
    "realnvp_d5_poisson": ("realnvp", 5, 2, (32, 32), 2, 0, 0.0, False, "poisson", 33),
    "nsf_d6_probit": ("nsf", 6, 2, (32, 32), 2, 8, 5.0, False, "probit", 33),
    "realnvp_d40_student": ("realnvp", 40, 3, (64, 64), 2, 0, 0.0, False, "student", 133),        # two accumulator blocks
    "realnvp_d70_wide_normal": ("realnvp", 70, 4, (128, 100), 2, 0, 0.0, False, "normal", 133),   # a weight-streaming shape
    "realnvp_d150_wide_probit": ("realnvp", 150, 8, (128, 100), 2, 0, 0.0, False, "probit", 133),  # two feature chunks per row block
    "realnvp_d5_f64_logit": ("realnvp", 5, 2, (32, 32), 2, 0, 0.0, True, "logit", 33),            # flat kernel, Float64 coupling path
}
N_FLOW = 48
INIT_SCALE = 0.3  # of o.init_params(spec, default_rng(3)): as drawn, tau reaches -14 at these shapes; scaled, it stays within +-3.6


def make_flow_case(nf, name):
    kind, d, G, hd, nl, K, B, f64, family, rows = FLOW_CASES[name]
    spec = o.FlowSpec(kind, d, nl, hd, K, B)
    th = INIT_SCALE * o.init_params(spec, np.random.default_rng(3))
    if not f64:
        th = th.astype(np.float32).astype(np.float64)
    flow = nf.Flow(kind, nf.MvNormal(d), nl, hd, K, B, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))
    tgt, ref = make_hier(nf, family, d, G, rows, f64)
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


def assert_tau_bounded(key, ys, p):
    worst = float(np.abs(ys[p:]).max())
    print(f"{key}: max |tau| over the oracle's ys {worst:.2f}")
    assert worst <= TAU_MAX, (key, worst)


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_coupling_flow(nf, name):
    """value_and_gradient(elbo_batch, flow, target, xs) at N = 48 (a ragged second tile) against the composed oracle; exactly one
    "target_linpred" launch and no "target" launch"""
    spec, th, flow, tgt, ref, f64 = make_flow_case(nf, name)
    xs = o.base_sample(spec.d, N_FLOW, 77, 0, 0)
    assert_tau_bounded(name, o.flow_fwd(spec, th, xs)[0], tgt.p)
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    l32, g32 = (None, None) if f64 else composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
    check_value_and_gradient(nf, f"hier flow {name} N={N_FLOW}", flow, tgt, xs, f64, l_ref, g_ref, l32, g32)


def test_value_and_gradient_through_a_fullrank_flow(nf):
    """fullrank d = 33 (the log-scales in the second 32-feature block), logit family"""
    d, G, rows = 33, 2, 33
    rng = np.random.default_rng(6)
    L = np.tril(0.1 * rng.standard_normal((d, d)) / np.sqrt(d), -1) + np.diag(rng.uniform(0.4, 0.7, d))
    th = fr.join(0.3 * rng.standard_normal(d), L).astype(np.float32).astype(np.float64)
    flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
    flow.theta = torch.tensor(th, dtype=torch.float32, device="cuda")
    tgt, ref = make_hier(nf, "logit", d, G, rows, False)
    xs = o.base_sample(d, N_FLOW, 77, 0, 0)
    assert_tau_bounded("fullrank_d33_logit", fr.fwd(th, xs)[0], tgt.p)
    l_ref, g_ref = fr.neg_elbo_value_and_grad(th, xs, ref)
    l32, g32 = fr.neg_elbo_value_and_grad(th.astype(np.float32), xs.astype(np.float32), ref)
    check_value_and_gradient(nf, f"hier flow fullrank_d33_logit N={N_FLOW}", flow, tgt, xs, False, l_ref, g_ref, l32, g32)


def test_value_and_gradient_through_a_composition(nf):
    """create_flow((planar, realnvp), q0) on a Poisson target: the composition's generic sequence launches the target kernel once"""
    d, G = 6, 2
    rng = np.random.default_rng(4)
    specs = [o.FlowSpec("planar", d, 3, ()), o.FlowSpec("realnvp", d, 2, (32, 32))]
    ths = [(INIT_SCALE * o.init_params(sp, rng)).astype(np.float32).astype(np.float64) for sp in specs]
    th = np.concatenate(ths)
    q0 = nf.MvNormal(d)
    segs = [nf.Flow(sp.kind, q0, sp.nlayers, sp.hdims, dtype=torch.float32, device="cuda", theta=torch.tensor(t, dtype=torch.float32, device="cuda"))
            for sp, t in zip(specs, ths)]
    flow = nf.create_flow(segs, q0)
    tgt, ref = make_hier(nf, "poisson", d, G, 33, False)
    xs = o.base_sample(d, N_FLOW, 77, 0, 0)
    assert_tau_bounded("composition", o.comp_fwd(specs, th, xs)[0], tgt.p)
    l_ref, g_ref = comp_neg_elbo(specs, th, ref, xs)
    l32, g32 = comp_neg_elbo(specs, P.f32(th), ref, P.f32(xs))
    check_value_and_gradient(nf, f"hier flow composition planar+realnvp d6 poisson N={N_FLOW}", flow, tgt, xs, False, l_ref, g_ref, l32, g32)


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
    assert not bool(m.any()) and not bool(v.any())
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


# ---- 6. the closure route ----------------------------------------------------------------------------------------------------------
def test_planar_float64_takes_the_closure_route(nf):
    d, G, nl, n = 3, 1, 10, 37
    flow = nf.planarflow(nf.MvNormal(d), nl, paramtype=torch.float64, seed=3)
    flow = flow.with_theta(flow.theta * 0.3)
    tgt, ref = make_hier(nf, "poisson", d, G, 33, True)
    xs = o.base_sample(d, n, 77, 0, 0)
    spec, th = o.FlowSpec("planar", d, nl), flow.theta.cpu().numpy()
    assert_tau_bounded("planar closure route", o.flow_fwd(spec, th, xs)[0], tgt.p)
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, True)))
    assert counts == ONE_LINPRED_LAUNCH, counts  # the device score, through the target's autograd node
    P.scalar("hier closure route planar d3x10 f64 poisson: loss", loss, l_ref, P.F64_RTOL)
    P.gradient("hier closure route planar d3x10 f64 poisson: grad", g, g_ref, P.F64_GRAD)


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------
def test_the_tiled_kernel_is_bitwise_reproducible(nf):
    """the same value_and_gradient call twice (d = 40: two accumulator blocks; rows = 133: every wave takes row blocks, combined
    in wave order; the prior's sums have one owner each)"""
    _, _, flow, tgt, _, _ = make_flow_case(nf, "realnvp_d40_student")
    xs = to_dev(o.base_sample(40, 97, 77, 0, 0), False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e1 = nf.batched_elbos(flow, tgt, xs).clone()
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e2 = nf.batched_elbos(flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------
def test_eight_schools_trains(nf):
    """Rubin's eight schools, centred: y_j ~ N(mu + eta_j, s_j^2), mu ~ N(0, 5^2), eta_j ~ N(0, exp(tau)^2), exp(tau) ~ half-Cauchy(5);
    z = [mu ; eta (8) ; tau], d = 10.  train_flow on a RealNVP at 256 draws: the ELBO on a fixed 4096-draw stream rises."""
    y = np.array([28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0])
    s = np.array([15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0])
    dv = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    A = np.concatenate([np.ones((8, 1)), np.eye(8)], 1) / s[:, None]
    const = float((-0.5 * np.log(2.0 * np.pi) - np.log(s)).sum())
    tgt = nf.HierarchicalGLMTarget("normal", dv(A), torch.tensor([-1] + [0] * 8, device="cuda"), 1, offset=dv(-y / s), const=const,
                                   fixed_sigma=5.0, hyper="halfcauchy", hyper_scale=5.0)
    assert tgt.d == 10 and tgt.p == 9 and tgt.G == 1
    flow = nf.realnvp(nf.MvNormal(10), (32, 32), 2, paramtype=torch.float32, seed=4)
    flow = flow.with_theta(flow.theta * 0.3)
    before = nf.elbo_batch(nf.PhiloxRNG(99), flow, tgt, 4096)
    trained, stats, _ = nf.train_flow(nf.PhiloxRNG(7), nf.elbo_batch, flow, tgt, 256, max_iters=300, optimiser=nf.Adam(5e-3))
    after = nf.elbo_batch(nf.PhiloxRNG(99), trained, tgt, 4096)
    print(f"eight schools: elbo {before:.3f} -> {after:.3f}")
    P.record("hier eight schools: elbo after", after)
    assert len(stats) == 300 and all(np.isfinite(a["loss"]) for a in stats)
    assert np.isfinite(before) and after > before
