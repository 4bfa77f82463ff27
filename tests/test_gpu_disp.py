"""GPU tests of the GLM targets with a learned dispersion (NF_TARGET_DGLM_NORMAL / STUDENT / NEGBIN; DispersionGLMTarget and the
constructors over it): nf_target_logp (flat kernel, both element types), the cross-check of the NORMAL kind against the shipped
hierarchical kernels at a pinned lambda, the exact drop of a zero-weight row, RealNVP / NSF / full-rank / preconditioned flows and
a composition (the tiled MFMA kernel; the flat one on the Float64 and the composition path), nf_elbo_step, the closure route,
determinism and a linear mixed model end to end.

Reference values are the numpy closed forms of tests/disp_forms.py evaluated on the target's own `A` and `p0` (test_disp_cpu.py
holds them to direct float64 evaluations); whole-flow references compose them with oracle.nf_oracle as neg_elbo_value_and_grad
does.  Tolerances are tests/parity.py's plain ones; every Float32 check passes `floor=`: the same form evaluated op by op in
numpy float32.

Inputs (disp_forms.arrays): hier_forms' row data over the coefficients (every fifth weight 0), counts up to max k with a larger
count on a zero-weight row, the three hyper-prior forms on lambda in turn; y standard normal.  No test feeds an out-of-range
index or table length: the kernels' bounds are a property of the code, to be read rather than provoked."""
import ctypes as C

import numpy as np
import pytest

import disp_forms as df
import fullrank_ref as fr
import hier_forms as hf
import nf_oracle as o
import parity as P
import precond_ref as pr
from __graft_entry__ import load_package
from test_gpu_glm import agree, comp_neg_elbo, device_logp
from test_gpu_hier import INIT_SCALE, ONE_LINPRED_LAUNCH, check_value_and_gradient
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, new_ctx, prof_counts, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOG_SCALE_MAX = 4.0  # a condition on the inputs: exp(-2 tau), exp(+-lambda) <= 3e3, no single sample carries the loss


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def make_disp(nf, family, d, G, rows, f64, seed=5, maxk=18, disp=None):
    tgt = df.build(nf, family, d, G, rows, tdt(f64), "cuda", seed, maxk, disp)
    return tgt, df.ref_of(tgt)


# ---- 1. nf_target_logp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", df.SHAPES, ids=lambda s: "d%d_G%d" % s)
@pytest.mark.parametrize("family", df.FAMILIES)
def test_target_logp(nf, family, shape, f64):
    """value and score at rows = 1, 33, 133 and N = 1, 37; (33, 0) puts lambda alone in the third 16-lane round; the three
    hyper-prior forms on lambda in turn over the rows; the value is the same whether or not the score is asked for (check_logp)"""
    d, G = shape
    seen = set()
    for rows in df.ROWS:
        tgt, ref = make_disp(nf, family, d, G, rows, f64)
        seen.add(tgt.disp_hyper)
        if family == "negbin":
            assert tgt.table_len == 17  # the zero-weight row's larger count did not lengthen it
        for n in df.NS:
            check_logp(nf, f"disp logp {family} d={d} G={G} rows={rows} N={n} {tag(f64)}", tgt, ref, df.sample_ys(d, n, f64), f64)
    assert seen == set(df.HYPERS)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("maxk", df.MAXK[:-1])
def test_negbin_short_tables(nf, maxk, f64):
    """max k = 0 and 1: an empty table; max k = 2: one entry (18, more entries than the summing threads, is test_target_logp's)"""
    d, G, rows = 5, 2, 33
    tgt, ref = make_disp(nf, "negbin", d, G, rows, f64, maxk=maxk)
    assert tgt.table_len == max(maxk - 1, 0)
    check_logp(nf, f"disp logp negbin maxk={maxk} {tag(f64)}", tgt, ref, df.sample_ys(d, 37, f64), f64)


# ---- 2. a pinned lambda is the hierarchical NORMAL kind --------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_pinned_lambda_reproduces_the_hierarchical_kernels(nf, f64):
    """ys[d - 1, :] = lambda0: the NORMAL kind's value and its (beta, tau)-score are those of HierarchicalGLMTarget("normal") built from
    A exp(-lambda0), off exp(-lambda0), plus what the host folded for lambda: lin[d - 1] lambda0 + h_G(lambda0 - hm_G) + its normaliser"""
    d, G, rows, n, lam0 = 5, 2, 33, 37, 0.75
    a = df.arrays("normal", d, G, rows)
    disp = df.from_arrays(nf, "normal", a, G, tdt(f64), "cuda")
    dv = lambda v: torch.tensor(np.asarray(v), dtype=tdt(f64), device="cuda")
    s = np.exp(-lam0)
    hier = nf.HierarchicalGLMTarget("normal", dv(a["A"] * s), torch.tensor(a["grp"], device="cuda"), G, dv(a["off"] * s), dv(a["wt"]), dv(a["lin"]),
                                    const=0.7, fixed_sigma=a["sig"].tolist(), hyper=a["hyper"], hyper_loc=a["loc"].tolist(),
                                    hyper_scale=a["scl"].tolist())
    q = df.split_p0(df.target_arrays(disp)[1], d, rows, G, False)
    qh = hf.split_p0(hf.target_arrays(hier)[1], d - 1, rows, G)
    extra = q["lin"][d - 1] * lam0 + hf.hyper(int(q["hk"][G]), np.array([lam0 - q["hm"][G]]), q["his"][G])[0][0] + (q["par"][1] - qh["par"][1])
    ys = df.sample_ys(d, n, f64)
    ys[d - 1] = np.float32(lam0)
    got = device_logp(nf, disp, ys, f64)
    want = device_logp(nf, hier, ys[:d - 1], f64)
    href = hf.ref_of(hier)
    r64, r32 = href(ys[:d - 1]), href(ys[:d - 1].astype(np.float32))
    agree(f"disp normal at a pinned lambda vs hier {tag(f64)}", (got[0], got[1][:d - 1]), (want[0] + extra, want[1]), f64,
          (r64[0] + extra, r64[1]), (r32[0] + np.float32(extra), r32[1]))


# ---- 3. a zero-weight row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_zero_weight_row_with_a_huge_predictor_and_count_is_dropped_exactly(nf, f64):
    """a NEGBIN row whose predictor is 1e4 + x . beta and whose count is 4000 under weight 0: value and score (d lambda and the table
    included) are those of the target without the row -- exactly in Float64 -- through nf_target_logp and, in Float32, through a
    flow's tiled kernel"""
    d, G, rows, n = 5, 2, 33, 37
    a = df.arrays("negbin", d, G, rows)
    b = dict(a, A=np.vstack([a["A"], np.ones((1, d - G - 1))]), off=np.append(a["off"], 1e4), wt=np.append(a["wt"], 0.0), cnt=np.append(a["cnt"], 4000))
    plain, masked = df.from_arrays(nf, "negbin", a, G, tdt(f64), "cuda"), df.from_arrays(nf, "negbin", b, G, tdt(f64), "cuda")
    assert plain.table_len == masked.table_len == 17
    ref = df.ref_of(plain)
    ys = df.sample_ys(d, n, f64)
    got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    if f64:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        return
    agree("disp zero-weight huge row f32", got, want, False, ref(ys), ref(ys.astype(np.float32)))
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    flow = flow.with_theta(flow.theta * 0.3)
    xs = to_dev(o.base_sample(d, 48, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    P.scalar("disp zero-weight huge row f32, tiled: loss", l1, l2)
    P.gradient("disp zero-weight huge row f32, tiled: grad", g1, g2)


# ---- 4. through flows ------------------------------------------------------------------------------------------------------------
FLOW_CASES = {
    # name: (kind, d, G, hdims, nblocks, K, B, f64, family, rows)
    "realnvp_d5_negbin": ("realnvp", 5, 2, (32, 32), 2, 0, 0.0, False, "negbin", 33),
    "nsf_d6_student": ("nsf", 6, 2, (32, 32), 2, 8, 5.0, False, "student", 33),
    "realnvp_d40_normal": ("realnvp", 40, 3, (64, 64), 2, 0, 0.0, False, "normal", 133),          # two accumulator blocks
    "realnvp_d70_wide_negbin": ("realnvp", 70, 4, (128, 100), 2, 0, 0.0, False, "negbin", 133),   # a weight-streaming shape
    "realnvp_d150_wide_student": ("realnvp", 150, 8, (128, 100), 2, 0, 0.0, False, "student", 133),  # two feature chunks per row block
    "realnvp_d5_f64_negbin": ("realnvp", 5, 2, (32, 32), 2, 0, 0.0, True, "negbin", 33),          # flat kernel, Float64 coupling path
}
N_FLOW = 48


def flow_case_inputs(name):
    """(spec, theta) of a case: the oracle's initialiser scaled by test_gpu_hier's INIT_SCALE (no GPU: the input bound is checked on the CPU)"""
    kind, d, G, hd, nl, K, B, f64, family, rows = FLOW_CASES[name]
    spec = o.FlowSpec(kind, d, nl, hd, K, B)
    th = INIT_SCALE * o.init_params(spec, np.random.default_rng(3))
    if not f64:
        th = th.astype(np.float32).astype(np.float64)
    return spec, th


def make_flow_case(nf, name):
    kind, d, G, hd, nl, K, B, f64, family, rows = FLOW_CASES[name]
    spec, th = flow_case_inputs(name)
    flow = nf.Flow(kind, nf.MvNormal(d), nl, hd, K, B, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))
    tgt, ref = make_disp(nf, family, d, G, rows, f64)
    return spec, th, flow, tgt, ref, f64


def assert_log_scales_bounded(key, ys, p):
    worst = float(np.abs(ys[p:]).max())
    print(f"{key}: max |tau|, |lambda| over the oracle's ys {worst:.2f}")
    assert worst <= LOG_SCALE_MAX, (key, worst)


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_coupling_flow(nf, name):
    """value_and_gradient(elbo_batch, flow, target, xs) at N = 48 (a ragged second tile) against the composed oracle; exactly one
    "target_linpred" launch and no "target" launch"""
    spec, th, flow, tgt, ref, f64 = make_flow_case(nf, name)
    xs = o.base_sample(spec.d, N_FLOW, 77, 0, 0)
    assert_log_scales_bounded(name, o.flow_fwd(spec, th, xs)[0], tgt.p)
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    l32, g32 = (None, None) if f64 else composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
    check_value_and_gradient(nf, f"disp flow {name} N={N_FLOW}", flow, tgt, xs, f64, l_ref, g_ref, l32, g32)


def fullrank_theta(d):
    rng = np.random.default_rng(6)
    L = np.tril(0.1 * rng.standard_normal((d, d)) / np.sqrt(d), -1) + np.diag(rng.uniform(0.4, 0.7, d))
    return fr.join(0.3 * rng.standard_normal(d), L).astype(np.float32).astype(np.float64)


def test_value_and_gradient_through_a_fullrank_flow(nf):
    """fullrank d = 33, G = 0 (lambda alone in the second 32-feature block), student family"""
    d, G, rows = 33, 0, 33
    th = fullrank_theta(d)
    flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
    flow.theta = torch.tensor(th, dtype=torch.float32, device="cuda")
    tgt, ref = make_disp(nf, "student", d, G, rows, False)
    xs = o.base_sample(d, N_FLOW, 77, 0, 0)
    assert_log_scales_bounded("fullrank_d33_student", fr.fwd(th, xs)[0], tgt.p)
    l_ref, g_ref = fr.neg_elbo_value_and_grad(th, xs, ref)
    l32, g32 = fr.neg_elbo_value_and_grad(th.astype(np.float32), xs.astype(np.float32), ref)
    check_value_and_gradient(nf, f"disp flow fullrank_d33_student N={N_FLOW}", flow, tgt, xs, False, l_ref, g_ref, l32, g32)


def precond_inputs(d=6):
    spec = o.FlowSpec("realnvp", d, 2, (32, 32))
    th = np.concatenate([fullrank_theta(d), (INIT_SCALE * o.init_params(spec, np.random.default_rng(3))).astype(np.float32).astype(np.float64)])
    return spec, th


def test_value_and_gradient_through_a_preconditioned_flow(nf):
    """preconditioned(realnvp) d = 6 on a negative-binomial target"""
    d, G = 6, 2
    spec, th = precond_inputs(d)
    flow = nf.preconditioned(nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32))
    assert flow.P == th.size
    flow = flow.with_theta(torch.tensor(th, dtype=torch.float32, device="cuda"))
    tgt, ref = make_disp(nf, "negbin", d, G, 33, False)
    xs = o.base_sample(d, N_FLOW, 77, 0, 0)
    assert_log_scales_bounded("preconditioned_d6_negbin", pr.fwd(spec, th, xs)[0], tgt.p)
    l_ref, g_ref = pr.neg_elbo_value_and_grad(spec, th, xs, ref)
    l32, g32 = pr.neg_elbo_value_and_grad(spec, th.astype(np.float32), xs.astype(np.float32), ref)
    check_value_and_gradient(nf, f"disp flow preconditioned realnvp d6 negbin N={N_FLOW}", flow, tgt, xs, False, l_ref, g_ref, l32, g32)


def composition_inputs(d=6):
    rng = np.random.default_rng(4)
    specs = [o.FlowSpec("planar", d, 3, ()), o.FlowSpec("realnvp", d, 2, (32, 32))]
    ths = [(INIT_SCALE * o.init_params(sp, rng)).astype(np.float32).astype(np.float64) for sp in specs]
    return specs, ths


def test_value_and_gradient_through_a_composition(nf):
    """create_flow((planar, realnvp), q0) on a NORMAL target: the composition's generic sequence launches the target kernel once"""
    d, G = 6, 2
    specs, ths = composition_inputs(d)
    th = np.concatenate(ths)
    q0 = nf.MvNormal(d)
    segs = [nf.Flow(sp.kind, q0, sp.nlayers, sp.hdims, dtype=torch.float32, device="cuda", theta=torch.tensor(t, dtype=torch.float32, device="cuda"))
            for sp, t in zip(specs, ths)]
    flow = nf.create_flow(segs, q0)
    tgt, ref = make_disp(nf, "normal", d, G, 33, False)
    xs = o.base_sample(d, N_FLOW, 77, 0, 0)
    assert_log_scales_bounded("composition", o.comp_fwd(specs, th, xs)[0], tgt.p)
    l_ref, g_ref = comp_neg_elbo(specs, th, ref, xs)
    l32, g32 = comp_neg_elbo(specs, P.f32(th), ref, P.f32(xs))
    check_value_and_gradient(nf, f"disp flow composition planar+realnvp d6 normal N={N_FLOW}", flow, tgt, xs, False, l_ref, g_ref, l32, g32)


# ---- 5. the step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["realnvp_d5_negbin", "nsf_d6_student"])
def test_elbo_step_equals_the_split_calls_and_the_graph_form_refuses(nf, name):
    """two consecutive nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit;
    nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED and leaves theta, the moments and the counter alone."""
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
def closure_inputs(nf=None):
    d, nl = 4, 10
    spec = o.FlowSpec("planar", d, nl)
    return d, nl, spec


def test_planar_float64_takes_the_closure_route(nf):
    d, nl, spec = closure_inputs()
    G, n = 1, 37
    flow = nf.planarflow(nf.MvNormal(d), nl, paramtype=torch.float64, seed=3)
    flow = flow.with_theta(flow.theta * 0.3)
    tgt, ref = make_disp(nf, "negbin", d, G, 33, True)
    xs = o.base_sample(d, n, 77, 0, 0)
    th = flow.theta.cpu().numpy()
    assert_log_scales_bounded("planar closure route", o.flow_fwd(spec, th, xs)[0], tgt.p)
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, True)))
    assert counts == ONE_LINPRED_LAUNCH, counts  # the device score, through the target's autograd node
    P.scalar("disp closure route planar d4x10 f64 negbin: loss", loss, l_ref, P.F64_RTOL)
    P.gradient("disp closure route planar d4x10 f64 negbin: grad", g, g_ref, P.F64_GRAD)


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["realnvp_d40_normal", "realnvp_d5_negbin"])
def test_the_tiled_kernel_is_bitwise_reproducible(nf, name):
    """the same value_and_gradient call twice: d = 40 / rows = 133 (two accumulator blocks; every wave takes row blocks, phi and
    d phi / d lambda combined in wave order) and NEGBIN at max k = 18 (the table's partials combined q = 0 .. 7)"""
    spec, _, flow, tgt, _, _ = make_flow_case(nf, name)
    xs = to_dev(o.base_sample(spec.d, 97, 77, 0, 0), False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e1 = nf.batched_elbos(flow, tgt, xs).clone()
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e2 = nf.batched_elbos(flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------
def test_linear_mixed_model_trains(nf):
    """y ~ x + (1 | level) on 40 synthetic rows in 5 levels; z = [b (2) ; a (5) ; tau ; lambda], d = 9.  train_flow on a RealNVP at
    256 draws: the ELBO on a fixed 4096-draw stream rises and every loss is finite."""
    rng = np.random.default_rng(11)
    rows, L = 40, 5
    X = np.concatenate([np.ones((rows, 1)), rng.standard_normal((rows, 1))], 1)
    lev = np.arange(rows) % L
    y = X @ np.array([0.5, -1.2]) + 0.8 * rng.standard_normal(L)[lev] + 0.4 * rng.standard_normal(rows)
    dv = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    tgt = nf.LinearMixedModelTarget(dv(X), dv(y), torch.tensor(lev, device="cuda"), L, fixed_sigma=5.0, hyper="halfcauchy", hyper_scale=1.0,
                                    disp_hyper="halfcauchy", disp_scale=1.0)
    assert tgt.d == 9 and tgt.p == 7 and tgt.G == 1
    flow = nf.realnvp(nf.MvNormal(9), (32, 32), 2, paramtype=torch.float32, seed=4)
    flow = flow.with_theta(flow.theta * 0.3)
    before = nf.elbo_batch(nf.PhiloxRNG(99), flow, tgt, 4096)
    trained, stats, _ = nf.train_flow(nf.PhiloxRNG(7), nf.elbo_batch, flow, tgt, 256, max_iters=300, optimiser=nf.Adam(5e-3))
    after = nf.elbo_batch(nf.PhiloxRNG(99), trained, tgt, 4096)
    print(f"linear mixed model: elbo {before:.3f} -> {after:.3f}")
    P.record("disp linear mixed model: elbo after", after)
    assert len(stats) == 300 and all(np.isfinite(a["loss"]) for a in stats)
    assert np.isfinite(before) and after > before
