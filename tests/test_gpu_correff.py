"""GPU tests of the correlated-random-effects targets (NF_TARGET_CRE_*, CorrelatedEffectsTarget) against tests/correff_forms.py's
definition (torch.distributions + autograd in float64; the same formula in float32 as the floor), composed with oracle.nf_oracle /
tests/fullrank_ref.py for flows, at tests/parity.py's tolerances through test_gpu_linpred.py's criterion."""
import ctypes as C

import numpy as np
import pytest

import correff_forms as cf
import fullrank_ref as fr
import nf_oracle as o
import parity as P
from test_gpu_linpred import B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, new_ctx, nf, sample_ys, tdt, to_dev, vp  # noqa: F401 (nf: the module fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGP_CASES = [(g, f) for g in "ac" for f in ("logit", "poisson", "dnormal", "dstudent")] + [("b", "normal"), ("d", "normal")]


def make(nf, geo, family, f64):
    c = cf.case(geo, family, f64)
    return c, cf.build(nf, c, tdt(f64), "cuda"), cf.ref_of(c)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("geo,family", LOGP_CASES)
def test_target_logp(nf, geo, family, f64):
    c, tgt, ref = make(nf, geo, family, f64)
    for n in (1, 37):
        check_logp(nf, f"correff logp {geo} {family} d={tgt.d} N={n} {'f64' if f64 else 'f32'}", tgt, ref, sample_ys(tgt.d, n, f64), f64)


@pytest.mark.parametrize("disp", [False, True], ids=["hier", "disp"])
def test_every_k_one_is_the_hierarchical_kind(nf, disp):
    """two varying intercepts (G = 5, 4): value and score of the Float64 flat kernels agree with HierarchicalGLMTarget /
    DispersionGLMTarget on the same rows, groups and hyper-priors (y permuted: the existing kinds keep every tau behind every b)"""
    rng = np.random.default_rng(4)
    rows, p, G = 33, 3, (5, 4)
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, device="cuda")
    A, off, wt, lin = rng.standard_normal((rows, 12)) / 3.0, 0.5 * rng.standard_normal(rows), rng.uniform(0.3, 2.5, rows), 0.5 * rng.standard_normal(12)
    wt[[4, 20]] = 0.0
    hyp, loc, scl, sig = ["halfcauchy", "lognormal"], [0.25, -0.5], [1.25, 0.75], [np.inf, 0.75, 1.5]  # (float32-exact: the existing wrappers pass lists through float32)
    terms = [(1, G[i], 1.0, hyp[i], loc[i], scl[i]) for i in range(2)]
    grp = torch.tensor([-1] * 3 + [0] * 5 + [1] * 4, device="cuda")
    if disp:
        new = nf.CorrelatedEffectsTarget("dstudent", t(A), terms, t(off), t(wt), t(lin), 0.7, 3.0, sig, "halfnormal", 0.0, 1.25)
        old = nf.DispersionGLMTarget("student", t(A), None, grp, 2, t(off), t(wt), t(lin), 0.7, 3.0, sig + [1.0] * 9, hyp, loc, scl, "halfnormal", 0.0, 1.25)
    else:
        new = nf.CorrelatedEffectsTarget("poisson", t(A), terms, t(off), t(wt), t(lin), 0.7, 0.0, sig)
        old = nf.HierarchicalGLMTarget("poisson", t(A), grp, 2, t(off), t(wt), t(lin), 0.7, 0.0, sig + [1.0] * 9, hyp, loc, scl)
    perm = list(range(8)) + list(range(9, 13)) + [8, 13] + ([14] if disp else [])  # old coordinate -> new coordinate
    assert new.d == old.d == len(perm)
    ys = sample_ys(new.d, 37, True)
    lp_n, sc_n = nf.target_logp(new, to_dev(ys, True), with_grad=True)
    lp_o, sc_o = nf.target_logp(old, to_dev(ys[perm], True), with_grad=True)
    P.elementwise(f"correff k=1 vs {'dglm' if disp else 'hglm'}: logp", lp_n, lp_o, P.F64_RTOL, 1e-12)
    P.elementwise(f"correff k=1 vs {'dglm' if disp else 'hglm'}: score", sc_n[perm], sc_o, P.F64_RTOL, 1e-12)


FLOW_CASES = {"realnvp_a": ("realnvp", "a", "dnormal"), "realnvp_c": ("realnvp", "c", "logit"), "fullrank_d": ("fullrank", "d", "normal")}


def make_flow_case(nf, name):  # -> (flow, target, oracle(theta, xs) -> (loss, grad), theta)
    kind, geo, family = FLOW_CASES[name]
    c, tgt, ref = make(nf, geo, family, False)
    d = tgt.d
    if kind == "fullrank":
        rng = np.random.default_rng(3 + d)
        th = P.f32(fr.join(0.3 * rng.standard_normal(d), np.eye(d) + 0.2 * np.tril(rng.standard_normal((d, d))) / np.sqrt(d))).astype(np.float64)
        flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32).with_theta(torch.tensor(th, dtype=torch.float32, device="cuda"))
        return flow, tgt, (lambda t, x: fr.neg_elbo_value_and_grad(t, x, ref)), th
    spec = o.FlowSpec(kind, d, 2, (32, 32))
    th = P.f32(o.init_params(spec, np.random.default_rng(3))).astype(np.float64)
    flow = nf.Flow(kind, nf.MvNormal(d), 2, (32, 32), 0, 0.0, dtype=torch.float32, device="cuda", theta=torch.tensor(th, dtype=torch.float32, device="cuda"))
    return flow, tgt, (lambda t, x: composed_neg_elbo(spec, t, ref, x)), th


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_flow(nf, name):
    """64 draws through the tiled kernel against the composed oracle"""
    flow, tgt, oracle, th = make_flow_case(nf, name)
    key, xs = f"correff flow {name} N=64", o.base_sample(tgt.d, 64, 77, 0, 0)
    l_ref, g_ref = oracle(th, xs)
    loss, g = nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, False))
    assert np.isfinite(l_ref) and np.isfinite(g_ref).all()
    l32, g32 = oracle(P.f32(th), P.f32(xs))
    print(f"{key}: loss {loss} ref {l_ref} f32 {l32}; grad err {np.abs(g.cpu().numpy() - g_ref).max():.3e} floor {np.abs(g32 - g_ref).max():.3e} of {np.abs(g_ref).max():.3e}")
    P.scalar(key + ": loss", loss, l_ref, floor=l32)
    P.gradient(key + ": grad", g, g_ref, floor=g32)


def test_elbo_step_equals_the_split_calls_and_the_other_routes_refuse(nf):
    """two nf_elbo_step calls == value-and-grad + Adam on a second context, bit for bit; two launches give equal bits; the graph form,
    the row minibatch, a planar flow and the non-centring layer refuse and touch nothing"""
    lib = nf.load_library()
    flow, tgt = make_flow_case(nf, "realnvp_a")[:2]
    n, seed = 97, 77
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    planar = nf.planarflow(nf.MvNormal(tgt.d), 4, paramtype=torch.float32, seed=1)
    pth, pm, pv = planar.theta.clone(), torch.zeros_like(planar.theta), torch.zeros_like(planar.theta)
    pcode = lib.nf_elbo_step(ctx_a.ptr, C.byref(planar.desc), C.byref(tgt.c), vp(pth), vp(pm), vp(pv), 16, 1, 0, LR, B1, B2, EPS, None, None)
    p0o, Ao, out = torch.full_like(tgt.p0, 7.0), torch.full_like(tgt.A, 7.0), nf._lib.Target()
    mcode = lib.nf_target_minibatch(ctx_a.ptr, 0, C.byref(tgt.c), tgt.d, tgt.p0.numel(), 32, 1, 0, None, None, vp(p0o), vp(Ao), C.byref(out))
    torch.cuda.synchronize()
    assert code == pcode == mcode == NF_ERR_UNSUPPORTED and torch.equal(th, flow.theta) and int(counter[0]) == 0
    assert torch.equal(pth, planar.theta) and not bool(pm.any()) and not bool(pv.any()) and bool((p0o == 7.0).all()) and bool((Ao == 7.0).all())
    with pytest.raises(nf.NFHipError, match="noncentred"):
        nf.noncentred(flow, tgt)
    ys = to_dev(sample_ys(tgt.d, 37, False), False)
    (l1, s1), (l2, s2) = nf.target_logp(tgt, ys, with_grad=True), nf.target_logp(tgt, ys, with_grad=True)
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    res, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    for step in range(2):
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS, C.byref(loss), C.byref(gnorm)))
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(res)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(res), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert loss.value == float(res[flow.P]) and gnorm.value == float(gn) and np.isfinite(loss.value) and abs(loss.value) > 0.1
    ctx_a.close(), ctx_b.close()


def test_train_flow_lowers_the_negative_elbo(nf):
    """the Python route end to end: 30 Adam steps on case (a), -ELBO on 2 048 fixed draws before and after (a decrease, nothing more)"""
    tgt = make(nf, "a", "dnormal", False)[1]
    flow = nf.realnvp(nf.MvNormal(tgt.d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(tgt.d, 2048, 5, 0, 0), False)
    before = -float(nf.elbo_batch(flow, tgt, xs))
    trained = nf.train_flow(nf.PhiloxRNG(9), nf.elbo_batch, flow, tgt, 256, max_iters=30, optimiser=nf.Adam(1e-2))[0]
    after = -float(nf.elbo_batch(trained, tgt, xs))
    print(f"correff train_flow: -ELBO {before} -> {after}")
    assert np.isfinite(after) and after < before
