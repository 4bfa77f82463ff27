"""GPU tests of the distributional regression targets (NF_TARGET_DR_*, DistributionalRegressionTarget) against tests/distreg_forms.py's
numpy form on the target's own buffers (composed with oracle.nf_oracle / tests/fullrank_ref.py for flows), at tests/parity.py's tolerances
through test_gpu_glm.py's criterion (check_logp; Float32 checks pass `floor=`).  Every target is distreg_forms.make_target's: 166 rows."""
import ctypes as C

import numpy as np
import pytest

import distreg_forms as df
import fullrank_ref as fr
import nf_oracle as o
import parity as P
from test_gpu_glm import device_logp, nf, tag  # noqa: F401 (nf: the module fixture)
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, new_ctx, prof_counts, sample_ys, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROF = ("target_distreg", "target_linpred", "target")
ONE_LAUNCH = {"target_distreg": 1, "target_linpred": 0, "target": 0}
DP = [(5, 2), (40, 33), (100, 1), (150, 75)]  # one block | p odd, block 32-63 holds both parts | DB = 4, a one-column X | DB = 8, two chunks, p inside one


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("d,p", DP)
@pytest.mark.parametrize("family", df.FAMILIES)
def test_target_logp(nf, family, d, p, f64):
    tgt = df.make_target(nf, family, d, p, tdt(f64), "cuda")
    for n in (1, 37):
        check_logp(nf, f"distreg logp {family} d={d} p={p} N={n} {tag(f64)}", tgt, df.ref_of(tgt), sample_ys(d, n, f64), f64)


FLOW_CASES = {  # name: (kind, d, p, hdims, f64, family)
    "realnvp_d5": ("realnvp", 5, 2, (32, 32), False, "normal"),
    "realnvp_d40": ("realnvp", 40, 33, (64, 64), False, "student"),          # the straddling block
    "realnvp_d150_wide": ("realnvp", 150, 75, (128, 100), False, "zipoisson"),  # two feature chunks per row block
    "realnvp_d5_f64": ("realnvp", 5, 2, (32, 32), True, "weibull"),          # the flat kernel
    "fullrank_d5": ("fullrank", 5, 2, (), False, "zipoisson"),
}
N_FLOW = 48


def make_flow_case(nf, name):  # -> (flow, target, oracle(theta, xs) -> (loss, grad), theta, f64)
    kind, d, p, hd, f64, family = FLOW_CASES[name]
    tgt = df.make_target(nf, family, d, p, tdt(f64), "cuda")
    ref = df.ref_of(tgt)
    if kind == "fullrank":
        rng = np.random.default_rng(3 + d)
        th = P.f32(fr.join(0.3 * rng.standard_normal(d), np.eye(d) + 0.2 * np.tril(rng.standard_normal((d, d))) / np.sqrt(d))).astype(np.float64)
        flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64)).with_theta(torch.tensor(th, dtype=tdt(f64), device="cuda"))
        return flow, tgt, (lambda t, x: fr.neg_elbo_value_and_grad(t, x, ref)), th, f64
    spec = o.FlowSpec(kind, d, 2, hd)
    th = P.f32(o.init_params(spec, np.random.default_rng(3))).astype(np.float64)  # float32-representable in either element type
    flow = nf.Flow(kind, nf.MvNormal(d), 2, hd, 0, 0.0, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))
    return flow, tgt, (lambda t, x: composed_neg_elbo(spec, t, ref, x)), th, f64


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_flow(nf, name):
    """N = 48 (a ragged second tile) against the composed oracle; exactly one "target_distreg" launch and no "target" launch"""
    flow, tgt, oracle, th, f64 = make_flow_case(nf, name)
    key, xs = f"distreg flow {name} N={N_FLOW}", o.base_sample(tgt.d, N_FLOW, 77, 0, 0)
    l_ref, g_ref = oracle(th, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)), PROF)
    assert counts == ONE_LAUNCH and np.isfinite(l_ref) and np.isfinite(g_ref).all(), counts
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        P.scalar(key + ": loss", loss, l_ref)
        P.gradient(key + ": grad", g, g_ref, floor=oracle(P.f32(th), P.f32(xs))[1])


# shifts of (offu, offv), applied with alternating signs so that all four sign pairs occur: the predictors sit in both tails of both
# arguments.  At these sizes the float64 form AND its float32 floor are finite at every y below (Weibull's u exp(v) reaches 66 of
# float32's 88, the Poisson rate exp(24)); the test asserts that before it asks the device.
TAILS = {"normal": (30.0, 8.0), "student": (30.0, 8.0), "zipoisson": (20.0, 20.0), "weibull": (3.0, 1.5)}


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", df.FAMILIES)
def test_both_tails_of_both_predictors_stay_finite_and_accurate(nf, family, f64):
    d, p, n = 5, 2, 37
    tgt = df.make_target(nf, family, d, p, tdt(f64), "cuda", shift=TAILS[family])
    ref, ys = df.ref_of(tgt), sample_ys(d, n, f64)
    u, v = df.predictors(ys, *df.target_arrays(tgt), p)
    su, sv = TAILS[family]
    assert u.max() > 0.8 * su and u.min() < -0.8 * su and v.max() > 0.8 * sv and v.min() < -0.8 * sv
    for y in (ys, ys.astype(np.float32)):
        assert all(np.isfinite(a).all() for a in ref(y)), (family, y.dtype)
    check_logp(nf, f"distreg tails {family} u+-{su:g} v+-{sv:g} {tag(f64)}", tgt, ref, ys, f64)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", df.FAMILIES)
def test_a_weight_zero_row_of_huge_features_contributes_exactly_nothing(nf, family, f64):
    """one more row of weight 0 with 1e30 features gives the bits of the target without it: the flat kernel in both element types, the
    tiled one through a Float32 flow (d = 40, p = 33: the row sits in both parts of the straddling block)"""
    d, p, n = 40, 33, 37
    base = df.case_arrays(d, rows=95)
    more = [np.vstack([base[0], np.full((1, d), 1e30)])] + [np.append(a, 0.0) for a in base[1:4]] + [np.append(base[4], 1.0), base[5]]
    plain, masked = (df.make_target(nf, family, d, p, tdt(f64), "cuda", arrays=a) for a in (base, more))
    assert masked.rows == plain.rows + 1 == 96 and float(masked.A[95, 0]) > 9e29 and float(masked.p0[3 * 96 - 1]) == 0.0
    ys = sample_ys(d, n, f64)
    got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.abs(want[1]).max() > 0.1 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if not f64:
        flow = nf.realnvp(nf.MvNormal(d), (64, 64), 2, paramtype=torch.float32, seed=2)
        xs = to_dev(o.base_sample(d, N_FLOW, 77, 0, 0), False)
        (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
        assert np.isfinite(l1) and l1 == l2 and torch.equal(g1, g2)


def test_elbo_step_equals_the_split_calls_and_the_other_routes_refuse(nf):
    """two nf_elbo_step calls == value-and-grad + Adam on a second context, bit for bit; the other routes refuse and touch nothing"""
    lib = nf.load_library()
    flow, tgt = make_flow_case(nf, "realnvp_d5")[:2]
    n, seed = 97, 77
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    planar = nf.planarflow(nf.MvNormal(5), 4, paramtype=torch.float32, seed=1)
    pth, pm, pv = planar.theta.clone(), torch.zeros_like(planar.theta), torch.zeros_like(planar.theta)
    pcode = lib.nf_elbo_step(ctx_a.ptr, C.byref(planar.desc), C.byref(tgt.c), vp(pth), vp(pm), vp(pv), 16, 1, 0, LR, B1, B2, EPS, None, None)
    p0o, Ao, out = torch.full_like(tgt.p0, 7.0), torch.full_like(tgt.A, 7.0), nf._lib.Target()
    mcode = lib.nf_target_minibatch(ctx_a.ptr, 0, C.byref(tgt.c), tgt.d, tgt.p0.numel(), 32, 1, 0, None, None, vp(p0o), vp(Ao), C.byref(out))
    torch.cuda.synchronize()
    assert code == pcode == mcode == NF_ERR_UNSUPPORTED and torch.equal(th, flow.theta) and int(counter[0]) == 0
    assert torch.equal(pth, planar.theta) and not bool(pm.any()) and not bool(pv.any()) and bool((p0o == 7.0).all()) and bool((Ao == 7.0).all())
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


def test_the_tiled_kernel_is_bitwise_reproducible(nf):
    """the same value_and_gradient call twice (d = 40: two accumulator blocks, one of them fed by both parts; six row blocks over four waves)"""
    flow, tgt = make_flow_case(nf, "realnvp_d40")[:2]
    xs = to_dev(o.base_sample(40, 97, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs), nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(nf.batched_elbos(flow, tgt, xs).clone(), nf.batched_elbos(flow, tgt, xs))
