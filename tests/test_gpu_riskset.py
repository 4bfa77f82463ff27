"""GPU tests of the risk-set regression target (NF_TARGET_RISKSET; RiskSetTarget, CoxRegressionTarget, ConditionalLogitTarget):
nf_target_logp (flat kernel, both element types) and the tiled MFMA kernel (through a Float32 full-rank flow) at every case of
riskset_forms.CASES -- every segment geometry at d = 7 and d = 130, every width at the two geometries that load all waves, R in
{32, 96, 160, 288}, N in {1, 31, 33, 70}, predictors of order 1 and |eta| up to about 60 -- tiled against flat, the weight-0 row,
determinism, RealNVP / NSF / Float64 / full-rank / preconditioned / weight-streaming flows as ELBO users, nf_elbo_step, the
refusals, the closure route and train_flow.

Reference values are tests/riskset_forms.py's float64 DEFINITION (explicit risk sets, one log-sum-exp per event row) evaluated on the
target's own `X` and `p0`; whole-flow references compose it with oracle.nf_oracle (or tests/fullrank_ref.py / tests/precond_ref.py)
as neg_elbo_value_and_grad does.  Tolerances are tests/parity.py's plain ones: log p element-wise at Y_RTOL / Y_ATOL, scores and
gradients by `gradient` at GRAD_RTOL, Float64 at F64_RTOL / F64_GRAD; every Float32 check passes `floor=`: the two recurrences
evaluated op by op in numpy float32 (test_riskset_cpu.py holds that floor to 0.5x of the tolerances on these inputs).

An identity full-rank flow (theta = [0 ; I]) hands its draws to the target unchanged (y = x bit for bit, ladj = 0): that is how the
tiled kernel is evaluated at chosen points y."""
import ctypes as C

import numpy as np
import pytest

import fullrank_ref as fr
import nf_oracle as o
import parity as P
import precond_ref as pr
import riskset_forms as rf
from __graft_entry__ import load_package
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, composed_neg_elbo, new_ctx, prof_counts, tdt, to_dev, vp)
from test_riskset_cpu import TRAIN, fullrank_numpy_losses, train_target

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROF = ("target_riskset", "target_ordinal", "target_bnn", "target_softmax", "target_linpred", "target")
ONE_LAUNCH = {"target_riskset": 1, "target_ordinal": 0, "target_bnn": 0, "target_softmax": 0, "target_linpred": 0, "target": 0}
CASE_IDS = ["%s_d%d" % c for c in rf.CASES]


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def dev(a, f64):
    return torch.tensor(np.asarray(a), dtype=tdt(f64), device="cuda")


def build_riskset(nf, X, seg, m, w, off, lin, f64, **kw):
    kw = {"prior_sigma": rf.SIGMA, **kw}
    tgt = nf.RiskSetTarget(dev(X, f64), seg, m, w, off, lin, **kw)
    return tgt, rf.ref_of(tgt)


_CASES, _REFS = {}, {}


def make_riskset(nf, case, f64):
    """the target of a case and its reference, built once per module and left unchanged"""
    key = (case, f64)
    if key not in _CASES:
        _CASES[key] = build_riskset(nf, *rf.arrays(*case), f64)
    return _CASES[key]


def ref_at(nf, case, n, regime, f64=False):
    """(ys, float64 definition, float32 floor) of a case at N = n on the target's own data (log w is rounded to the element type),
    computed once and shared"""
    key = (case, n, regime, f64)
    if key not in _REFS:
        ref = make_riskset(nf, case, f64)[1]
        ys = rf.sample_ys(case[1], n, regime)
        _REFS[key] = (ys, ref(ys), (None, None) if f64 else ref(ys.astype(np.float32)))
    return _REFS[key]


def device_logp(nf, tgt, ys, f64):
    lp, sc = nf.target_logp(tgt, to_dev(ys, f64), with_grad=True)
    torch.cuda.synchronize()
    return lp.double().cpu().numpy(), sc.double().cpu().numpy()


def compare(key, lp, sc, lr, sr, f64, l32=None, s32=None):
    print(f"{key}: logp err {np.abs(lp - lr).max():.3e} of max |logp| {np.abs(lr).max():.3e}; score err / |s|inf {np.abs(sc - sr).max() / np.abs(sr).max():.3e}")
    assert np.isfinite(lp).all() and np.isfinite(sc).all(), key
    if f64:
        P.elementwise(key + ": logp", lp, lr, P.F64_RTOL, 1e-12)
        P.gradient(key + ": score", sc, sr, P.F64_GRAD)
    else:
        P.elementwise(key + ": logp", lp, lr, floor=l32)
        P.gradient(key + ": score", sc, sr, floor=s32)


def fullrank_flow(nf, d, f64, theta):
    flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64))
    return flow.with_theta(torch.tensor(theta, dtype=tdt(f64), device="cuda"))


def fullrank_theta(d, seed=3):
    """mu = 0.3 randn, L = I + 0.2 tril(randn) / sqrt(d): float32-representable"""
    rng = np.random.default_rng(seed + d)
    L = np.eye(d) + 0.2 * np.tril(rng.standard_normal((d, d))) / np.sqrt(d)
    return fr.join(0.3 * rng.standard_normal(d), L).astype(np.float32).astype(np.float64)


def identity_flow(nf, d):
    return fullrank_flow(nf, d, False, fr.join(np.zeros(d), np.eye(d)))


def tiled_logp_score(nf, tgt, ys):
    """the TILED kernel at the points ys (Float32) -> (log p (N,), mean score (d,)): the per-sample ELBO terms of the identity
    full-rank flow plus log q0, and minus the shift's part of the loss gradient (the mean over the samples of the score)"""
    d, n = ys.shape
    flow = identity_flow(nf, d)
    xs = to_dev(ys, False)
    (e, counts) = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, xs), PROF)
    assert counts == ONE_LAUNCH, counts
    ((_, g), counts) = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs), PROF)
    assert counts == ONE_LAUNCH, counts
    return e.double().cpu().numpy() + o.std_normal_logpdf(ys), -g.double().cpu().numpy()[:d]


# ---- 1. nf_target_logp, and the tiled kernel, at every case ----------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("case", rf.CASES, ids=CASE_IDS)
def test_target_logp(nf, case, f64):
    """value element-wise, score by `gradient`; the value does not depend on whether the score is asked for"""
    tgt, _ = make_riskset(nf, case, f64)
    for n in rf.N_SIZES:
        for regime in rf.REGIMES:
            ys, (lr, sr), (l32, s32) = ref_at(nf, case, n, regime, f64)
            key = f"riskset logp {case} N={n} {regime} {tag(f64)}"
            lp, sc = device_logp(nf, tgt, ys, f64)
            assert np.array_equal(lp, nf.target_logp(tgt, to_dev(ys, f64)).double().cpu().numpy()), key
            compare(key, lp, sc, lr, sr, f64, l32, s32)


@pytest.mark.parametrize("case", rf.CASES, ids=CASE_IDS)
def test_tiled_kernel_at_chosen_points(nf, case):
    """the identity full-rank flow hands the tiled layout to k_target_riskset_tiled AT the flat kernel's points: log p within the
    tolerances of the reference and the mean score against the reference and against the flat kernel's -- one target launch per call"""
    tgt, _ = make_riskset(nf, case, False)
    for n in rf.N_SIZES:
        for regime in rf.REGIMES:
            ys, (lr, sr), (l32y, s32y) = ref_at(nf, case, n, regime)
            lt, st = tiled_logp_score(nf, tgt, ys)
            lf, sf = device_logp(nf, tgt, ys, False)
            kk = f"riskset tiled {case} N={n} {regime}"
            print(f"{kk}: logp err {np.abs(lt - lr).max():.3e} of {np.abs(lr).max():.3e}; mean score err / |s|inf {np.abs(st - sr.mean(1)).max() / np.abs(sr.mean(1)).max():.3e}")
            assert np.isfinite(lt).all() and np.isfinite(st).all(), kk
            P.elementwise(kk + ": logp (tiled)", lt, lr, floor=l32y)
            P.elementwise(kk + ": logp (tiled vs flat)", lt, lf, floor=l32y + (lf - lr))
            P.gradient(kk + ": mean score (tiled)", st, sr.mean(1), floor=s32y.astype(np.float64).mean(1))
            P.gradient(kk + ": mean score (tiled vs flat)", st, sf.mean(1), floor=sf.mean(1) + (s32y.astype(np.float64).mean(1) - sr.mean(1)))


@pytest.mark.parametrize("case", [("one_segment", 33), ("strata_2_to_5", 130), ("dead_block_mid_segment", 7), ("one_segment", 256)],
                         ids=lambda c: "%s_d%d" % c)
def test_tiled_kernel_through_a_fullrank_flow(nf, case):
    """a Float32 full-rank flow away from the identity: per-sample ELBO terms and the whole gradient (the matrix's part is the scores
    times the draws, so every sample's score counts, not their mean)"""
    d = case[1]
    tgt, ref = make_riskset(nf, case, False)
    theta = fullrank_theta(d)
    flow = fullrank_flow(nf, d, False, theta)
    for n in (33, 70):
        key = f"riskset fullrank {case} N={n}"
        xs = o.base_sample(d, n, 77, 0, 0)
        (elbos, counts) = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, to_dev(xs, False)), PROF)
        assert counts == ONE_LAUNCH, counts
        (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, False)), PROF)
        assert counts == ONE_LAUNCH, counts
        e_ref = fr.elbos(theta, xs, ref)
        l_ref, g_ref = fr.neg_elbo_value_and_grad(theta, xs, ref)
        e32 = fr.elbos(P.f32(theta), P.f32(xs), ref)
        l32, g32 = fr.neg_elbo_value_and_grad(P.f32(theta), P.f32(xs), ref)
        print(f"{key}: loss {loss!r} ref {l_ref!r}; elbo err {np.abs(elbos.double().cpu().numpy() - e_ref).max():.3e}; "
              f"grad err / |g|inf {np.abs(g.double().cpu().numpy() - g_ref).max() / np.abs(g_ref).max():.3e}")
        assert np.isfinite(loss) and bool(torch.isfinite(g).all())
        P.elementwise(key + ": elbos", elbos, e_ref, floor=e32)
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": grad", g, g_ref, floor=g32)


def test_limit_is_unsupported_and_nothing_is_written(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx = new_ctx(nf)
    buf, X = torch.zeros(8192, device="cuda"), torch.zeros(8192, device="cuda")
    for dtype in (0, 1):
        for sigma in (2.0, np.inf):
            t = Target(33, buf.data_ptr(), X.data_ptr(), 32.0, sigma)
            assert lib.nf_target_logp(ctx.ptr, dtype, C.byref(t), 257, 2, vp(buf), vp(buf), vp(buf)) == NF_ERR_UNSUPPORTED
        t = Target(33, buf.data_ptr(), X.data_ptr(), 8192.0 + 32.0, 2.0)
        assert lib.nf_target_logp(ctx.ptr, dtype, C.byref(t), 4, 2, vp(buf), vp(buf), vp(buf)) == NF_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(X.any())
    ctx.close()


# ---- 2. definitional checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_zero_weight_rows_of_huge_features_change_no_bit(nf, f64):
    """the rows of risk weight 0 (three that open the first segment, six that open the second, random ones inside) hold 1e30 in X
    and an offset of 50 (their predictors overflow or cancel to NaN): value and score are bit for bit those of the target with the
    plain rows -- through nf_target_logp and, in Float32, through the tiled kernel of a flow"""
    case = ("dead_rows_at_segment_start", 7)
    X, seg, m, w, off, lin = rf.arrays(*case)
    dead = np.nonzero(w == 0)[0]
    Xb, ob = X.copy(), off.copy()
    Xb[dead], ob[dead] = 1e30, 50.0
    plain, _ = build_riskset(nf, X, seg, m, w, off, lin, f64)
    masked, _ = build_riskset(nf, Xb, seg, m, w, ob, lin, f64)
    assert dead.size >= 9 and float(masked.A.abs().max()) > 9e29 and torch.equal(masked.p0[plain.padded_rows:], plain.p0[plain.padded_rows:])
    for regime in rf.REGIMES:
        ys = rf.sample_ys(7, 33, regime)
        got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if f64:
        return
    flow = nf.realnvp(nf.MvNormal(7), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(7, 33, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    e1, e2 = nf.batched_elbos(flow, masked, xs), nf.batched_elbos(flow, plain, xs)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)


def test_two_identical_launches_are_bit_equal(nf):
    """one segment over 288 rows at d = 64: every wave takes blocks in three rounds, carries and G combined in wave order; the flat
    kernel too"""
    case = ("one_segment", 64)
    tgt, _ = make_riskset(nf, case, False)
    flow = nf.realnvp(nf.MvNormal(64), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(64, 33, 77, 0, 0), False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e1 = nf.batched_elbos(flow, tgt, xs).clone()
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e2 = nf.batched_elbos(flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)
    ys = rf.sample_ys(64, 33, "spread")
    for f64 in (False, True):
        t = make_riskset(nf, case, f64)[0]
        a, b = device_logp(nf, t, ys, f64), device_logp(nf, t, ys, f64)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_cox_and_conditional_logit_wrappers_on_the_device(nf, f64):
    """CoxRegressionTarget (ties, strata, weights, offsets) and ConditionalLogitTarget against the definition on their own packing"""
    from test_riskset_cpu import _clogit_data, _cox_data

    X, time, event, strata, wt, off = _cox_data(rows=75, p=5)
    cox = nf.CoxRegressionTarget(dev(X, f64), time, event, strata, wt, off, prior_sigma=rf.SIGMA)
    Xc, cs, chosen, wc = _clogit_data(sets=40, p=5)
    cl = nf.ConditionalLogitTarget(dev(Xc, f64), cs, chosen, wc, prior_sigma=rf.SIGMA)
    ys = rf.sample_ys(5, 33, "unit")
    for name, tgt in (("cox", cox), ("clogit", cl)):
        ref = rf.ref_of(tgt)
        lp, sc = device_logp(nf, tgt, ys, f64)
        l32, s32 = (None, None) if f64 else ref(ys.astype(np.float32))
        compare(f"riskset {name} wrapper {tag(f64)}", lp, sc, *ref(ys), f64, l32, s32)
        if not f64:
            P.elementwise(f"riskset {name} wrapper: logp (tiled)", tiled_logp_score(nf, tgt, ys)[0], ref(ys)[0], floor=l32)


# ---- 3. through flows ------------------------------------------------------------------------------------------------------------
S8, S64, S70, S256 = ("strata_2_to_5", 8), ("one_segment", 64), ("boundary_at_a_round_edge", 70), ("one_segment", 256)
FLOW_CASES = {
    # name: (kind, case, hdims, nblocks, K, B, f64)
    "realnvp_d8": ("realnvp", S8, (32, 32), 2, 0, 0.0, False),
    "realnvp_d64": ("realnvp", S64, (32, 32), 2, 0, 0.0, False),
    "realnvp_d70_wide": ("realnvp", S70, (128, 100), 2, 0, 0.0, False),   # the weight-streaming shape of the sibling tests
    "nsf_d8": ("nsf", S8, (32, 32), 2, 8, 5.0, False),
    "realnvp_d8_f64": ("realnvp", S8, (32, 32), 2, 0, 0.0, True),         # the flat kernel
    "fullrank_d256": ("fullrank", S256, (), 1, 0, 0.0, False),
    "preconditioned_d8": ("preconditioned", S8, (32, 32), 2, 0, 0.0, False),
}
N = 33


def make_flow_case(nf, name):
    """-> (flow, tgt, neg_elbo(theta, xs) -> (loss, grad), elbos(theta, xs), theta, f64, mask); theta and xs in float64 give the
    reference, in float32 the floor; mask: the entries of the gradient that are compared (all but L's strict upper triangle)"""
    kind, case, hd, nl, K, B, f64 = FLOW_CASES[name]
    d = case[1]
    tgt, ref = make_riskset(nf, case, f64)
    rnd = (lambda a: a) if f64 else (lambda a: a.astype(np.float32).astype(np.float64))
    q0 = nf.MvNormal(d)
    if kind == "fullrank":
        th = fullrank_theta(d)
        flow = fullrank_flow(nf, d, f64, th)
        return flow, tgt, (lambda t, x: fr.neg_elbo_value_and_grad(t, x, ref)), (lambda t, x: fr.elbos(t, x, ref)), th, f64, None
    if kind == "preconditioned":
        spec = o.FlowSpec("realnvp", d, nl, hd)
        th = np.concatenate([fullrank_theta(d), rnd(o.init_params(spec, np.random.default_rng(3)))])
        flow = nf.preconditioned(nf.realnvp(q0, hd, nl, paramtype=tdt(f64)))
        assert flow.P == th.size
        flow = flow.with_theta(torch.tensor(th, dtype=tdt(f64), device="cuda"))
        return (flow, tgt, (lambda t, x: pr.neg_elbo_value_and_grad(spec, t, x, ref)), (lambda t, x: pr.elbos(spec, t, x, ref)), th, f64,
                ~pr.upper_mask(spec))
    spec = o.FlowSpec(kind, d, nl, hd, K, B)
    th = rnd(o.init_params(spec, np.random.default_rng(3)))
    flow = nf.Flow(spec.kind, q0, nl, hd, K, B, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))

    def elbos(t, x):
        ys, ladj, _ = o.flow_fwd(spec, t, x, keep=True)
        return ref(ys)[0] - o.std_normal_logpdf(x) + ladj

    return flow, tgt, (lambda t, x: composed_neg_elbo(spec, t, ref, x)), elbos, th, f64, None


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_elbo_value_and_gradient_through_a_flow(nf, name):
    """N = 33 on the flow's own Philox draws: value_and_gradient and the per-sample terms against the composed reference with exactly
    one target launch each; nf_elbo_batch on the regenerated draws equals nf_elbo_batch_rng"""
    flow, tgt, neg_elbo, elbos_of, th, f64, mask = make_flow_case(nf, name)
    key = f"riskset flow {name} N={N}"
    xs_dev = nf.device_specific_rand(nf.PhiloxRNG(41), flow.dist, N, dtype=tdt(f64))
    xs = xs_dev.double().cpu().numpy()
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs_dev), PROF)
    assert counts == ONE_LAUNCH, counts
    elbos, counts = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, xs_dev), PROF)
    assert counts == ONE_LAUNCH, counts
    pick = (lambda a: a) if mask is None else (lambda a: np.where(mask, a, 0.0))
    l_ref, g_ref = neg_elbo(th, xs)
    g_ref = pick(g_ref)
    e_ref = elbos_of(th, xs)
    print(f"{key}: loss {loss!r} reference {l_ref!r}; grad err / |g|inf {np.abs(g.double().cpu().numpy() - g_ref).max() / np.abs(g_ref).max():.3e}")
    assert np.isfinite(l_ref) and np.isfinite(g_ref).all() and np.isfinite(loss) and bool(torch.isfinite(g).all())
    v_xs = nf.elbo_batch(flow, tgt, xs_dev)
    v_rng = nf.elbo_batch(nf.PhiloxRNG(41), flow, tgt, N)
    l_rng, g_rng = nf.value_and_gradient(nf.elbo_batch, flow, tgt, N, rng=nf.PhiloxRNG(41))
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
        P.elementwise(key + ": elbos", elbos, e_ref, P.F64_RTOL, 1e-12)
        P.scalar(key + ": elbo_batch(xs)", v_xs, e_ref.mean(), P.F64_RTOL)
        P.scalar(key + ": elbo_batch(rng) vs elbo_batch(xs)", v_rng, v_xs, P.F64_RTOL)
        P.scalar(key + ": loss (rng) vs loss (xs)", l_rng, loss, P.F64_RTOL)
        P.gradient(key + ": grad (rng) vs grad (xs)", g_rng, g, P.F64_GRAD)
    else:
        l32, g32 = neg_elbo(P.f32(th), P.f32(xs))
        e32 = elbos_of(P.f32(th), P.f32(xs))
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": grad", g, g_ref, floor=pick(g32))
        P.elementwise(key + ": elbos", elbos, e_ref, floor=e32)
        P.scalar(key + ": elbo_batch(xs)", v_xs, e_ref.mean(), floor=e32.mean())
        P.scalar(key + ": elbo_batch(rng) vs elbo_batch(xs)", v_rng, v_xs)
        P.scalar(key + ": loss (rng) vs loss (xs)", l_rng, loss)
        P.gradient(key + ": grad (rng) vs grad (xs)", g_rng, g)


# ---- 4. the step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["realnvp_d8", "nsf_d8", "fullrank_d256", "realnvp_d70_wide"])
def test_elbo_step_equals_the_split_calls_and_the_graph_form_refuses(nf, name):
    """two consecutive nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit;
    nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED and leaves theta and the counter alone."""
    lib = nf.load_library()
    flow, tgt = make_flow_case(nf, name)[:2]
    n, seed = 33, 77
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert code == NF_ERR_UNSUPPORTED and torch.equal(th, flow.theta) and int(counter[0]) == 0 and not bool(m.any()) and not bool(v.any())
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    for step in range(2):
        loss, gnorm = C.c_double(0), C.c_double(0)
        _, counts = prof_counts(nf, ctx_a, lambda: nf._lib.check(lib.nf_elbo_step(
            ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS, C.byref(loss), C.byref(gnorm))), PROF)
        assert counts == ONE_LAUNCH, counts
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert loss.value == float(out[flow.P]) and gnorm.value == float(gn), (step, loss.value, float(out[flow.P]), gnorm.value, float(gn))
        assert np.isfinite(loss.value) and abs(loss.value) > 0.1
    assert not torch.equal(th, flow.theta)
    ctx_a.close()
    ctx_b.close()


# ---- 5. refusals and routes ------------------------------------------------------------------------------------------------------
def test_flows_with_in_kernel_targets_refuse_and_touch_nothing(nf):
    """planar, radial, mean-field and Hamiltonian flows (as ELBO target and as score) at all five ELBO entry points"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    lib = nf.load_library()
    ctx = new_ctx(nf)

    def five(desc, tc, th, m, v, out, counter, val, xs, n=16):
        return [lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(desc), C.byref(tc), vp(th), None, n, n, 1, 0, 0, vp(out)),
                lib.nf_elbo_batch(ctx.ptr, C.byref(desc), C.byref(tc), vp(th), vp(xs), n, None, C.byref(val)),
                lib.nf_elbo_batch_rng(ctx.ptr, C.byref(desc), C.byref(tc), vp(th), n, 1, 0, 0, C.byref(val)),
                lib.nf_elbo_step(ctx.ptr, C.byref(desc), C.byref(tc), vp(th), vp(m), vp(v), n, 1, 0, LR, B1, B2, EPS, None, None),
                lib.nf_elbo_step_enqueue(ctx.ptr, C.byref(desc), C.byref(tc), vp(th), vp(m), vp(v), n, 1, vp(counter), LR, B1, B2, EPS, None)]

    cases = [(nf.planarflow(nf.MvNormal(8), 4, paramtype=torch.float32, seed=1), False),
             (nf.radialflow(nf.MvNormal(8), 4, paramtype=torch.float32, seed=1), False),
             (nf.meanfield(nf.MvNormal(8), paramtype=torch.float64), True)]
    for flow, f64 in cases:
        tgt = make_riskset(nf, S8, f64)[0]
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        out = torch.full((flow.P + 1,), 7.0, dtype=tdt(f64), device="cuda")
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        val = C.c_double(123.0)
        xs = to_dev(o.base_sample(8, 16, 5, 0, 0), f64)
        assert five(flow.desc, tgt.c, th, m, v, out, counter, val, xs) == [NF_ERR_UNSUPPORTED] * 5, flow.kind
        torch.cuda.synchronize()
        assert val.value == 123.0 and bool((out == 7.0).all()) and torch.equal(th, flow.theta) and not bool(m.any()) and not bool(v.any())
        assert int(counter[0]) == 0
    # a Hamiltonian flow: neither as its score nor as the ELBO target of its joint density
    t3 = build_riskset(nf, *rf.arrays("mass_on_last_live_row", 3), False)[0]
    diag = nf.DiagGaussTarget(torch.zeros(3, device="cuda"), torch.ones(3, device="cuda"))
    buf = torch.zeros(256, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    val = C.c_double(123.0)
    for score, target in ((t3.c, diag.c), (diag.c, t3.c)):
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 6, 2, 3
        hd.score = C.cast(C.pointer(score), C.c_void_p)
        assert five(hd, target, buf, buf, buf, buf, counter, val, buf) == [NF_ERR_UNSUPPORTED] * 5
    torch.cuda.synchronize()
    assert not bool(buf.any()) and int(counter[0]) == 0 and val.value == 123.0
    ctx.close()


CLOSURE_CASES = {"planar_f64": ("planar", 10, True), "radial_f32": ("radial", 4, False), "meanfield_f64": ("meanfield", 1, True)}


@pytest.mark.parametrize("name", list(CLOSURE_CASES))
def test_flows_with_in_kernel_targets_take_the_closure_route(nf, name):
    """value_and_gradient on strata of 2-5 rows at d = 8: the generic closure with the device score (one flat target launch) matches
    the reference"""
    kind, nl, f64 = CLOSURE_CASES[name]
    d, n = 8, 37
    q0 = nf.MvNormal(d)
    if kind == "meanfield":
        flow = nf.meanfield(q0, paramtype=tdt(f64))
        flow = flow.with_theta(torch.tensor(np.concatenate([0.2 * np.arange(d) - 0.5, 0.7 + 0.1 * np.arange(d)]), dtype=tdt(f64), device="cuda"))
    else:
        flow = (nf.planarflow if kind == "planar" else nf.radialflow)(q0, nl, paramtype=tdt(f64), seed=3)
        flow = flow.with_theta(flow.theta * 0.3)
    tgt, ref = make_riskset(nf, S8, f64)
    xs = o.base_sample(d, n, 77, 0, 0)
    spec, th = o.FlowSpec(kind, d, nl), flow.theta.double().cpu().numpy()
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)), PROF)
    assert counts == ONE_LAUNCH, counts  # the device score, through the target's autograd node
    key = f"riskset closure route {name}"
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        l32, g32 = composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": grad", g, g_ref, floor=g32)


def test_train_flow_with_fullrank_lowers_the_loss_on_a_fixed_draw_set(nf):
    """train_flow(elbo_batch, fullrank Float64, RiskSetTarget (strata of 2-5 rows, d = 8), 64), six Adam(0.05) steps from seed 9, runs
    nf_elbo_step per iteration; losses and theta are those of the float64 numpy loop on the same Philox draws, and -ELBO on a fixed
    set of 256 draws is lower after training than before"""
    from normalizingflows_jl_amd import objectives as ob

    (_, d), n, seed, lr, iters = TRAIN
    tgt = train_target(nf, "cuda")
    X, p0 = rf.target_arrays(tgt)
    fixed = o.base_sample(d, 256, 1234, 0, 0, precision="f64")
    ref_losses, ref_theta, before, after = fullrank_numpy_losses(X, p0, n, seed, lr, iters, fixed)
    flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float64)
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(seed), None, {})
    fx = to_dev(fixed, True)
    loss0 = -nf.elbo_batch(flow, tgt, fx)
    trained, stats, st = nf.train_flow(nf.PhiloxRNG(seed), nf.elbo_batch, flow, tgt, n, max_iters=iters, optimiser=nf.Adam(lr))
    loss1 = -nf.elbo_batch(trained, tgt, fx)
    losses = [s["loss"] for s in stats]
    print("riskset train_flow losses", losses, "numpy loop", ref_losses, "fixed draws", loss0, loss1, "numpy", before, after)
    assert len(losses) == iters and st.t == iters and all(np.isfinite(losses)) and loss1 < loss0
    P.scalar("riskset train_flow fullrank f64: fixed draws before", loss0, before, P.F64_GRAD)
    P.scalar("riskset train_flow fullrank f64: fixed draws after", loss1, after, P.F64_GRAD)
    for i in range(iters):
        P.scalar(f"riskset train_flow fullrank f64: loss[{i}]", losses[i], ref_losses[i], P.F64_GRAD)
    P.gradient("riskset train_flow fullrank f64: theta after six steps", trained.theta, ref_theta, P.F64_GRAD)
