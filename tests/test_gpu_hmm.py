"""GPU tests of the hidden-Markov-model targets (NF_TARGET_HMM_*, HiddenMarkovTarget) against tests/hmm_forms.py's log-space numpy form
on the target's own buffers (composed with oracle.nf_oracle / tests/fullrank_ref.py for flows), at tests/parity.py's tolerances through
test_gpu_glm.py's criterion (check_logp; Float32 checks pass `floor=`).  Every target is hmm_forms.fixture."""
import ctypes as C

import numpy as np
import pytest

import fullrank_ref as fr
import hmm_forms as hf
import nf_oracle as o
import parity as P
from test_gpu_glm import device_logp, nf, tag  # noqa: F401 (nf: the module fixture)
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, new_ctx, prof_counts, sample_ys, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROF = ("target_hmm", "target")
ONE_LAUNCH = {"target_hmm": 1, "target": 0}
FAMILIES = ("normal", "poisson", "bernoulli")


def cases():  # (K, R, starts): L the segment length the package exports
    from __graft_entry__ import load_package
    L = load_package()._lib.NF_HMM_SEGMENT
    return [(2, 1, (0,)),                                          # no transition
            (3, L - 1, (0,)), (3, L, (0,)), (3, L + 1, (0,)),      # one checkpoint boundary from each side
            (5, 2 * L + 3, (0, L + L // 2)),                       # idle lanes in a group of 8, three segments, the second start in mid-segment
            (8, L + 1, (0,))]                                      # the full group


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("K,R,starts", cases())
@pytest.mark.parametrize("family", FAMILIES)
def test_target_logp(nf, family, K, R, starts, f64):
    tgt = hf.fixture(nf, family, K, R, starts, tdt(f64), "cuda")
    ref = hf.ref_of(tgt)
    for n in (1, 37):
        check_logp(nf, f"hmm logp {family} K={K} R={R} N={n} {tag(f64)}", tgt, ref, 0.7 * sample_ys(tgt.d, n, f64), f64)


def test_an_outlier_forty_sigma_from_every_mean_does_not_underflow(nf):
    """sigma_k = 0.1 and one observation 40 sigma past the nearest mean: min l - max l spans more than float32's exponent range and
    exp(max l) is 0 in float32, so a float32 recursion without the row shift would divide by 0; the device stays finite, at tolerance"""
    K, R = 3, nf._lib.NF_HMM_SEGMENT + 1

    def edit(x, wt, off):
        x[R // 3], wt[R // 3] = 8.0 + off[R // 3], 1.0

    tgt = hf.fixture(nf, "normal", K, R, (0,), torch.float32, "cuda", x_edit=edit)
    ys = 0.3 * sample_ys(tgt.d, 5, False)
    ys[K + K * K:K + K * K + K] = np.float32([0.0, 2.0, 4.0])[:, None]     # means; offsets are 0.3 randn
    ys[K + K * K + K:] = np.float32(np.log(0.1))
    x, off = float(tgt.p0[R // 3]), float(tgt.p0[R + R // 3])
    l = -0.5 * ((x - off - np.array([0.0, 2.0, 4.0])) / 0.1) ** 2
    assert l.max() < -700 and l.min() - l.max() < -104 and np.exp(np.float32(l.max())) == 0  # (below float32's smallest subnormal)
    lr, sr = hf.ref_of(tgt)(ys)
    assert np.isfinite(lr).all() and np.isfinite(sr).all()
    check_logp(nf, "hmm logp normal outlier f32", tgt, hf.ref_of(tgt), ys, False)


FLOW_CASES = {"realnvp": ("realnvp", (32, 32), False), "fullrank": ("fullrank", (), False), "realnvp_f64": ("realnvp", (32, 32), True)}
N_FLOW = 48


def make_flow_case(nf, name):  # -> (flow, target, oracle(theta, xs) -> (loss, grad), theta, f64): K = 2, normal family, d = 10
    kind, hd, f64 = FLOW_CASES[name]
    tgt = hf.fixture(nf, "normal", 2, nf._lib.NF_HMM_SEGMENT + 5, (0, 20), tdt(f64), "cuda")
    d, ref = tgt.d, hf.ref_of(tgt)
    if kind == "fullrank":
        rng = np.random.default_rng(3 + d)
        th = P.f32(fr.join(0.3 * rng.standard_normal(d), 0.5 * (np.eye(d) + 0.2 * np.tril(rng.standard_normal((d, d))) / np.sqrt(d)))).astype(np.float64)
        flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64)).with_theta(torch.tensor(th, dtype=tdt(f64), device="cuda"))
        return flow, tgt, (lambda t, x: fr.neg_elbo_value_and_grad(t, x, ref)), th, f64
    spec = o.FlowSpec(kind, d, 2, hd)
    th = P.f32(o.init_params(spec, np.random.default_rng(3))).astype(np.float64)
    flow = nf.Flow(kind, nf.MvNormal(d), 2, hd, 0, 0.0, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))
    return flow, tgt, (lambda t, x: composed_neg_elbo(spec, t, ref, x)), th, f64


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_flow(nf, name):
    """N = 48 (a ragged second tile) against the composed oracle; exactly one "target_hmm" launch, no "target" launch"""
    flow, tgt, oracle, th, f64 = make_flow_case(nf, name)
    key, xs = f"hmm flow {name} N={N_FLOW}", o.base_sample(tgt.d, N_FLOW, 77, 0, 0)
    l_ref, g_ref = oracle(th, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)), PROF)
    assert counts == ONE_LAUNCH and np.isfinite(l_ref) and np.isfinite(g_ref).all(), counts
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        P.scalar(key + ": loss", loss, l_ref)
        P.gradient(key + ": grad", g, g_ref, floor=oracle(P.f32(th), P.f32(xs))[1])


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_a_missing_row_holds_anything_and_a_call_repeats_its_bits(nf, f64):
    """the weight-0 row with x = 1e30: the bits of the same target with x = 0 there; the same value_and_gradient call twice: the same bits"""
    K, R = 5, 2 * nf._lib.NF_HMM_SEGMENT + 3

    def edit(v):
        def f(x, wt, off):
            x[R // 2] = v
        return f

    huge, plain = (hf.fixture(nf, "normal", K, R, (0, 70), tdt(f64), "cuda", x_edit=edit(v)) for v in (1e30, 0.0))
    assert float(huge.p0[R // 2]) > 9e29 and float(huge.p0[2 * R + R // 2]) == 0.0
    ys = 0.7 * sample_ys(huge.d, 37, f64)
    got, want = device_logp(nf, huge, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.abs(want[1]).max() > 0.1 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    flow, tgt = make_flow_case(nf, "realnvp_f64" if f64 else "realnvp")[:2]
    xs = to_dev(o.base_sample(tgt.d, 97, 77, 0, 0), f64)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs), nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    assert np.isfinite(l1) and l1 == l2 and torch.equal(g1, g2)


def test_elbo_step_equals_the_split_calls_and_the_other_routes_refuse(nf):
    """two nf_elbo_step calls == value-and-grad + Adam on a second context, bit for bit; the other routes refuse and touch nothing"""
    lib = nf.load_library()
    flow, tgt = make_flow_case(nf, "realnvp")[:2]
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
    ys, lp = to_dev(sample_ys(108, 4, False), False), torch.full((4,), 7.0, device="cuda")
    big = [nf._lib.Target(tgt.c.kind, tgt.p0.data_ptr(), tgt.A.data_ptr(), 8.0, 9.0), nf._lib.Target(tgt.c.kind, tgt.p0.data_ptr(), tgt.A.data_ptr(), nf._lib.NF_HMM_MAXR + 1.0, 2.0)]
    bcodes = [lib.nf_target_logp(ctx_a.ptr, 0, C.byref(t), dd, 4, vp(ys), vp(lp), None) for t, dd in zip(big, (108, 10))]  # K = 9; R = NF_HMM_MAXR + 1
    torch.cuda.synchronize()
    assert code == pcode == mcode == NF_ERR_UNSUPPORTED and bcodes == [NF_ERR_UNSUPPORTED] * 2 and torch.equal(th, flow.theta) and int(counter[0]) == 0
    assert torch.equal(pth, planar.theta) and not bool(pm.any()) and not bool(pv.any()) and bool((p0o == 7.0).all()) and bool((Ao == 7.0).all()) and bool((lp == 7.0).all())
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
