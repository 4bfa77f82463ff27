"""GPU tests of the scaled-block GLM target (NF_TARGET_SCALEGLM, ScaledGLMTarget) against tests/scaled_forms.py's numpy form on the
target's own buffers (composed with oracle.nf_oracle / tests/fullrank_ref.py for flows), at tests/parity.py's tolerances through
test_gpu_glm.py's criterion (check_logp, agree; Float32 checks pass `floor=`).  Every target is scaled_forms.fixture."""
import ctypes as C

import numpy as np
import pytest

import fullrank_ref as fr
import nf_oracle as o
import parity as P
import scaled_forms as sf
from test_gpu_glm import device_logp, nf, tag  # noqa: F401 (nf: the module fixture)
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, check_logp, composed_neg_elbo, new_ctx, prof_counts, sample_ys, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROF = ("target_scaleglm", "target_mixglm", "target")
ONE_LAUNCH = {"target_scaleglm": 1, "target_mixglm": 0, "target": 0}


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("p,S", [(3, 2), (31, 2), (84, 16), (140, 10)])  # tau rows over two accumulator blocks | DB = 4, most scales | second chunk
def test_target_logp(nf, p, S, f64):
    tgt = sf.fixture(nf, p, S, tdt(f64), "cuda")
    ref = sf.ref_of(tgt)
    assert len(set(tgt.families)) == 6 and tgt.rows == (384 if S > 3 else 352) and max(tgt.scales) == max(S - 2, 0) and -1 in tgt.scales
    for n in (1, 37):
        ys, cz = sample_ys(p + S, n, f64), []  # 1.5 randn: exp(-tau) spans more than a decade
        ref(ys, cz)
        assert min(c.min() for c in cz) >= 1e-3 and (n == 1 or np.ptp(ys[p:]) > 2.3)  # float32 cannot sit on the other side of the check function's kink
        check_logp(nf, f"scaleglm logp p={p} S={S} N={n} {tag(f64)}", tgt, ref, ys, f64)


FLOW_CASES = {  # name: (kind, p, S, hdims, f64)
    "realnvp_d5": ("realnvp", 3, 2, (32, 32), False),
    "realnvp_d33": ("realnvp", 31, 2, (64, 64), False),         # G over two accumulator blocks, tau in both
    "realnvp_d150_wide": ("realnvp", 140, 10, (128, 100), False),  # two feature chunks per row block
    "realnvp_d5_f64": ("realnvp", 3, 2, (32, 32), True),        # the flat kernel
    "fullrank_d5": ("fullrank", 3, 2, (), False),
}
N_FLOW = 48


def make_flow_case(nf, name):  # -> (flow, target, oracle(theta, xs) -> (loss, grad), theta, f64)
    kind, p, S, hd, f64 = FLOW_CASES[name]
    d = p + S
    tgt = sf.fixture(nf, p, S, tdt(f64), "cuda")
    ref = sf.ref_of(tgt)
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
    """N = 48 (a ragged second tile) against the composed oracle; exactly one "target_scaleglm" launch, no "target" / "target_mixglm" launch"""
    flow, tgt, oracle, th, f64 = make_flow_case(nf, name)
    key, xs = f"scaleglm flow {name} N={N_FLOW}", o.base_sample(tgt.d, N_FLOW, 77, 0, 0)
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
def test_a_weight_zero_row_a_block_without_a_family_and_a_nan_scale_index(nf, f64):
    """a weight-0 row of 1e30 features under scale 0 and the check block's code overwritten with 9: the bits of the target without the row and
    with that block's weights 0; the student blocks' scale index NaN: the bits of sidx = -1, and the numpy form at s = -1"""
    p, S, n = 3, 4, 37
    d = p + S
    plain = sf.fixture(nf, p, S, tdt(f64), "cuda")
    masked = sf.fixture(nf, p, S, tdt(f64), "cuda", edit=lambda i, A, off, wt: (np.vstack([A, np.full((1, p), 1e30)]), np.append(off, 0.0), np.append(wt, 0.0)) if i == 3 else (A, off, wt))
    R = masked.rows
    wt0, fam0, sidx0 = d + R, d + 2 * R, d + 2 * R + 2 * (R // 32)
    cb, sb = masked.families.index("check"), masked.families.index("student")
    assert R == plain.rows == 384 and masked.scales[sb:sb + 2] == [0, 0] and float(masked.A[32 * sb + 33, 0]) > 9e29 and float(masked.p0[fam0 + cb]) == 5.0
    plain.p0[wt0 + 32 * cb:wt0 + 32 * cb + 32] = 0.0  # (on the device buffer: the host's fold of the check rows' -tau stays in both)
    masked.p0[fam0 + cb] = 9.0
    ys = sample_ys(d, n, f64)
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(d, N_FLOW, 77, 0, 0), False)

    def same_bits(a, b):
        got, want = device_logp(nf, a, ys, f64), device_logp(nf, b, ys, f64)
        assert np.isfinite(got[0]).all() and np.abs(want[1]).max() > 0.1 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if not f64:
            (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, a, xs), nf.value_and_gradient(nf.elbo_batch, flow, b, xs)
            assert np.isfinite(l1) and l1 == l2 and torch.equal(g1, g2)

    same_bits(masked, plain)
    masked.p0[sidx0 + sb:sidx0 + sb + 2] = float("nan")
    plain.p0[sidx0 + sb:sidx0 + sb + 2] = -1.0
    same_bits(masked, plain)
    check_logp(nf, f"scaleglm NaN scale index {tag(f64)}", masked, sf.ref_of(masked), ys, f64)


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
    flow2, tgt2 = make_flow_case(nf, "realnvp_d33")[:2]  # the same call twice: the same bits (twelve row blocks: every wave takes several scales)
    xs = to_dev(o.base_sample(33, 97, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow2, tgt2, xs), nf.value_and_gradient(nf.elbo_batch, flow2, tgt2, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(nf.batched_elbos(flow2, tgt2, xs).clone(), nf.batched_elbos(flow2, tgt2, xs))
