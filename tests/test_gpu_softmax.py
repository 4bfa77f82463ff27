"""GPU tests of the softmax regression target (NF_TARGET_SOFTMAX; SoftmaxRegressionTarget / MultinomialRegressionTarget):
nf_target_logp (flat kernel, both element types) and the tiled MFMA kernel (through a Float32 full-rank flow) at every shape of
softmax_forms.SHAPES, the definitional checks, RealNVP / NSF / full-rank / Float64 / weight-streaming / composed / general-base
flows as ELBO users, nf_elbo_step, the refusals, the closure route and train_flow.

Reference values are the numpy form of tests/softmax_forms.py evaluated on the target's own `X` and `p0` in float64; whole-flow
references compose it with oracle.nf_oracle (or tests/fullrank_ref.py) as neg_elbo_value_and_grad does.  Tolerances are
tests/parity.py's: log p element-wise at Y_RTOL / Y_ATOL, scores and gradients by `gradient` at GRAD_RTOL, Float64 at F64_RTOL /
F64_GRAD; every Float32 check passes `floor=`: the same form evaluated op by op in numpy float32 (test_softmax_cpu.py holds that
floor to 0.25x / 0.05x of the tolerances on these inputs, so it never decides a nf_target_logp check).

Inputs (softmax_forms.arrays / sample_ys): X ~ N(0, 1) / sqrt(p) rounded to float32 with a ones column, weights from
{1, 1, 2, 0.5, 0}, sigma = 3, y ~ N(0, 1) float32-representable, 70 samples (two tiles and a ragged third)."""
import ctypes as C

import numpy as np
import pytest

import fullrank_ref as fr
import nf_oracle as o
import parity as P
import softmax_forms as sf
from __graft_entry__ import load_package
from test_gpu_glm import comp_neg_elbo
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, composed_neg_elbo, logreg_logp_score, new_ctx, prof_counts, tdt, to_dev, vp)
from test_softmax_cpu import fullrank_numpy_losses

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROF = ("target_softmax", "target_linpred", "target")
ONE_SOFTMAX_LAUNCH = {"target_softmax": 1, "target_linpred": 0, "target": 0}
N = sf.N_FULL
SHAPE_IDS = ["C%d_p%d_r%d" % s for s in sf.SHAPES]


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def dev(a, f64):
    return torch.tensor(np.asarray(a), dtype=tdt(f64), device="cuda")


def build_softmax(nf, C_, X, lab, wt, f64, sigma=sf.SIGMA):
    tgt = nf.SoftmaxRegressionTarget(dev(X, f64), dev(lab, f64), C_, weights=None if wt is None else dev(wt, f64), prior_sigma=sigma)
    return tgt, sf.ref_of(tgt)


_CASES = {}


def make_softmax(nf, shape, f64):
    """the target of a shape and its reference, built once per module and left unchanged"""
    key = (shape, f64)
    if key not in _CASES:
        C_, p, rows = shape
        _CASES[key] = build_softmax(nf, C_, *sf.arrays(C_, p, rows), f64)
    return _CASES[key]


def device_logp(nf, tgt, ys, f64):
    lp, sc = nf.target_logp(tgt, to_dev(ys, f64), with_grad=True)
    torch.cuda.synchronize()
    return lp.double().cpu().numpy(), sc.double().cpu().numpy()


def check_logp(nf, key, tgt, ref, ys, f64):
    """value element-wise, score by `gradient`; the value does not depend on whether the score is asked for"""
    lp, sc = device_logp(nf, tgt, ys, f64)
    lp_only = nf.target_logp(tgt, to_dev(ys, f64)).double().cpu().numpy()
    assert np.isfinite(lp).all() and np.isfinite(sc).all(), key
    assert np.array_equal(lp, lp_only), key
    lr, sr = ref(ys)
    print(f"{key}: logp err {np.abs(lp - lr).max():.3e} of max |logp| {np.abs(lr).max():.3e}; score err / |s|inf {np.abs(sc - sr).max() / np.abs(sr).max():.3e}")
    if f64:
        P.elementwise(key + ": logp", lp, lr, P.F64_RTOL, 1e-12)
        P.gradient(key + ": score", sc, sr, P.F64_GRAD)
    else:
        l32, s32 = ref(ys.astype(np.float32))
        P.elementwise(key + ": logp", lp, lr, floor=l32)
        P.gradient(key + ": score", sc, sr, floor=s32)
    return lp, sc


# ---- 1. nf_target_logp, and the tiled kernel, at every shape ---------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sf.SHAPES, ids=SHAPE_IDS)
def test_target_logp(nf, shape, f64):
    C_, p, rows = shape
    tgt, ref = make_softmax(nf, shape, f64)
    for n in sf.n_of(shape):
        check_logp(nf, f"softmax logp {shape} N={n} {tag(f64)}", tgt, ref, sf.sample_ys(C_ * p, n), f64)


def fullrank_theta(d, seed=3):
    """mu = 0.3 randn, L = I + 0.2 tril(randn) / sqrt(d): float32-representable"""
    rng = np.random.default_rng(seed + d)
    L = np.eye(d) + 0.2 * np.tril(rng.standard_normal((d, d))) / np.sqrt(d)
    return fr.join(0.3 * rng.standard_normal(d), L).astype(np.float32).astype(np.float64)


def fullrank_flow(nf, d, f64, theta):
    flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64))
    return flow.with_theta(torch.tensor(theta, dtype=tdt(f64), device="cuda"))


@pytest.mark.parametrize("shape", sf.SHAPES, ids=SHAPE_IDS)
def test_tiled_kernel_through_a_fullrank_flow(nf, shape):
    """the Float32 full-rank flow hands the tiled layout to k_target_softmax_tiled: per-sample ELBO terms and the gradient (the
    shift's part is minus the mean score, the matrix's the scores times the draws) at every shape -- one target launch per call"""
    C_, p, rows = shape
    d = C_ * p
    tgt, ref = make_softmax(nf, shape, False)
    theta = fullrank_theta(d)
    flow = fullrank_flow(nf, d, False, theta)
    for n in sf.n_of(shape):
        key = f"softmax tiled {shape} N={n}"
        xs = o.base_sample(d, n, 77, 0, 0)
        (elbos, counts) = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, to_dev(xs, False)), PROF)
        assert counts == ONE_SOFTMAX_LAUNCH, counts
        (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, False)), PROF)
        assert counts == ONE_SOFTMAX_LAUNCH, counts
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


def test_wider_than_256_is_unsupported(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx = new_ctx(nf)
    buf = torch.zeros(4096, device="cuda")
    for dtype in (0, 1):
        t = Target(15, buf.data_ptr(), buf.data_ptr(), 4.0, 2.0)
        assert lib.nf_target_logp(ctx.ptr, dtype, C.byref(t), 258, 2, vp(buf), vp(buf), None) == NF_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(buf.any())
    ctx.close()


# ---- 2. definitional checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(3, 5, 33), (16, 16, 70)], ids=["C3_p5_r33", "C16_p16_r70"])
def test_at_zero_every_class_is_equally_likely(nf, shape, f64):
    """log p(0) = par[1] - log C sum_i wt_i, to the loss tolerance"""
    C_, p, rows = shape
    tgt, _ = make_softmax(nf, shape, f64)
    p0 = tgt.p0.double().cpu().numpy()
    want = p0[-1] - np.log(C_) * p0[rows:2 * rows].sum()
    lp, sc = device_logp(nf, tgt, np.zeros((C_ * p, 3)), f64)
    for j in range(3):
        P.scalar(f"softmax y = 0 {shape} {tag(f64)}: logp[{j}]", lp[j], want, P.F64_RTOL if f64 else P.LOSS_RTOL)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_two_classes_are_logistic_regression_on_the_difference(nf, f64):
    """C = 2 with unit weights: the likelihood part equals LogisticRegressionTarget's at w_1 - w_0 with t_i = +-1 from the labels.
    Each target's own prior term and constant are subtracted on the host in float64.  w_0 and w_1 - w_0 are multiples of 1 / 64, so
    the difference the logistic target reads is exact in either element type."""
    p, rows, n, sig_lr = 5, 33, 37, 2.0
    X, lab, _ = sf.arrays(2, p, rows)
    sm, ref = build_softmax(nf, 2, X, lab, None, f64)
    lr = nf.LogisticRegressionTarget(dev(X, f64), dev(lab, f64), prior_sigma=sig_lr)
    rng = np.random.default_rng(17)
    w0, v = np.round(64 * rng.standard_normal((p, n))) / 64, np.round(64 * rng.standard_normal((p, n))) / 64
    ys = np.vstack([w0, w0 + v])
    p0 = sm.p0.double().cpu().numpy()
    lik_sm = device_logp(nf, sm, ys, f64)[0] + 0.5 * p0[-2] * (ys * ys).sum(0) - p0[-1]
    lik_lr = device_logp(nf, lr, v, f64)[0] + (v * v).sum(0) / (2 * sig_lr**2) + 0.5 * p * np.log(2 * np.pi * sig_lr**2)
    A = X * (2 * lab - 1)[:, None]
    want = logreg_logp_score(v, A, sig_lr)[0] + (v * v).sum(0) / (2 * sig_lr**2) + 0.5 * p * np.log(2 * np.pi * sig_lr**2)
    key = f"softmax C = 2 vs logreg {tag(f64)}"
    if f64:
        P.elementwise(key + ": softmax likelihood", lik_sm, want, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": the two kernels", lik_sm, lik_lr, P.F64_RTOL, 1e-12)
    else:
        floor = ref(ys.astype(np.float32))[0].astype(np.float64) + 0.5 * p0[-2] * (ys * ys).sum(0) - p0[-1]
        P.elementwise(key + ": softmax likelihood", lik_sm, want, floor=floor)
        P.elementwise(key + ": logreg likelihood", lik_lr, want, floor=floor)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_zero_weight_row_of_huge_features_changes_no_bit(nf, f64):
    """a row of weight 0 whose X row holds 1e30 (its logits overflow or cancel to NaN): value and score are bit for bit those of the
    target without the row -- through nf_target_logp and, in Float32, through the tiled kernel of a flow"""
    shape = (3, 5, 33)
    C_, p, rows = shape
    X, lab, wt = sf.arrays(*shape)
    plain, _ = build_softmax(nf, C_, X, lab, wt, f64)
    masked, _ = build_softmax(nf, C_, np.vstack([X, np.full((1, p), 1e30)]), np.append(lab, 1.0), np.append(wt, 0.0), f64)
    ys = sf.sample_ys(C_ * p, N)
    got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if f64:
        return
    flow = nf.realnvp(nf.MvNormal(C_ * p), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(C_ * p, N, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    e1, e2 = nf.batched_elbos(flow, masked, xs), nf.batched_elbos(flow, plain, xs)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_large_logits_stay_finite_and_accurate(nf, f64):
    """y scaled by 30: logits of about +-100.  The row maximum is subtracted, nothing overflows; against float64 with `floor=`.
    (The scaled y is rounded to float32 again, so both element types read the same numbers.)"""
    shape = (3, 5, 33)
    tgt, ref = make_softmax(nf, shape, f64)
    ys = (30.0 * sf.sample_ys(15, 33)).astype(np.float32).astype(np.float64)
    u = np.einsum("if,cfn->icn", tgt.A.double().cpu().numpy(), ys.reshape(3, 5, 33))
    assert 60.0 < np.abs(u).max() < 400.0, np.abs(u).max()
    check_logp(nf, f"softmax large logits |u| <= {np.abs(u).max():.0f} {tag(f64)}", tgt, ref, ys, f64)


def test_permuting_rows_inside_their_32_row_blocks_leaves_logp(nf):
    """(3, 21, 133): five row blocks.  Both kernels, Float32: the permuted target's values against the float64 reference (the
    flat kernel) and the per-sample ELBO terms of a RealNVP flow (the tiled kernel) against the unpermuted ones"""
    shape = (3, 21, 133)
    C_, p, rows = shape
    d = C_ * p
    X, lab, wt = sf.arrays(*shape)
    perm = np.concatenate([b + np.random.default_rng(b).permutation(min(32, rows - b)) for b in range(0, rows, 32)])
    assert sorted(perm) == list(range(rows)) and (perm != np.arange(rows)).any() and (perm // 32 == np.arange(rows) // 32).all()
    tgt, ref = make_softmax(nf, shape, False)
    pt, _ = build_softmax(nf, C_, X[perm], lab[perm], wt[perm], False)
    ys = sf.sample_ys(d, N)
    lp = device_logp(nf, pt, ys, False)[0]
    P.elementwise("softmax rows permuted in blocks: logp", lp, ref(ys)[0], floor=ref(ys.astype(np.float32))[0])
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(d, N, 77, 0, 0), False)
    P.elementwise("softmax rows permuted in blocks: elbos (tiled)", nf.batched_elbos(flow, pt, xs), nf.batched_elbos(flow, tgt, xs))


def test_two_identical_launches_are_bit_equal(nf):
    """(3, 21, 133): every wave takes row blocks, combined in wave order; the flat kernel too"""
    shape = (3, 21, 133)
    d = 63
    tgt, _ = make_softmax(nf, shape, False)
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(d, N, 77, 0, 0), False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e1 = nf.batched_elbos(flow, tgt, xs).clone()
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e2 = nf.batched_elbos(flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)
    ys = sf.sample_ys(d, N)
    a, b = device_logp(nf, tgt, ys, False), device_logp(nf, tgt, ys, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 3. through flows ------------------------------------------------------------------------------------------------------------
S6, S70 = (3, 2, 33), (2, 35, 40)
FLOW_CASES = {
    # name: (kind, shape, hdims, nblocks, K, B, f64)
    "realnvp_d6": ("realnvp", S6, (32, 32), 2, 0, 0.0, False),
    "nsf_d6": ("nsf", S6, (32, 32), 2, 8, 5.0, False),
    "fullrank_d6": ("fullrank", S6, (), 1, 0, 0.0, False),
    "realnvp_d6_f64": ("realnvp", S6, (32, 32), 2, 0, 0.0, True),           # the flat kernel
    "composition_d6": ("planar+realnvp", S6, (32, 32), 2, 0, 0.0, False),
    "dense_base_d6": ("realnvp/dense", S6, (32, 32), 2, 0, 0.0, False),
    "realnvp_d70": ("realnvp", S70, (32, 32), 2, 0, 0.0, False),            # 35 conditioner inputs: a weight-streaming shape already
    "realnvp_d70_wide": ("realnvp", S70, (128, 100), 2, 0, 0.0, False),     # the weight-streaming shape of the sibling tests
    "fullrank_d70": ("fullrank", S70, (), 1, 0, 0.0, False),
    "fullrank_d70_f64": ("fullrank", S70, (), 1, 0, 0.0, True),
    "realnvp_d70_f64": ("realnvp", S70, (32, 32), 2, 0, 0.0, True),
}


def make_flow_case(nf, name):
    """-> (flow, tgt, neg_elbo(theta, xs) -> (loss, grad), elbos(theta, xs), theta, f64); theta and xs in float64 give the reference,
    in float32 the floor"""
    kind, shape, hd, nl, K, B, f64 = FLOW_CASES[name]
    d = shape[0] * shape[1]
    tgt, ref = make_softmax(nf, shape, f64)
    rnd = (lambda a: a) if f64 else (lambda a: a.astype(np.float32).astype(np.float64))
    q0 = nf.MvNormal(d)
    logq = o.std_normal_logpdf
    if kind == "fullrank":
        th = fullrank_theta(d)
        flow = fullrank_flow(nf, d, f64, th)
        return flow, tgt, (lambda t, x: fr.neg_elbo_value_and_grad(t, x, ref)), (lambda t, x: fr.elbos(t, x, ref)), th, f64
    if kind == "planar+realnvp":
        rng = np.random.default_rng(4)
        specs = [o.FlowSpec("planar", d, 3, ()), o.FlowSpec("realnvp", d, nl, hd)]
        ths = [rnd(0.3 * o.init_params(specs[0], rng)), rnd(o.init_params(specs[1], rng))]
        segs = [nf.Flow(sp.kind, q0, sp.nlayers, sp.hdims, dtype=tdt(f64), device="cuda", theta=torch.tensor(t, dtype=tdt(f64), device="cuda"))
                for sp, t in zip(specs, ths)]

        def elbos(t, x):
            ys, ladj = o.comp_fwd(specs, t, x)[:2]
            return ref(ys)[0] - o.std_normal_logpdf(x) + ladj

        return nf.create_flow(segs, q0), tgt, (lambda t, x: comp_neg_elbo(specs, t, ref, x)), elbos, np.concatenate(ths), f64
    spec = o.FlowSpec("realnvp" if kind == "realnvp/dense" else kind, d, nl, hd, K, B)
    th = rnd(o.init_params(spec, np.random.default_rng(3)))
    if kind == "realnvp/dense":  # q0 = MvNormal(mu, Sigma): the draws xs are q0's own, log q0 is the multivariate normal's
        rng = np.random.default_rng(d)
        A = rng.standard_normal((d, d)) / np.sqrt(d)
        mu, Sigma = rnd(rng.standard_normal(d)), rnd(A @ A.T + 0.5 * np.eye(d))
        q0 = nf.MvNormal(dev(mu, f64), dev(Sigma, f64))
        obase = ("dense", mu, np.linalg.cholesky(Sigma))
        logq = lambda x: o.base_logpdf(obase, x.astype(np.float64)).astype(x.dtype)
    flow = nf.Flow(spec.kind, q0, nl, hd, K, B, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))

    def neg_elbo(t, x):  # composed_neg_elbo with q0's own density (which does not depend on theta)
        n = x.shape[1]
        ys, ladj, states = o.flow_fwd(spec, t, x, keep=True)
        lp, sc = ref(ys)
        _, grad = o.flow_bwd(spec, t, states, (-sc / n).astype(x.dtype), np.full(n, -1.0 / n, dtype=x.dtype))
        return -(lp - logq(x) + ladj).mean(), grad

    def elbos(t, x):
        ys, ladj, _ = o.flow_fwd(spec, t, x, keep=True)
        return ref(ys)[0] - logq(x) + ladj

    return flow, tgt, neg_elbo, elbos, th, f64


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_elbo_value_and_gradient_through_a_flow(nf, name):
    """N = 70 on the flow's own Philox draws: value_and_gradient and the per-sample terms against the composed reference with exactly
    one target launch each; nf_elbo_batch on the regenerated draws equals nf_elbo_batch_rng"""
    flow, tgt, neg_elbo, elbos_of, th, f64 = make_flow_case(nf, name)
    key = f"softmax flow {name} N={N}"
    xs_dev = nf.device_specific_rand(nf.PhiloxRNG(41), flow.dist, N, dtype=tdt(f64))
    xs = xs_dev.double().cpu().numpy()
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs_dev), PROF)
    assert counts == ONE_SOFTMAX_LAUNCH, counts
    elbos, counts = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, xs_dev), PROF)
    assert counts == ONE_SOFTMAX_LAUNCH, counts
    l_ref, g_ref = neg_elbo(th, xs)
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
        P.gradient(key + ": grad", g, g_ref, floor=g32)
        P.elementwise(key + ": elbos", elbos, e_ref, floor=e32)
        P.scalar(key + ": elbo_batch(xs)", v_xs, e_ref.mean(), floor=e32.mean())
        P.scalar(key + ": elbo_batch(rng) vs elbo_batch(xs)", v_rng, v_xs)
        P.scalar(key + ": loss (rng) vs loss (xs)", l_rng, loss)
        P.gradient(key + ": grad (rng) vs grad (xs)", g_rng, g)


# ---- 4. the step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["realnvp_d6", "nsf_d6", "fullrank_d6", "realnvp_d70_wide"])
def test_elbo_step_equals_the_split_calls_and_the_graph_form_refuses(nf, name):
    """two consecutive nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit;
    nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED and leaves theta and the counter alone."""
    lib = nf.load_library()
    flow, tgt = make_flow_case(nf, name)[:2]
    n, seed = 70, 77
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
        assert counts == ONE_SOFTMAX_LAUNCH, counts
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

    cases = [(nf.planarflow(nf.MvNormal(6), 4, paramtype=torch.float32, seed=1), False),
             (nf.radialflow(nf.MvNormal(6), 4, paramtype=torch.float32, seed=1), False),
             (nf.meanfield(nf.MvNormal(6), paramtype=torch.float64), True)]
    for flow, f64 in cases:
        tgt = make_softmax(nf, S6, f64)[0]
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        out = torch.full((flow.P + 1,), 7.0, dtype=tdt(f64), device="cuda")
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        val = C.c_double(123.0)
        xs = to_dev(o.base_sample(6, 16, 5, 0, 0), f64)
        assert five(flow.desc, tgt.c, th, m, v, out, counter, val, xs) == [NF_ERR_UNSUPPORTED] * 5, flow.kind
        torch.cuda.synchronize()
        assert val.value == 123.0 and bool((out == 7.0).all()) and torch.equal(th, flow.theta) and not bool(m.any()) and not bool(v.any())
        assert int(counter[0]) == 0
    # a Hamiltonian flow: neither as its score nor as the ELBO target of its joint density
    sm2 = build_softmax(nf, 2, *sf.arrays(2, 1, 7), False)[0]  # d = 2
    diag = nf.DiagGaussTarget(torch.zeros(2, device="cuda"), torch.ones(2, device="cuda"))
    buf = torch.zeros(256, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    val = C.c_double(123.0)
    for score, target in ((sm2.c, diag.c), (diag.c, sm2.c)):
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
        hd.score = C.cast(C.pointer(score), C.c_void_p)
        assert five(hd, target, buf, buf, buf, buf, counter, val, buf) == [NF_ERR_UNSUPPORTED] * 5
    torch.cuda.synchronize()
    assert not bool(buf.any()) and int(counter[0]) == 0 and val.value == 123.0
    ctx.close()


CLOSURE_CASES = {"planar_f64": ("planar", 10, True), "radial_f32": ("radial", 4, False), "meanfield_f64": ("meanfield", 1, True)}


@pytest.mark.parametrize("name", list(CLOSURE_CASES))
def test_flows_with_in_kernel_targets_take_the_closure_route(nf, name):
    """value_and_gradient on (3, 2, 33): the generic closure with the device score (one flat target launch) matches the reference"""
    kind, nl, f64 = CLOSURE_CASES[name]
    d, n = 6, 37
    q0 = nf.MvNormal(d)
    if kind == "meanfield":
        flow = nf.meanfield(q0, paramtype=tdt(f64))
        flow = flow.with_theta(torch.tensor(np.concatenate([0.2 * np.arange(d) - 0.5, 0.7 + 0.1 * np.arange(d)]), dtype=tdt(f64), device="cuda"))
    else:
        flow = (nf.planarflow if kind == "planar" else nf.radialflow)(q0, nl, paramtype=tdt(f64), seed=3)
        flow = flow.with_theta(flow.theta * 0.3)
    tgt, ref = make_softmax(nf, S6, f64)
    xs = o.base_sample(d, n, 77, 0, 0)
    spec, th = o.FlowSpec(kind, d, nl), flow.theta.double().cpu().numpy()
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)), PROF)
    assert counts == ONE_SOFTMAX_LAUNCH, counts  # the device score, through the target's autograd node
    key = f"softmax closure route {name}"
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        l32, g32 = composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": grad", g, g_ref, floor=g32)


def test_train_flow_with_fullrank_matches_the_float64_numpy_loop(nf):
    """train_flow(elbo_batch, fullrank Float64, SoftmaxRegressionTarget (3, 2, 33), 64), six Adam(0.05) steps from seed 9, runs
    nf_elbo_step per iteration; losses and theta are those of the float64 numpy loop on the same Philox draws
    (test_softmax_cpu.py runs that loop alone and checks that it descends)."""
    from normalizingflows_jl_amd import objectives as ob

    C_, p, rows = S6
    d, n, seed, lr = 6, 64, 9, 0.05
    tgt, _ = make_softmax(nf, S6, True)
    X, p0 = sf.target_arrays(tgt)
    ref_losses, ref_theta = fullrank_numpy_losses(X, p0, C_, n, seed, lr, 6)
    flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float64)
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(seed), None, {})
    trained, stats, st = nf.train_flow(nf.PhiloxRNG(seed), nf.elbo_batch, flow, tgt, n, max_iters=6, optimiser=nf.Adam(lr))
    losses = [s["loss"] for s in stats]
    print("softmax train_flow losses", losses, "numpy loop", ref_losses)
    assert len(losses) == 6 and st.t == 6 and all(np.isfinite(losses)) and losses[5] < losses[0]
    for i in range(6):
        P.scalar(f"softmax train_flow fullrank f64: loss[{i}]", losses[i], ref_losses[i], P.F64_GRAD)
    P.gradient("softmax train_flow fullrank f64: theta after six steps", trained.theta, ref_theta, P.F64_GRAD)


def test_multinomial_counts_are_the_expanded_rows(nf):
    """MultinomialRegressionTarget on the device against scipy's multinomial log-pmf plus the prior (Float64)"""
    from scipy import special as sp
    from scipy import stats

    rng = np.random.default_rng(6)
    rows, p, C_ = 9, 3, 4
    X = rng.standard_normal((rows, p)) / np.sqrt(p)
    counts = rng.integers(0, 5, (rows, C_))
    w = rng.choice(np.array(sf.WEIGHTS), rows)
    tgt = nf.MultinomialRegressionTarget(dev(X, True), torch.tensor(counts, device="cuda"), weights=dev(w, True), prior_sigma=2.0)
    ys = sf.sample_ys(C_ * p, 5)
    probs = sp.softmax(np.einsum("if,cfn->inc", X, ys.reshape(C_, p, 5)), axis=2)
    want = sum(w[i] * stats.multinomial.logpmf(counts[i], counts[i].sum(), probs[i]) for i in range(rows)) + stats.norm.logpdf(ys, 0.0, 2.0).sum(0)
    P.elementwise("softmax multinomial f64: logp vs scipy", device_logp(nf, tgt, ys, True)[0], want, P.F64_RTOL, 1e-12)
