"""GPU tests of the one-hidden-layer Bayesian neural-network targets (NF_TARGET_BNN_*; BNNTarget / BNNRegressionTarget /
BNNClassifierTarget): nf_target_logp (flat kernel, both element types) and the tiled MFMA kernel (through a Float32 full-rank flow)
at every shape of bnn_forms.SHAPES, v = 0 against GLMTarget, the sign and permutation symmetries, the zero-weight row, saturation,
determinism, the limits, RealNVP / NSF / Float64 / full-rank / preconditioned / weight-streaming flows as ELBO users, nf_elbo_step,
the refusals, the closure route and train_flow.

Reference values are the numpy form of tests/bnn_forms.py evaluated on the target's own `X` and `p0` in float64; whole-flow
references compose it with oracle.nf_oracle (or tests/fullrank_ref.py / tests/precond_ref.py) as neg_elbo_value_and_grad does.
Tolerances are tests/parity.py's: log p element-wise at Y_RTOL / Y_ATOL, scores and gradients by `gradient` at GRAD_RTOL, Float64
at F64_RTOL / F64_GRAD; every Float32 check passes `floor=`: the same form evaluated op by op in numpy float32 (test_bnn_cpu.py
holds that floor to 0.3x / 0.2x of the tolerances on these inputs, so it is not expected to decide a nf_target_logp check).

An identity full-rank flow (theta = [0 ; I]) hands its draws to the target unchanged (y = x bit for bit, ladj = 0): that is how the
tiled kernel is evaluated at chosen points y."""
import ctypes as C

import numpy as np
import pytest

import bnn_forms as bf
import fullrank_ref as fr
import glm_forms as gf
import nf_oracle as o
import parity as P
import precond_ref as pr
from __graft_entry__ import load_package
from test_bnn_cpu import TRAIN, fullrank_numpy_losses, train_target
from test_gpu_linpred import (B1, B2, EPS, LR, NF_ERR_UNSUPPORTED, composed_neg_elbo, new_ctx, prof_counts, tdt, to_dev, vp)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PROF = ("target_bnn", "target_softmax", "target_linpred", "target")
ONE_BNN_LAUNCH = {"target_bnn": 1, "target_softmax": 0, "target_linpred": 0, "target": 0}
N = bf.N_FULL
SHAPE_IDS = ["H%d_p%d_r%d" % s for s in bf.SHAPES]


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def tag(f64):
    return "f64" if f64 else "f32"


def dev(a, f64):
    return torch.tensor(np.asarray(a), dtype=tdt(f64), device="cuda")


def build_bnn(nf, family, H, X, scl, off, wt, par, f64, sigma_hidden=bf.SIGMA_HIDDEN, sigma_out=bf.SIGMA_OUT):
    tgt = nf.BNNTarget(family, dev(X, f64), H, scale=dev(scl, f64), offset=dev(off, f64), weights=dev(wt, f64),
                       param=par if family == "student" else None, prior_sigma_hidden=sigma_hidden, prior_sigma_out=sigma_out)
    return tgt, bf.ref_of(tgt)


_CASES = {}


def make_bnn(nf, family, shape, f64):
    """the target of a family and shape and its reference, built once per module and left unchanged"""
    key = (family, shape, f64)
    if key not in _CASES:
        H, p, rows = shape
        _CASES[key] = build_bnn(nf, family, H, *bf.arrays(family, H, p, rows), f64)
    return _CASES[key]


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


def check_logp(nf, key, tgt, ref, ys, f64):
    """value element-wise, score by `gradient`; the value does not depend on whether the score is asked for"""
    lp, sc = device_logp(nf, tgt, ys, f64)
    lp_only = nf.target_logp(tgt, to_dev(ys, f64)).double().cpu().numpy()
    assert np.array_equal(lp, lp_only), key
    lr, sr = ref(ys)
    l32, s32 = (None, None) if f64 else ref(ys.astype(np.float32))
    compare(key, lp, sc, lr, sr, f64, l32, s32)
    return lp, sc


def fullrank_flow(nf, d, f64, theta):
    flow = nf.fullrank(nf.MvNormal(d), paramtype=tdt(f64))
    return flow.with_theta(torch.tensor(theta, dtype=tdt(f64), device="cuda"))


def fullrank_theta(d, seed=3):
    """mu = 0.3 randn, L = I + 0.2 tril(randn) / sqrt(d): float32-representable"""
    rng = np.random.default_rng(seed + d)
    L = np.eye(d) + 0.2 * np.tril(rng.standard_normal((d, d))) / np.sqrt(d)
    return fr.join(0.3 * rng.standard_normal(d), L).astype(np.float32).astype(np.float64)


def tiled_logp(nf, tgt, ys):
    """log p of the TILED kernel at the points ys (Float32): the per-sample ELBO terms of the identity full-rank flow plus log q0"""
    d, n = ys.shape
    flow = fullrank_flow(nf, d, False, fr.join(np.zeros(d), np.eye(d)))
    xs = to_dev(ys, False)
    (e, counts) = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, xs), PROF)
    assert counts == ONE_BNN_LAUNCH, counts
    return e.double().cpu().numpy() + o.std_normal_logpdf(ys)


# ---- 1. nf_target_logp, and the tiled kernel, at every shape ---------------------------------------------------------------------
LOGP_CASES = [(fam, s) for fam in ("logit", "normal") for s in bf.SHAPES] + \
             [(fam, s) for fam in ("probit", "poisson", "student") for s in ((3, 5, 33), (16, 14, 70))]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family,shape", LOGP_CASES, ids=["%s-H%d_p%d_r%d" % ((f,) + s) for f, s in LOGP_CASES])
def test_target_logp(nf, family, shape, f64):
    H, p, rows = shape
    tgt, ref = make_bnn(nf, family, shape, f64)
    for n in bf.n_of(shape):
        check_logp(nf, f"bnn logp {family} {shape} N={n} {tag(f64)}", tgt, ref, bf.sample_ys(bf.dim(H, p), n), f64)


@pytest.mark.parametrize("family,shape", [("normal", s) for s in bf.SHAPES] + [("logit", (3, 5, 33)), ("probit", (3, 5, 33)),
                                                                              ("poisson", (2, 14, 133)), ("student", (4, 14, 40))],
                         ids=lambda v: v if isinstance(v, str) else "H%d_p%d_r%d" % v)
def test_tiled_kernel_through_a_fullrank_flow(nf, family, shape):
    """the Float32 full-rank flow hands the tiled layout to k_target_bnn_tiled: per-sample ELBO terms and the gradient (the shift's
    part is minus the mean score, the matrix's the scores times the draws) at every shape -- one target launch per call"""
    H, p, rows = shape
    d = bf.dim(H, p)
    tgt, ref = make_bnn(nf, family, shape, False)
    theta = fullrank_theta(d)
    flow = fullrank_flow(nf, d, False, theta)
    for n in bf.n_of(shape):
        key = f"bnn tiled {family} {shape} N={n}"
        xs = o.base_sample(d, n, 77, 0, 0)
        (elbos, counts) = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, to_dev(xs, False)), PROF)
        assert counts == ONE_BNN_LAUNCH, counts
        (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, False)), PROF)
        assert counts == ONE_BNN_LAUNCH, counts
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


def test_limits_are_unsupported_and_nothing_is_written(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx = new_ctx(nf)
    buf = torch.zeros(8192, device="cuda")
    for dtype in (0, 1):
        for H, d in ((2.0, 257), (16.0, 257), (1.0, 131)):  # d = 257 twice; p = 129
            t = Target(26, buf.data_ptr(), buf.data_ptr(), 4.0, H)
            assert lib.nf_target_logp(ctx.ptr, dtype, C.byref(t), d, 2, vp(buf), vp(buf), vp(buf)) == NF_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(buf.any())
    ctx.close()


# ---- 2. definitional checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", bf.FAMILIES)
def test_without_output_weights_the_network_is_a_glm_on_the_bias(nf, family, f64):
    """v = 0: f_i = c, so log p is GLMTarget's of the same family on the one-column design A_i = scl_i at z = c, with the same
    off / wt (flat GLM prior), plus the network's own constant and its prior on c -- the hidden prior is flat here.  Within the
    tolerances of the other checks.  The whole W block of the gradient is exactly +-0.0: g v_k (1 - a^2) x with v_k = 0."""
    shape = (3, 5, 33)
    H, p, rows = shape
    d, HP = bf.dim(H, p), H * p
    X, scl, off, wt, par = bf.arrays(family, H, p, rows)
    tgt, ref = build_bnn(nf, family, H, X, scl, off, wt, par, f64, sigma_hidden=np.inf)
    glm = nf.GLMTarget(family, dev(scl[:, None], f64), offset=dev(off, f64), weights=dev(wt, f64), param=par, prior_sigma=np.inf)
    ys = bf.sample_ys(d, 37)
    ys[HP:HP + H] = 0.0
    p0 = tgt.p0.double().cpu().numpy()
    assert p0[-2] == 0.0 and p0[-1] == 0.25
    lp, sc = device_logp(nf, tgt, ys, f64)
    lik = lp - p0[-3] + 0.5 * p0[-1] * ys[-1] ** 2
    lg = device_logp(nf, glm, ys[-1:], f64)[0]
    want = gf.logp_score(family, ys[-1:], scl[:, None], glm.p0.double().cpu().numpy(), np.inf)[0]
    key = f"bnn v = 0 vs glm {family} {tag(f64)}"
    if f64:
        P.elementwise(key + ": network likelihood", lik, want, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": the two kernels", lik, lg, P.F64_RTOL, 1e-12)
    else:
        floor = ref(ys.astype(np.float32))[0].astype(np.float64) - p0[-3] + 0.5 * p0[-1] * ys[-1] ** 2
        P.elementwise(key + ": network likelihood", lik, want, floor=floor)
        P.elementwise(key + ": glm likelihood", lg, want, floor=floor)
    assert (sc[:HP] == 0.0).all(), key
    assert np.abs(sc[HP:]).min() > 0.0  # v and c do move
    if not f64:  # the tiled kernel at the same points
        flow = fullrank_flow(nf, d, False, fr.join(np.zeros(d), np.eye(d)))
        _, g = nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(ys, False))
        g = g.double().cpu().numpy()
        assert (g[:HP] == 0.0).all(), key  # d loss / d mu_W = -mean of the W scores
        P.elementwise(key + ": tiled likelihood", tiled_logp(nf, tgt, ys) - p0[-3] + 0.5 * p0[-1] * ys[-1] ** 2, want, floor=floor)


def _flip(a, H, p, k):
    """the sign of (w_k, v_k) flipped in a (d, N) array"""
    b = a.copy()
    b[k * p:(k + 1) * p] *= -1.0
    b[H * p + k] *= -1.0
    return b


def _permute(a, H, p, perm):
    """hidden unit j of the result is unit perm[j] of a"""
    HP = H * p
    W = a[:HP].reshape(H, p, -1)[perm].reshape(HP, -1)
    return np.concatenate([W, a[HP:HP + H][perm], a[HP + H:]])


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["logit", "normal"])
def test_sign_and_permutation_symmetries(nf, family, f64):
    """tanh is odd: flipping the sign of (w_k, v_k) leaves log p, and flips those blocks of the gradient; permuting the hidden units
    leaves log p and permutes the blocks.  Device values at the transformed points against the transformed float64 reference --
    through nf_target_logp and, in Float32, log p through the tiled kernel"""
    shape = (3, 5, 33)
    H, p, rows = shape
    d = bf.dim(H, p)
    tgt, ref = make_bnn(nf, family, shape, f64)
    ys = bf.sample_ys(d, N)
    lr, sr = ref(ys)
    l32, s32 = (None, None) if f64 else ref(ys.astype(np.float32))
    moves = [("flip unit 1", lambda a: _flip(a, H, p, 1), lambda s: _flip(s, H, p, 1)),
             ("permute units", lambda a: _permute(a, H, p, [2, 0, 1]), lambda s: _permute(s, H, p, [2, 0, 1]))]
    for name, move, move_score in moves:
        y2 = move(ys)
        assert not np.array_equal(y2, ys)
        lp, sc = device_logp(nf, tgt, y2, f64)
        key = f"bnn {name} {family} {tag(f64)}"
        compare(key, lp, sc, lr, move_score(sr), f64, l32, None if f64 else move_score(s32))
        if not f64:
            P.elementwise(key + ": logp (tiled)", tiled_logp(nf, tgt, y2), lr, floor=l32)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["poisson", "normal"])
def test_zero_weight_row_of_huge_features_changes_no_bit(nf, family, f64):
    """a row of weight 0 whose X row holds 1e30 (its pre-activations overflow or cancel to NaN; for poisson phi overflows): value
    and score are bit for bit those of the target without the row -- through nf_target_logp and, in Float32, through the tiled
    kernel of a flow"""
    shape = (3, 5, 33)
    H, p, rows = shape
    d = bf.dim(H, p)
    X, scl, off, wt, par = bf.arrays(family, *shape)
    plain, _ = build_bnn(nf, family, H, X, scl, off, wt, par, f64)
    masked, _ = build_bnn(nf, family, H, np.vstack([X, np.full((1, p), 1e30)]), np.append(scl, 3.0), np.append(off, 50.0), np.append(wt, 0.0), par, f64)
    ys = bf.sample_ys(d, N)
    got, want = device_logp(nf, masked, ys, f64), device_logp(nf, plain, ys, f64)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if f64:
        return
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(d, N, 77, 0, 0), False)
    (l1, g1), (l2, g2) = nf.value_and_gradient(nf.elbo_batch, flow, masked, xs), nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    e1, e2 = nf.batched_elbos(flow, masked, xs), nf.batched_elbos(flow, plain, xs)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["logit", "normal"])
def test_saturated_units_stay_finite_and_accurate(nf, family, f64):
    """y scaled by 6 (pre-activations of tens), and the same with unit 0's weight on the ones column set to 1e4 (tanh is +-1 there and
    1 - a^2 exactly 0): finite, within tolerance of the float64 reference, and the saturated unit's W gradient is the prior's
    -par[2] w alone.  (The scaled y is rounded to float32 again, so both element types read the same numbers.)"""
    shape = (3, 5, 33)
    H, p, rows = shape
    d = bf.dim(H, p)
    tgt, ref = make_bnn(nf, family, shape, f64)
    ys = bf.sample_ys(d, 33, scale=6.0)
    pre = np.einsum("if,kfn->ikn", tgt.A.double().cpu().numpy(), ys[:H * p].reshape(H, p, 33))
    assert 15.0 < np.abs(pre).max() < 200.0, np.abs(pre).max()
    check_logp(nf, f"bnn saturation y x6 |pre| <= {np.abs(pre).max():.0f} {family} {tag(f64)}", tgt, ref, ys, f64)
    big = ys.copy()
    big[0] = 1e4 * np.where(np.arange(33) % 2 == 0, 1.0, -1.0)  # x_i0 = 1: the pre-activation is +-1e4 plus tens
    lp, sc = check_logp(nf, f"bnn saturation pre-activation 1e4 {family} {tag(f64)}", tgt, ref, big, f64)
    par2 = float(tgt.p0[-2])
    assert np.isfinite(sc[:p]).all() and np.allclose(sc[:p], -par2 * big[:p], rtol=1e-6, atol=0)
    if not f64:
        lt = tiled_logp(nf, tgt, ys)  # (not at 1e4: log q0 of such a draw is -5e7, and log p would drown in the ELBO term)
        assert np.isfinite(lt).all()
        P.elementwise(f"bnn saturation y x6 {family}: logp (tiled)", lt, ref(ys)[0], floor=ref(ys.astype(np.float32))[0])
        flow = fullrank_flow(nf, d, False, fr.join(np.zeros(d), np.eye(d)))
        _, g = nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(big, False))
        assert bool(torch.isfinite(g).all())
        P.gradient(f"bnn saturation pre-activation 1e4 {family}: grad (tiled)", g, fr.neg_elbo_value_and_grad(fr.join(np.zeros(d), np.eye(d)), big, ref)[1],
                   floor=fr.neg_elbo_value_and_grad(P.f32(fr.join(np.zeros(d), np.eye(d))), P.f32(big), ref)[1])


def test_two_identical_launches_are_bit_equal(nf):
    """(2, 14, 133): every wave takes row blocks, combined in wave order -- G, d/dv and d/dc; the flat kernel too"""
    shape = (2, 14, 133)
    d = bf.dim(2, 14)
    tgt, _ = make_bnn(nf, "logit", shape, False)
    flow = nf.realnvp(nf.MvNormal(d), (32, 32), 2, paramtype=torch.float32, seed=2)
    xs = to_dev(o.base_sample(d, N, 77, 0, 0), False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e1 = nf.batched_elbos(flow, tgt, xs).clone()
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    e2 = nf.batched_elbos(flow, tgt, xs)
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(e1, e2)
    ys = bf.sample_ys(d, N)
    for f64 in (False, True):
        t = make_bnn(nf, "logit", shape, f64)[0]
        a, b = device_logp(nf, t, ys, f64), device_logp(nf, t, ys, f64)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 3. through flows ------------------------------------------------------------------------------------------------------------
S7, S70 = (2, 2, 33), (3, 22, 40)
FLOW_CASES = {
    # name: (kind, family, shape, hdims, nblocks, K, B, f64)
    "realnvp_d7": ("realnvp", "normal", S7, (32, 32), 2, 0, 0.0, False),
    "nsf_d7": ("nsf", "logit", S7, (32, 32), 2, 8, 5.0, False),
    "realnvp_d7_f64": ("realnvp", "normal", S7, (32, 32), 2, 0, 0.0, True),               # the flat kernel
    "fullrank_d7": ("fullrank", "student", S7, (), 1, 0, 0.0, False),
    "preconditioned_d7": ("preconditioned", "normal", S7, (32, 32), 2, 0, 0.0, False),
    "realnvp_d70_wide": ("realnvp", "logit", S70, (128, 100), 2, 0, 0.0, False),          # the weight-streaming shape of the sibling tests
}


def make_flow_case(nf, name):
    """-> (flow, tgt, neg_elbo(theta, xs) -> (loss, grad), elbos(theta, xs), theta, f64, mask); theta and xs in float64 give the
    reference, in float32 the floor; mask: the entries of the gradient that are compared (all but L's strict upper triangle)"""
    kind, family, shape, hd, nl, K, B, f64 = FLOW_CASES[name]
    d = bf.dim(shape[0], shape[1])
    tgt, ref = make_bnn(nf, family, shape, f64)
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
    """N = 70 on the flow's own Philox draws: value_and_gradient and the per-sample terms against the composed reference with exactly
    one target launch each; nf_elbo_batch on the regenerated draws equals nf_elbo_batch_rng"""
    flow, tgt, neg_elbo, elbos_of, th, f64, mask = make_flow_case(nf, name)
    key = f"bnn flow {name} N={N}"
    xs_dev = nf.device_specific_rand(nf.PhiloxRNG(41), flow.dist, N, dtype=tdt(f64))
    xs = xs_dev.double().cpu().numpy()
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs_dev), PROF)
    assert counts == ONE_BNN_LAUNCH, counts
    elbos, counts = prof_counts(nf, flow.ctx, lambda: nf.batched_elbos(flow, tgt, xs_dev), PROF)
    assert counts == ONE_BNN_LAUNCH, counts
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
@pytest.mark.parametrize("name", ["realnvp_d7", "nsf_d7", "fullrank_d7", "realnvp_d70_wide"])
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
        assert counts == ONE_BNN_LAUNCH, counts
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

    cases = [(nf.planarflow(nf.MvNormal(7), 4, paramtype=torch.float32, seed=1), False),
             (nf.radialflow(nf.MvNormal(7), 4, paramtype=torch.float32, seed=1), False),
             (nf.meanfield(nf.MvNormal(7), paramtype=torch.float64), True)]
    for flow, f64 in cases:
        tgt = make_bnn(nf, "normal", S7, f64)[0]
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        out = torch.full((flow.P + 1,), 7.0, dtype=tdt(f64), device="cuda")
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        val = C.c_double(123.0)
        xs = to_dev(o.base_sample(7, 16, 5, 0, 0), f64)
        assert five(flow.desc, tgt.c, th, m, v, out, counter, val, xs) == [NF_ERR_UNSUPPORTED] * 5, flow.kind
        torch.cuda.synchronize()
        assert val.value == 123.0 and bool((out == 7.0).all()) and torch.equal(th, flow.theta) and not bool(m.any()) and not bool(v.any())
        assert int(counter[0]) == 0
    # a Hamiltonian flow: neither as its score nor as the ELBO target of its joint density
    bn3 = build_bnn(nf, "normal", 1, *bf.arrays("normal", 1, 1, 7), False)[0]  # d = 3
    diag = nf.DiagGaussTarget(torch.zeros(3, device="cuda"), torch.ones(3, device="cuda"))
    buf = torch.zeros(256, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    val = C.c_double(123.0)
    for score, target in ((bn3.c, diag.c), (diag.c, bn3.c)):
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
    """value_and_gradient on (2, 2, 33): the generic closure with the device score (one flat target launch) matches the reference"""
    kind, nl, f64 = CLOSURE_CASES[name]
    d, n = 7, 37
    q0 = nf.MvNormal(d)
    if kind == "meanfield":
        flow = nf.meanfield(q0, paramtype=tdt(f64))
        flow = flow.with_theta(torch.tensor(np.concatenate([0.2 * np.arange(d) - 0.5, 0.7 + 0.1 * np.arange(d)]), dtype=tdt(f64), device="cuda"))
    else:
        flow = (nf.planarflow if kind == "planar" else nf.radialflow)(q0, nl, paramtype=tdt(f64), seed=3)
        flow = flow.with_theta(flow.theta * 0.3)
    tgt, ref = make_bnn(nf, "normal", S7, f64)
    xs = o.base_sample(d, n, 77, 0, 0)
    spec, th = o.FlowSpec(kind, d, nl), flow.theta.double().cpu().numpy()
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)), PROF)
    assert counts == ONE_BNN_LAUNCH, counts  # the device score, through the target's autograd node
    key = f"bnn closure route {name}"
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        l32, g32 = composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": grad", g, g_ref, floor=g32)


def test_train_flow_with_fullrank_matches_the_float64_numpy_loop(nf):
    """train_flow(elbo_batch, fullrank Float64, BNNTarget (2, 2, 33), 64), six Adam(0.05) steps from seed 9, runs nf_elbo_step per
    iteration; losses and theta are those of the float64 numpy loop on the same Philox draws (test_bnn_cpu.py runs that loop alone
    and checks that it descends)."""
    from normalizingflows_jl_amd import objectives as ob

    family, (H, p, rows), n, seed, lr, iters = TRAIN
    d = bf.dim(H, p)
    tgt = train_target(nf, "cuda")
    X, p0 = bf.target_arrays(tgt)
    ref_losses, ref_theta = fullrank_numpy_losses(X, p0, H, family, n, seed, lr, iters)
    flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float64)
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(seed), None, {})
    trained, stats, st = nf.train_flow(nf.PhiloxRNG(seed), nf.elbo_batch, flow, tgt, n, max_iters=iters, optimiser=nf.Adam(lr))
    losses = [s["loss"] for s in stats]
    print("bnn train_flow losses", losses, "numpy loop", ref_losses)
    assert len(losses) == iters and st.t == iters and all(np.isfinite(losses)) and losses[-1] < losses[0]
    for i in range(iters):
        P.scalar(f"bnn train_flow fullrank f64: loss[{i}]", losses[i], ref_losses[i], P.F64_GRAD)
    P.gradient("bnn train_flow fullrank f64: theta after six steps", trained.theta, ref_theta, P.F64_GRAD)
