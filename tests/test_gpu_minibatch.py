"""GPU checks of the row-minibatch target (nf_target_minibatch, MinibatchTarget): the indices against the numpy rule, the gathered
buffers bit for bit against a numpy gather of host copies (every kind of the main grid, both element types, the row-width cases),
m = R as the full target (buffers, nf_target_logp, three training steps), m < R training against a manual loop and log p against the
kinds' float64 forms on the gathered rows, exact unbiasedness over all batches of a small case, the closure route, the non-centring
layer over the full target's groups, and the refusals -- with the output buffers untouched and out-of-range indices bounded."""
import ctypes as C

import numpy as np
import pytest
import torch

import bnn_forms as bf
import disp_forms as df
import glm_forms as gf
import hier_forms as hf
import minibatch_ref as mr
import nf_oracle as o
import parity as P
import softmax_forms as sf
from __graft_entry__ import load_package
from test_gpu_linpred import B1, B2, EPS, LR, NF_ERR_ARG, NF_ERR_UNSUPPORTED, check_logp, tdt, to_dev, vp

pytestmark = pytest.mark.gpu

F64 = pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
R, D = mr.R_MAIN, mr.D_MAIN


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


_FULL = {}


def full_target(nf, kind, f64):
    """the main grid's full targets, built once and never changed"""
    if (kind, f64) not in _FULL:
        _FULL[kind, f64] = mr.build(nf, kind, tdt(f64), "cuda")
    return _FULL[kind, f64]


def host(t):
    return t.detach().cpu().numpy()


def numpy_batch(nf, full, m, idx):
    segs, wseg, _ = nf.flows.minibatch_segments(full)
    return mr.gather(host(full.p0), host(full.A), segs, wseg, full.rows, m, np.asarray(idx, dtype=np.int64))


def assert_bits(got, want, what):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.flatnonzero(got.ravel() != want.ravel())[:8])


def ref_on(kind, full, A, p0):
    """the kind's float64 form (its float32 floor for float32 y) on host buffers A, p0"""
    A, p0 = A.astype(np.float64), p0.astype(np.float64)
    if kind == "glm":
        return lambda y: gf.logp_score(full.family, y, A, p0, full.prior_sigma)
    if kind == "hglm":
        return lambda y: hf.logp_score(full.family, y, A, p0, full.G)
    if kind.startswith("dglm"):
        return lambda y: df.logp_score(full.family, y, A, p0, full.G)
    if kind == "softmax":
        return lambda y: sf.logp_score(y, A, p0, full.n_classes)
    return lambda y: bf.logp_score(y, A, p0, full.n_hidden, full.family)


def sample_ys(d, n, f64, seed=4):
    ys = 0.5 * np.random.default_rng(seed + d + n).standard_normal((d, n))
    return ys if f64 else ys.astype(np.float32).astype(np.float64)


# ---- 1. indices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", mr.M_MAIN)
def test_indices_follow_the_numpy_rule(nf, m):
    full = full_target(nf, "glm", False)
    seen = []
    for seed, stream in ((0, 0), (1, 0), (1, 1), (1, 2**32 - 1), (2**64 - 1, 5), (0x1234567800000000, 77)):
        mb = nf.MinibatchTarget(full, m, seed=seed)
        assert mb.rows == m and mb.d == D and mb.full is full and mb.indices is mb.idx
        assert_bits(mb.indices, mr.indices(R, m, seed, 0).astype(np.int32), "constructed at stream 0")
        assert mb.resample(stream) is mb
        want = mr.indices(R, m, seed, stream).astype(np.int32)
        assert_bits(mb.indices, want, (seed, stream))
        first = (mb.indices.clone(), mb.p0.clone(), mb.A.clone())
        mb.resample(stream)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, (mb.indices, mb.p0, mb.A))), "the same call twice"
        assert (mb.c.kind, mb.c.p0, mb.c.p1, mb.c.s0, mb.c.s1) == (full.c.kind, mb.p0.data_ptr(), mb.A.data_ptr(), float(m), full.c.s1)
        seen.append(want)
    if m in (7, 33):
        assert (seen[1] != seen[2]).any() and (seen[0] != seen[1]).any()  # two streams differ; so do two seeds
    if m == R:
        assert all((s == np.arange(R)).all() for s in seen)


# ---- 2. buffers ----------------------------------------------------------------------------------------------------------------------
@F64
@pytest.mark.parametrize("m", mr.M_MAIN)
@pytest.mark.parametrize("kind", mr.KINDS)
def test_buffers_are_a_numpy_gather_bit_for_bit(nf, kind, m, f64):
    full = full_target(nf, kind, f64)
    mb = nf.MinibatchTarget(full, m, seed=11)
    for stream in (0, 3):
        mb.resample(stream)
        idx = mr.indices(R, m, 11, stream)
        p0, p1 = numpy_batch(nf, full, m, idx)
        assert_bits(mb.indices, idx.astype(np.int32), "idx")
        assert_bits(mb.p0, p0, f"p0 {kind} m={m}")
        assert_bits(mb.A, p1, f"p1 {kind} m={m}")
    if m < R and kind == "glm":  # the scale is in the weights: some stratum holds more than one row
        wt_full, n = host(full.p0)[D + R:D + 2 * R], mr.strata(R, m)[1]
        assert n.max() > 1 and np.array_equal(host(mb.p0)[D + m:D + 2 * m], wt_full[idx] * n.astype(wt_full.dtype))


@F64
@pytest.mark.parametrize("d,rows,m", mr.WIDTH_CASES)
def test_row_widths(nf, d, rows, m, f64):
    """d = 256: 16-byte accesses in both element types; d = 255: rows that are not 16-byte aligned take the scalar path"""
    full = mr.build_wide(nf, d, rows, tdt(f64), "cuda")
    mb = nf.MinibatchTarget(full, m, seed=2)
    for stream in (0, 1, 9):
        mb.resample(stream)
        idx = mr.indices(rows, m, 2, stream)
        p0, p1 = numpy_batch(nf, full, m, idx)
        assert_bits(mb.p0, p0, "p0")
        assert_bits(mb.A, p1, "p1")


# ---- 3. m = R is the full target -----------------------------------------------------------------------------------------------------
@F64
@pytest.mark.parametrize("kind", mr.KINDS)
def test_all_rows_give_the_full_buffers_and_the_full_logp(nf, kind, f64):
    full = full_target(nf, kind, f64)
    mb = nf.MinibatchTarget(full, R, seed=5).resample(17)
    assert torch.equal(mb.p0, full.p0) and torch.equal(mb.A, full.A)
    assert host(mb.p0).tobytes() == host(full.p0).tobytes() and host(mb.A).tobytes() == host(full.A).tobytes()
    ys = to_dev(sample_ys(full.d, 37, f64), f64)
    la, ga = nf.target_logp(full, ys, with_grad=True)
    lb, gb = nf.target_logp(mb, ys, with_grad=True)
    assert torch.equal(la, lb) and torch.equal(ga, gb) and bool(torch.isfinite(la).all())


def _train(nf, flow, target, n, iters=3, seed=9, **kw):
    f, stats, st = nf.train_flow(nf.PhiloxRNG(seed), nf.elbo_batch, flow, target, n, max_iters=iters, optimiser=nf.Adam(LR), **kw)
    torch.cuda.synchronize()
    return f.theta, st, [s["loss"] for s in stats]


@pytest.mark.parametrize("case", ["realnvp_f32", "realnvp_f64", "fullrank_f32"])
def test_three_training_steps_on_all_rows_are_the_full_targets(nf, case):
    f64 = case.endswith("f64")
    full = full_target(nf, "glm", f64)
    if case.startswith("realnvp"):
        flow = nf.realnvp(nf.MvNormal(D), (8, 8), 1, paramtype=tdt(f64), seed=2)  # one block: two couplings
    else:
        flow = nf.fullrank(nf.MvNormal(D), paramtype=tdt(f64))
    th_a, st_a, loss_a = _train(nf, flow, full, 64)
    th_b, st_b, loss_b = _train(nf, flow, nf.MinibatchTarget(full, R, seed=123), 64)
    assert torch.equal(th_a, th_b) and torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v) and st_a.t == st_b.t == 3
    assert loss_a == loss_b and all(np.isfinite(loss_a)) and not torch.equal(th_a, flow.theta)


# ---- 4. m < R ------------------------------------------------------------------------------------------------------------------------
@F64
def test_train_flow_resamples_with_the_step_index(nf, f64):
    """train_flow over a MinibatchTarget == resample(s) + nf_elbo_step on .c, s = 0, 1, 2, bit for bit"""
    from normalizingflows_jl_amd import objectives as ob

    full = full_target(nf, "glm", f64)
    flow = nf.realnvp(nf.MvNormal(D), (8, 8), 1, paramtype=tdt(f64), seed=2)
    mb = nf.MinibatchTarget(full, 33, seed=21)
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [mb, 64], nf.PhiloxRNG(9), None, {})
    th_a, st_a, loss_a = _train(nf, flow, mb, 64)
    mb2 = nf.MinibatchTarget(full, 33, seed=21)
    lib, ctx = nf.load_library(), flow.ctx
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    loss_b, batches = [], []
    for s in range(3):
        mb2.resample(s)
        batches.append(mb2.indices.clone())
        loss, gn = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(mb2.c), vp(th), vp(m), vp(v), 64, 9, s, LR, B1, B2, EPS, C.byref(loss),
                                       C.byref(gn)))
        loss_b.append(loss.value)
    torch.cuda.synchronize()
    assert torch.equal(th_a, th) and torch.equal(st_a.m, m) and torch.equal(st_a.v, v) and loss_a == loss_b
    assert torch.equal(mb.indices, mb2.indices) and not torch.equal(batches[0], batches[1]) and not torch.equal(batches[1], batches[2])
    # and not the full target's run: the batch is in the numbers
    th_full, _, _ = _train(nf, flow, full, 64)
    assert not torch.equal(th_full, th)


def test_the_generic_loop_resamples_once_per_gradient(nf):
    """an optimiser the fused loop does not take: optimize over value_and_gradient, the batch of the stream its draws are about to use"""
    full = full_target(nf, "glm", False)
    flow = nf.realnvp(nf.MvNormal(D), (8, 8), 1, paramtype=torch.float32, seed=2)
    mb = nf.MinibatchTarget(full, 7, seed=4)
    fa, _, _ = nf.train_flow(nf.PhiloxRNG(9), nf.elbo_batch, flow, mb, 64, max_iters=3, optimiser=nf.Descent(1e-3))
    mb2, rng = nf.MinibatchTarget(full, 7, seed=4), nf.PhiloxRNG(9)
    theta, re = flow.destructure()
    st = nf.setup(nf.Descent(1e-3), theta)
    for s in range(3):
        mb2.resample(s)
        assert rng.stream == s
        _, g = nf.value_and_gradient(nf.elbo_batch, re(theta), mb2, 64, rng)
        nf.update(nf.Descent(1e-3), st, theta, g)
    torch.cuda.synchronize()
    assert torch.equal(fa.theta, theta) and torch.equal(mb.indices, mb2.indices)
    assert_bits(mb.indices, mr.indices(R, 7, 4, 2).astype(np.int32), "the last step's batch")


@F64
@pytest.mark.parametrize("m", mr.M_MAIN)
@pytest.mark.parametrize("kind", mr.KINDS)
def test_logp_on_the_batch_matches_the_float64_form_on_the_gathered_rows(nf, kind, m, f64):
    """the kinds' own check (test_gpu_linpred.check_logp: the plain tolerance of tests/parity.py, with the float32 oracle's floor on
    the same array in Float32) against the kind's float64 form on rows gathered in numpy.  Measured: Float64 at most 8e-4 of the
    tolerance; Float32 45 of 48 rows inside the plain element-wise tolerance, three score rows above it on their worst element --
    dglm_normal m = 33 1.11x (floor 0.31x), dglm_negbin m = 7 1.30x (floor 3.2x), dglm_negbin m = 77 1.81x (floor 2.4x; m = R is the
    full target on the unchanged kernel) -- each with an rms of 0.08-0.17x."""
    full = full_target(nf, kind, f64)
    mb = nf.MinibatchTarget(full, m, seed=8).resample(2)
    p0, p1 = numpy_batch(nf, full, m, mr.indices(R, m, 8, 2))  # host copies of the FULL buffers, gathered in numpy
    check_logp(nf, f"minibatch logp {kind} m={m} {'f64' if f64 else 'f32'}", mb, ref_on(kind, full, p1, p0), sample_ys(full.d, 37, f64), f64)


# ---- 5. unbiasedness -----------------------------------------------------------------------------------------------------------------
def test_the_mean_over_all_batches_is_the_full_target(nf):
    """Float64 GLM, R = 6, m = 3: strata {0,1}, {2,3}, {4,5}, all 8 batches through indices=; the mean of log p and of the score over
    them equals the full target's to 1e-12 of the largest term"""
    rows, m, d, n = 6, 3, 4, 9
    rng = np.random.default_rng(31)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    full = nf.GLMTarget("poisson", t(rng.standard_normal((rows, d)) / 2), offset=t(0.2 * rng.standard_normal(rows)), weights=t(rng.uniform(0.5, 2, rows)),
                        lin=t(rng.standard_normal(d)), const=0.75, prior_sigma=1.5)
    ys = to_dev(sample_ys(d, n, True), True)
    lf, gf_ = nf.target_logp(full, ys, with_grad=True)
    mb = nf.MinibatchTarget(full, m)
    lps, grads = [], []
    for a in (0, 1):
        for b in (2, 3):
            for c in (4, 5):
                mb.resample(0, indices=[a, b, c])
                assert host(mb.indices).tolist() == [a, b, c]
                lp, g = nf.target_logp(mb, ys, with_grad=True)
                lps.append(lp.clone())
                grads.append(g.clone())
    lps, grads = torch.stack(lps), torch.stack(grads)
    for name, mean, want, terms in (("logp", lps.mean(0), lf, lps), ("score", grads.mean(0), gf_, grads)):
        scale = float(terms.abs().max())
        err = float((mean - want).abs().max()) / scale
        P.record(f"minibatch unbiasedness {name} [max abs err / largest term]", err)
        assert err <= 1e-12, (name, err)
    assert float((lps - lf).abs().max()) > 1e-3  # the batches do differ from the full target


# ---- 6. the closure route ------------------------------------------------------------------------------------------------------------
def test_planar_flow_takes_the_closure_route_on_the_current_batch(nf):
    from normalizingflows_jl_amd import objectives as ob

    full = full_target(nf, "glm", True)
    mb = nf.MinibatchTarget(full, 7, seed=6).resample(4)
    flow = nf.planarflow(nf.MvNormal(D), 4, paramtype=torch.float64, seed=3)
    flow = flow.with_theta(flow.theta * 0.3)
    assert not ob._builtin(flow, mb) and isinstance(mb, ob._LINPRED)
    p0 = mb.p0.clone()
    plain = nf.GLMTarget(full.family, mb.A.clone(), offset=p0[D:D + 7], weights=p0[D + 7:D + 14], lin=p0[:D], const=float(p0[D + 15]),
                         param=float(p0[D + 14]), prior_sigma=full.prior_sigma)
    assert torch.equal(plain.p0, mb.p0) and torch.equal(plain.A, mb.A)  # an equivalent plain target from the gathered buffers
    xs = to_dev(o.base_sample(D, 37, 77, 0, 0), True)
    la, ga = nf.value_and_gradient(nf.elbo_batch, flow, mb, xs)
    lb, gb = nf.value_and_gradient(nf.elbo_batch, flow, plain, xs)
    assert la == lb and torch.equal(ga, gb) and np.isfinite(la) and bool(ga.abs().max() > 0)
    lfull, _ = nf.value_and_gradient(nf.elbo_batch, flow, full, xs)
    assert lfull != la


# ---- the non-centring layer reads the full target's groups ---------------------------------------------------------------------------
def test_noncentred_over_the_full_targets_groups_trains_against_the_batch(nf):
    full = full_target(nf, "hglm", False)
    inner = nf.realnvp(nf.MvNormal(D), (8, 8), 1, paramtype=torch.float32, seed=2)
    with pytest.raises(nf.NFHipError, match="HierarchicalGLMTarget"):
        nf.noncentred(inner, nf.MinibatchTarget(full, 33))
    flow = nf.noncentred(inner, full, lam=0.5)
    xs = to_dev(o.base_sample(D, 64, 5, 0, 0), False)
    la, ga = nf.value_and_gradient(nf.elbo_batch, flow, full, xs)
    lb, gb = nf.value_and_gradient(nf.elbo_batch, flow, nf.MinibatchTarget(full, R), xs)
    assert la == lb and torch.equal(ga, gb)
    th, st, losses = _train(nf, flow, nf.MinibatchTarget(full, 33, seed=3), 64)
    assert all(np.isfinite(losses)) and bool(torch.isfinite(th).all()) and st.t == 3


# ---- 7. refusals and robustness ------------------------------------------------------------------------------------------------------
def _raw_call(nf, full, d, m, p0_out, p1_out, elems=None, f64=False):
    from normalizingflows_jl_amd._lib import Target, context_for

    ctx, out = context_for(torch.device("cuda:0")), Target(-7, 0, 0, -1.0, -1.0)
    code = nf.load_library().nf_target_minibatch(ctx.ptr, int(f64), C.byref(full.c), d, full.p0.numel() if elems is None else elems, m, 1, 0, None, None,
                                                 C.c_void_p(p0_out), C.c_void_p(p1_out), C.byref(out))
    assert code != 0 and (out.kind, out.p0, out.p1, out.s0, out.s1) == (-7, None, None, -1.0, -1.0)
    return code


def test_refusals_leave_the_outputs_untouched(nf):
    dt = torch.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
    rng = np.random.default_rng(3)
    X = rng.standard_normal((64, 3))
    lab = np.arange(64) % 2
    unsupported = [nf.MvNormalTarget(t(np.zeros(3)), t(np.eye(3))),                                        # 5
                   nf.LogisticRegressionTarget(t(X), t(lab)),                                              # 6
                   nf.MixtureTarget(t([0.5, 0.5]), t(rng.standard_normal((2, 3))), t(np.stack([np.eye(3)] * 2))),  # 8
                   nf.OrdinalRegressionTarget(t(X), torch.tensor(lab, device="cuda"), 2),                  # 32
                   nf.ConditionalLogitTarget(t(X), torch.tensor(np.arange(64) // 4, device="cuda"), torch.tensor(np.arange(64) % 4 == 0, device="cuda"))]  # 33
    assert [u.c.kind for u in unsupported] == [5, 6, 8, 32, 33]
    o0, o1 = torch.full((4096,), 7.0, dtype=dt, device="cuda"), torch.full((4096,), 7.0, dtype=dt, device="cuda")
    for u in unsupported:
        assert _raw_call(nf, u, 3, 1, o0.data_ptr(), o1.data_ptr(), elems=64) == NF_ERR_UNSUPPORTED, u.c.kind
        with pytest.raises(nf.NFHipError, match="row-minibatch"):
            nf.MinibatchTarget(u, 1)
    full = full_target(nf, "glm", False)
    before = (full.p0.clone(), full.A.clone())
    for m in (0, R + 1, -1):
        assert _raw_call(nf, full, D, m, o0.data_ptr(), o1.data_ptr()) == NF_ERR_ARG
    assert _raw_call(nf, full, D, 7, full.p0.data_ptr(), o1.data_ptr()) == NF_ERR_ARG  # aliased outputs
    assert _raw_call(nf, full, D, 7, o0.data_ptr(), full.A.data_ptr()) == NF_ERR_ARG
    for elems in (full.p0.numel() - 1, full.p0.numel() + 1, 0):
        assert _raw_call(nf, full, D, 7, o0.data_ptr(), o1.data_ptr(), elems=elems) == NF_ERR_ARG
    assert _raw_call(nf, full, D + 1, 7, o0.data_ptr(), o1.data_ptr()) == NF_ERR_ARG           # p0_elems is not the layout's at this d
    assert _raw_call(nf, full, D, 7, 0, o1.data_ptr()) == NF_ERR_ARG and _raw_call(nf, full, D, 7, o0.data_ptr(), 0) == NF_ERR_ARG
    torch.cuda.synchronize()
    assert bool((o0 == 7.0).all()) and bool((o1 == 7.0).all()) and torch.equal(full.p0, before[0]) and torch.equal(full.A, before[1])
    for bad in (0, R + 1):
        with pytest.raises(nf.NFHipError, match="batch_rows"):
            nf.MinibatchTarget(full, bad)
    with pytest.raises(nf.NFHipError, match="indices"):
        nf.MinibatchTarget(full, 7).resample(0, indices=[1, 2, 3])


@F64
def test_indices_outside_the_rows_are_bounded_by_select(nf, f64):
    full = full_target(nf, "dglm_negbin", f64)
    m = 7
    mb = nf.MinibatchTarget(full, m)
    given = [-5, 10**9, 3, -2**31, 2**31 - 1, 76, 0]
    mb.resample(0, indices=given)
    torch.cuda.synchronize()
    bounded = np.clip(np.asarray(given, dtype=np.int64), 0, R - 1)
    assert host(mb.indices).tolist() == bounded.tolist() == [0, 76, 3, 0, 76, 76, 0]
    p0, p1 = numpy_batch(nf, full, m, bounded)
    assert_bits(mb.p0, p0, "p0")
    assert_bits(mb.A, p1, "p1")
    assert torch.equal(mb.A[0], full.A[0]) and torch.equal(mb.A[1], full.A[R - 1])  # rows 0 and R - 1
    lp = nf.target_logp(mb, to_dev(sample_ys(full.d, 5, f64), f64))
    assert bool(torch.isfinite(lp).all())
