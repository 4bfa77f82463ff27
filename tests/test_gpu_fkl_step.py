"""GPU tests of the forward-KL training step (nf_loglikelihood_step, nf_loglikelihood_step_enqueue): one iteration of
train_flow(loglikelihood, flow, ys) -- value and gradient of -loglikelihood (src/objectives/loglikelihood.jl:26-33 inside the
loss closure of src/NormalizingFlows.jl:69), Adam and norm(g) -- in one call.  The reference for every number is the split
sequence nf_loglikelihood_value_and_grad + nf_adam_update on another context: theta, m and v must match it bit for bit."""
import ctypes as C

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from __graft_entry__ import load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
NF_ERR_ARG, NF_ERR_UNSUPPORTED, NF_ERR_NO_RCCL, NF_ERR_WORKSPACE = -1, -2, -5, -7


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def vp(t):
    return C.c_void_p(t.data_ptr())


def cm(a, dt):
    """d x N column-major device matrix (the library's batch layout)"""
    return torch.tensor(np.ascontiguousarray(a.T), dtype=dt, device="cuda").t()


SHAPES = {
    # name: (kind, d, hdims, nlayers, K, n)
    "d64_h64": ("realnvp", 64, (64, 64), 4, 0, 4101),
    "d20_h32": ("realnvp", 20, (32, 32), 2, 0, 777),
    "nsf_d32_k8": ("nsf", 32, (32, 32), 3, 8, 2055),
    "nsf_d9_k10": ("nsf", 9, (24, 32), 2, 10, 333),
}


def make(nf, shape, seed=3):
    kind, d, hd, nl, K, n = SHAPES[shape]
    if kind == "nsf":
        flow = nf.nsf(nf.MvNormal(d), hd, K, 5.0, nl, paramtype=torch.float32, seed=seed)
    else:
        flow = nf.realnvp(nf.MvNormal(d), hd, nl, paramtype=torch.float32, seed=seed)
    ys = np.random.default_rng(seed + d).standard_normal((d, n))
    return flow, cm(ys, torch.float32), n


def dcode(flow):
    return 0 if flow.theta.dtype == torch.float32 else 1


def split_steps(nf, flow, ys, n, nsteps, ctx, theta=None, first=0):
    """nsteps of nf_loglikelihood_value_and_grad + nf_adam_update on `ctx` (from `theta`, zero moments)"""
    lib = nf.load_library()
    dt = flow.theta.dtype
    th = (flow.theta if theta is None else theta).clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    out, gn = torch.empty(flow.P + 1, dtype=dt, device="cuda"), torch.empty(1, dtype=dt, device="cuda")
    stats = []
    for step in range(first, first + nsteps):
        nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx.ptr, C.byref(flow.desc), vp(th), vp(ys), n, n, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, dcode(flow), vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        stats.append((float(out[flow.P]), float(gn)))
    return th, m, v, stats


def fused_step(nf, ctx, flow, th, m, v, ys, n, step, want=True, n_global=None):
    lib = nf.load_library()
    loss, gn = C.c_double(0), C.c_double(0)
    nf._lib.check(lib.nf_loglikelihood_step(ctx.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(ys), n, n if n_global is None else n_global,
                                            step, LR, B1, B2, EPS, C.byref(loss) if want else None, C.byref(gn) if want else None))
    return loss.value, gn.value


def new_ctx(nf):
    return nf.Context(0, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_equals_split_calls_over_consecutive_steps(nf, shape, cache):
    """Five steps against the split calls: theta, m, v bit for bit, loss and norm(g) to float rounding (steps 2-4 without a
    host readback).  Then an in-place edit of theta: declared with nf_ctx_weights_changed under the weight cache, undeclared
    without it -- either way the next step runs on the edited weights."""
    lib = nf.load_library()
    flow, ys, n = make(nf, shape)
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    if cache:
        nf._lib.check(lib.nf_ctx_set_weight_cache(ctx_a.ptr, 1))
    th_b, m_b, v_b, stats_b = split_steps(nf, flow, ys, n, 5, ctx_b)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(5):
        want = step in (0, 4)
        loss, gn = fused_step(nf, ctx_a, flow, th, m, v, ys, n, step, want)
        if want:
            assert loss == pytest.approx(stats_b[step][0], rel=1e-6)
            assert gn == pytest.approx(stats_b[step][1], rel=1e-6)
    torch.cuda.synchronize()
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    th.mul_(0.5)
    if cache:
        nf._lib.check(lib.nf_ctx_weights_changed(ctx_a.ptr))
    fused_step(nf, ctx_a, flow, th, m, v, ys, n, 5, want=False)
    th_c, m_c, v_c = th_b * 0.5, m_b.clone(), v_b.clone()
    out, gnd = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx_b.ptr, C.byref(flow.desc), vp(th_c), vp(ys), n, n, vp(out)))
    nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_c), vp(out), vp(m_c), vp(v_c), flow.P, LR, B1, B2, EPS, 6, vp(gnd)))
    torch.cuda.synchronize()
    assert torch.equal(th, th_c) and torch.equal(m, m_c) and torch.equal(v, v_c)
    ctx_a.close()
    ctx_b.close()


def test_stash_budget_chunks_the_batch(nf):
    """A 1.5 MB stash budget forces chunks of 128 samples: bit for bit the split calls under the same budget, and the
    gradient (Adam's first moment after one step is 0.1 g) equal to the one-chunk run up to float32 summation order."""
    lib = nf.load_library()
    flow, ys, n = make(nf, "d64_h64")
    ctx_a, ctx_b, ctx_c = new_ctx(nf), new_ctx(nf), new_ctx(nf)
    budget = 3 * (1 << 19)
    for c in (ctx_a, ctx_b):
        nf._lib.check(lib.nf_ctx_set_stash_budget(c.ptr, budget))
    th_b, m_b, v_b, stats_b = split_steps(nf, flow, ys, n, 2, ctx_b)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(2):
        loss, gn = fused_step(nf, ctx_a, flow, th, m, v, ys, n, step)
        assert loss == pytest.approx(stats_b[step][0], rel=1e-6) and gn == pytest.approx(stats_b[step][1], rel=1e-6)
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    th1, m1, v1 = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    th2, m2, v2 = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    l1, g1 = fused_step(nf, ctx_a, flow, th1, m1, v1, ys, n, 0)
    l2, g2 = fused_step(nf, ctx_c, flow, th2, m2, v2, ys, n, 0)
    assert l1 == pytest.approx(l2, rel=1e-6) and g1 == pytest.approx(g2, rel=1e-5)
    assert float((m1 - m2).abs().max()) <= 1e-5 * float(m2.abs().max())
    for c in (ctx_a, ctx_b, ctx_c):
        c.close()


@pytest.mark.parametrize("shape", ["d20_h32", "d64_h64"])
def test_first_step_against_the_oracle(nf, shape):
    """Step-1 loss against oracle.nf_oracle.neg_loglik_value_and_grad, the gradient (Adam's m / (1 - beta1)) at the plain
    gradient tolerance, and theta after the step against a float64 host Adam on the oracle gradient."""
    kind, d, hd, nl, K, n = SHAPES[shape]
    flow, ys, n = make(nf, shape)
    n = min(n, 777)
    ys = ys[:, :n]
    ys = cm(ys.cpu().numpy(), torch.float32)
    spec = o.FlowSpec(kind, d, nl, hd)
    th64 = flow.theta.double().cpu().numpy()
    ys64 = ys.double().cpu().numpy()
    lo, go = o.neg_loglik_value_and_grad(spec, th64, ys64)
    _, g32 = o.neg_loglik_value_and_grad(spec, P.f32(th64), P.f32(ys64))
    ctx = new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    loss, _ = fused_step(nf, ctx, flow, th, m, v, ys, n, 0)
    P.scalar(f"fkl step {shape}: loss", loss, lo)
    P.gradient(f"fkl step {shape}: grad (m / (1 - beta1))", m.double().cpu().numpy() / (1 - B1), go, floor=g32)
    # float64 Adam, t = 1: theta - lr * mhat / (sqrt(vhat) + eps) with mhat = g, vhat = g^2
    th_ref = th64 - LR * go / (np.sqrt(go * go) + EPS)
    big = np.abs(go) > 1e-2 * np.abs(go).max()  # where |g| is far above its error the step's sign and size are fixed
    got = th.double().cpu().numpy()
    err = np.abs(got - th_ref)[big].max()
    assert np.all(np.abs(got - th_ref)[big] <= 4 * 2.0**-24 * np.abs(th64[big]) + P.GRAD_RTOL * LR), err
    ctx.close()


@pytest.mark.parametrize("shape", ["d64_h64", "nsf_d32_k8", "nsf_d9_k10"])
def test_step_with_device_counter_replays_as_a_graph(nf, shape):
    """nf_loglikelihood_step_enqueue captured once into a hipGraph and replayed five times: the eager split calls' theta,
    the device counter advanced by one per replay, [loss ; norm] of the last step in out_loss_gnorm_device -- the RealNVP
    and the spline forms."""
    lib = nf.load_library()
    flow, ys, n = make(nf, shape)
    ctx_b = new_ctx(nf)
    th_b, m_b, v_b, stats_b = split_steps(nf, flow, ys, n, 6, ctx_b)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    stat = torch.zeros(2, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    ctx_a = nf.Context(0, side.cuda_stream)

    def enqueue():
        nf._lib.check(lib.nf_loglikelihood_step_enqueue(ctx_a.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(ys), n, n, vp(counter),
                                                        LR, B1, B2, EPS, vp(stat)))

    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()  # step 0, eager: sizes the workspace, sets kernel attributes, packs the weights
    side.synchronize()
    assert int(counter[0]) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue()  # captured, not executed
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert int(counter[0]) == 6
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    assert float(stat[0]) == pytest.approx(stats_b[5][0], rel=1e-6) and float(stat[1]) == pytest.approx(stats_b[5][1], rel=1e-6)
    ctx_a.close()
    ctx_b.close()


def _fallback_flow(nf, name):
    if name == "realnvp_f64":
        return nf.realnvp(nf.MvNormal(5), (32, 32), 2, paramtype=torch.float64, seed=2), 97
    if name == "planar":
        f = nf.planarflow(nf.MvNormal(6), 5, paramtype=torch.float32, seed=2)
        return f.with_theta(f.theta * 0.3), 500
    if name == "nsf_k10_d32":  # the K = 10, d <= 32 spline geometry has no forward-KL chain kernel (its chain kernels spill)
        return nf.nsf(nf.MvNormal(32), (32, 32), 10, 5.0, 1, paramtype=torch.float32, seed=2), 300
    if name == "composite":
        q0 = nf.MvNormal(16)
        segs = [nf.planarflow(q0, 2, paramtype=torch.float32, seed=1), nf.realnvp(q0, (32, 32), 1, paramtype=torch.float32, seed=2),
                nf.radialflow(q0, 2, paramtype=torch.float32, seed=3)]
        segs = [segs[0].with_theta(segs[0].theta * 0.3), segs[1], segs[2].with_theta(segs[2].theta * 0.3)]
        return nf.create_flow(segs, q0), 300
    return nf.realnvp(nf.MvNormal(64), (64,), 2, paramtype=torch.float32, seed=2), 1000  # deep RealNVP: no stash


@pytest.mark.parametrize("name", ["realnvp_f64", "planar", "composite", "deep_h64", "nsf_k10_d32"])
def test_flows_without_the_fused_form_run_the_split_sequence(nf, name):
    """Float64, planar, a composite, a one-hidden-layer RealNVP and the K = 10, d = 32 spline geometry: nf_loglikelihood_step
    equals the split calls bit for bit; the graph-capturable form refuses them with NF_ERR_UNSUPPORTED."""
    lib = nf.load_library()
    flow, n = _fallback_flow(nf, name)
    dt, d = flow.theta.dtype, flow.dist.d
    ys = cm(np.random.default_rng(7).standard_normal((d, n)), dt)
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th_b, m_b, v_b, stats_b = split_steps(nf, flow, ys, n, 2, ctx_b)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(2):
        loss, gn = fused_step(nf, ctx_a, flow, th, m, v, ys, n, step)
        assert loss == stats_b[step][0] and gn == stats_b[step][1]
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = lib.nf_loglikelihood_step_enqueue(ctx_a.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(ys), n, n, vp(counter), LR, B1, B2, EPS,
                                           None)
    assert st == NF_ERR_UNSUPPORTED
    ctx_a.close()
    ctx_b.close()


def _launches(nf, ctx, run):
    lib = nf.load_library()
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
    run()
    torch.cuda.synchronize()
    counts = {}
    for name in ("layout_convert", "target", "reduce_slabs", "adam", "pack_weights", "affine_chain", "affine_chain_fkl", "affine_bwd_inv",
                 "rqs_chain", "rqs_chain_fkl", "rqs_bwd_inv"):
        a, c = C.c_double(0.0), C.c_int64(0)
        lib.nf_prof_read(ctx.ptr, name.encode(), C.byref(a), C.byref(c))
        counts[name] = c.value
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
    return counts


def test_fused_realnvp_step_launches(nf):
    """The fused RealNVP step: no layout conversion, no separate target launch, no Adam launch, and the slab reduction only
    inside the fused epilogue (one launch, profiled under "reduce_slabs" like nf_elbo_step's) -- one forward-KL chain launch
    and one reverse launch per stash chunk.  The split calls, for contrast, run all of them."""
    lib = nf.load_library()
    flow, ys, n = make(nf, "d64_h64")
    ctx = new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    fused_step(nf, ctx, flow, th, m, v, ys, n, 0)  # warm-up (workspace, attributes)
    got = _launches(nf, ctx, lambda: fused_step(nf, ctx, flow, th, m, v, ys, n, 1, want=False))
    packs = got.pop("pack_weights")  # the pack from theta (+ the reverse kernel's derived images)
    assert got == {"layout_convert": 0, "target": 0, "reduce_slabs": 1, "adam": 0, "affine_chain": 0, "affine_chain_fkl": 1,
                   "affine_bwd_inv": 1, "rqs_chain": 0, "rqs_chain_fkl": 0, "rqs_bwd_inv": 0}, got
    nf._lib.check(lib.nf_ctx_set_weight_cache(ctx.ptr, 1))
    fused_step(nf, ctx, flow, th, m, v, ys, n, 2, want=False)
    got = _launches(nf, ctx, lambda: fused_step(nf, ctx, flow, th, m, v, ys, n, 3, want=False))
    assert got["pack_weights"] == packs - 1 and got["affine_chain_fkl"] == 1, got  # the cache: no pack from theta
    nf._lib.check(lib.nf_ctx_set_weight_cache(ctx.ptr, 0))
    nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, 3 * (1 << 19)))
    got = _launches(nf, ctx, lambda: fused_step(nf, ctx, flow, th, m, v, ys, n, 4, want=False))
    chunks = (n + 127) // 128
    assert got["affine_chain_fkl"] == chunks and got["affine_bwd_inv"] == chunks and got["layout_convert"] == 0, got
    nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, -1))
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")

    def split():
        nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx.ptr, C.byref(flow.desc), vp(th), vp(ys), n, n, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, 0, vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, 6, vp(gn)))

    got = _launches(nf, ctx, split)
    assert got["layout_convert"] == 1 and got["target"] == 1 and got["adam"] == 1 and got["affine_chain_fkl"] == 0, got
    ctx.close()


@pytest.mark.parametrize("shape", ["nsf_d32_k8", "nsf_d9_k10"])
def test_fused_spline_step_launches(nf, shape):
    """The fused spline step: one forward-KL chain launch (ys read in place), one inverse-direction reverse launch per
    coupling, the fused epilogue (profiled under "reduce_slabs") -- no layout conversion, target, plain chain or Adam launch.
    The split calls, for contrast, run all of them."""
    lib = nf.load_library()
    flow, ys, n = make(nf, shape)
    ncoup = 2 * SHAPES[shape][3]
    ctx = new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    fused_step(nf, ctx, flow, th, m, v, ys, n, 0)
    got = _launches(nf, ctx, lambda: fused_step(nf, ctx, flow, th, m, v, ys, n, 1, want=False))
    got.pop("pack_weights")
    assert got == {"layout_convert": 0, "target": 0, "reduce_slabs": 1, "adam": 0, "affine_chain": 0, "affine_chain_fkl": 0,
                   "affine_bwd_inv": 0, "rqs_chain": 0, "rqs_chain_fkl": 1, "rqs_bwd_inv": ncoup}, got
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")

    def split():
        nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx.ptr, C.byref(flow.desc), vp(th), vp(ys), n, n, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, 0, vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, 3, vp(gn)))

    got = _launches(nf, ctx, split)
    assert got["layout_convert"] == 1 and got["target"] == 1 and got["adam"] == 1 and got["rqs_chain"] == 1, got
    assert got["rqs_chain_fkl"] == 0 and got["rqs_bwd_inv"] == ncoup, got
    ctx.close()


@pytest.mark.parametrize("shape", ["d64_h64", "nsf_d32_k8"])
def test_caller_arena_runs_both_calls(nf, shape):
    """An arena of nf_workspace_bytes(desc, N) runs both calls with the owned mode's bits; a batch twice as large is
    refused with NF_ERR_WORKSPACE instead of allocating.  (Not N + 32 columns: nf_workspace_bytes is the maximum over EVERY
    entry point at N, and the fused step needs less than nf_loglikelihood_value_and_grad -- which keeps z, ladj and its own
    seed buffer -- so at N + 32 it still fits that arena legitimately; twice the batch exceeds it.)"""
    lib = nf.load_library()
    flow, ys, n = make(nf, shape)
    d = SHAPES[shape][1]
    n = 1000
    big = cm(np.random.default_rng(1).standard_normal((d, 2 * n)), torch.float32)
    ys = big[:, :n]
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(ctx):
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        fused_step(nf, ctx, flow, th, m, v, ys, n, 0)
        counter.fill_(1)
        nf._lib.check(lib.nf_loglikelihood_step_enqueue(ctx.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(ys), n, n, vp(counter),
                                                        LR, B1, B2, EPS, None))
        torch.cuda.synchronize()
        return th, m, v

    ctx_ref = new_ctx(nf)
    ref = run(ctx_ref)
    ctx = new_ctx(nf)
    need = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), n))
    arena = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    base = (arena.data_ptr() + 255) // 256 * 256
    try:
        nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, C.c_void_p(base), need))
        got = run(ctx)
        assert all(torch.equal(a, b) for a, b in zip(ref, got))
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        st = lib.nf_loglikelihood_step(ctx.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(big), 2 * n, 2 * n, 0, LR, B1, B2, EPS,
                                       None, None)
        assert st == NF_ERR_WORKSPACE
        st = lib.nf_loglikelihood_step_enqueue(ctx.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(big), 2 * n, 2 * n, vp(counter),
                                               LR, B1, B2, EPS, None)
        assert st == NF_ERR_WORKSPACE
        assert torch.equal(th, flow.theta)
    finally:
        nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, None, 0))
    ctx.close()
    ctx_ref.close()


@pytest.mark.parametrize("kind", ["realnvp_resident", "planar"])
def test_train_flow_loglikelihood_runs_one_library_call_per_iteration(nf, kind, monkeypatch):
    """train_flow(loglikelihood, flow, xs) with Adam: one nf_loglikelihood_step per iteration (no value_and_grad, no
    separate Adam), theta and Adam state bit for bit those of `optimize` over loglikelihood_value_and_gradient + update,
    the stats to rounding, the callback seeing the parameters before the update; continued from the returned state."""
    from normalizingflows_jl_amd import objectives as ob

    if kind == "realnvp_resident":
        flow = nf.realnvp(nf.MvNormal(64), (64, 64), 2, paramtype=torch.float32, seed=5)
    else:
        flow = nf.planarflow(nf.MvNormal(6), 5, paramtype=torch.float32, seed=5)
        flow = flow.with_theta(flow.theta * 0.3)
    d, n = flow.dist.d, 1000
    xs = cm(np.random.default_rng(0).standard_normal((d, n)), torch.float32)
    seen = []

    def cb(i, stats, re, theta):
        seen.append(theta.clone())
        return {"extra": i}

    assert ob._fused_fkl_steps_apply(nf.loglikelihood, flow, [xs], None, {})
    assert not ob._fused_fkl_steps_apply(nf.loglikelihood, flow, [xs], nf.Descent(0.1), {})
    assert not ob._fused_fkl_steps_apply(nf.loglikelihood, flow, [xs], None, {"all_reduce": lambda b: None})
    lib = flow.ctx.lib
    calls = {"nf_loglikelihood_step": 0, "nf_loglikelihood_value_and_grad": 0, "nf_adam_update": 0}
    for name in calls:
        fn = getattr(lib, name)

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)

        monkeypatch.setattr(lib, name, counted)
    fa, sa, sta = nf.train_flow(nf.loglikelihood, flow, xs, max_iters=6, optimiser=nf.Adam(2e-3), callback=cb)
    assert calls == {"nf_loglikelihood_step": 6, "nf_loglikelihood_value_and_grad": 0, "nf_adam_update": 0}, calls
    monkeypatch.undo()
    seen_a, seen = seen, []
    theta0, re = flow.destructure()
    tb, sb, stb = nf.optimize(lambda th: nf.loglikelihood_value_and_gradient(re(th), xs), theta0, re, max_iters=6,
                              optimiser=nf.Adam(2e-3), callback=cb)
    assert torch.equal(fa.theta, tb) and torch.equal(sta.m, stb.m) and torch.equal(sta.v, stb.v) and sta.t == stb.t == 6
    for a, b in zip(sa, sb):
        assert a["iteration"] == b["iteration"] and a["extra"] == b["extra"]
        assert a["loss"] == pytest.approx(b["loss"], rel=1e-6) and a["gradient_norm"] == pytest.approx(b["gradient_norm"], rel=1e-6)
    assert all(torch.equal(x, y) for x, y in zip(seen_a, seen)) and torch.equal(seen_a[0], theta0)
    f3, _, st3 = nf.train_flow(nf.loglikelihood, flow, xs, max_iters=3, optimiser=nf.Adam(2e-3))
    f33, _, st33 = nf.train_flow(nf.loglikelihood, f3, xs, max_iters=100, optimiser=nf.Adam(2e-3), state=st3,
                                 hasconverged=lambda i, stat, re, th, st: st.t >= 6)
    assert st33.t == 6 and torch.equal(f33.theta, tb)
    # the one-step wrapper
    f1 = flow.with_theta(flow.theta.clone())
    st1 = nf.setup(nf.Adam(2e-3), f1.theta)
    for _ in range(6):
        nf.loglikelihood_step(f1, xs, nf.Adam(2e-3), st1)
    assert st1.t == 6 and torch.equal(f1.theta, tb)


def test_communicator_of_one_rank(nf):
    """nf_comm_init_all with one context: the step under the communicator (N_global <= 0 resolves to N_local * 1) equals
    the step without one bit for bit.  (The split epilogue around the all-reduce needs more than one rank.)"""
    lib = nf.load_library()
    flow, ys, n = make(nf, "d20_h32")
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    arr = (C.c_void_p * 1)(ctx_a.ptr)
    st = lib.nf_comm_init_all(arr, 1)
    if st == NF_ERR_NO_RCCL:
        ctx_a.close()
        ctx_b.close()
        pytest.skip("librccl.so.1 is not available")
    nf._lib.check(st)
    try:
        assert lib.nf_comm_size(ctx_a.ptr) == 1
        res = []
        for ctx, ng in ((ctx_a, 0), (ctx_b, n)):
            th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
            stats = [fused_step(nf, ctx, flow, th, m, v, ys, n, s, n_global=ng) for s in range(3)]
            res.append((th, m, v, stats))
        assert all(torch.equal(a, b) for a, b in zip(res[0][:3], res[1][:3]))
        assert res[0][3] == res[1][3]
    finally:
        nf._lib.check(lib.nf_comm_destroy(ctx_a.ptr))
        ctx_a.close()
        ctx_b.close()
