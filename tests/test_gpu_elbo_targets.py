"""GPU tests of the fused ELBO step on the Banana, Funnel, WarpedGauss and Cross targets (k_affine_chain_tgt, k_rqs_chain_tgt)
and of the reverse-KL graph form of spline couplings: nf_elbo_step / nf_elbo_step_enqueue / nf_elbo_value_and_grad /
nf_elbo_batch_rng on the two LDS-resident coupling families.  The reference for bits is the split sequence
nf_elbo_value_and_grad + nf_adam_update on another context; the reference for values is the float64 oracle on the regenerated
in-library draws, at tests/parity.py's tolerances."""
import ctypes as C

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from __graft_entry__ import load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
NF_ERR_ARG, NF_ERR_UNSUPPORTED, NF_ERR_NO_RCCL = -1, -2, -5
# every launch name the step may be profiled under; the new forward kernels have names of their own
PROF_NAMES = ("layout_convert", "target", "reduce_slabs", "adam", "base_sample", "affine_chain", "affine_chain_tgt", "rqs_chain",
              "rqs_chain_tgt", "affine_bwd", "rqs_bwd")


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def vp(t):
    return C.c_void_p(t.data_ptr())


def new_ctx(nf):
    return nf.Context(0, torch.cuda.current_stream().cuda_stream)


def make_flow(nf, kind, d, hd, nl, K=0, seed=3):
    if kind == "nsf":
        return nf.nsf(nf.MvNormal(d), hd, K, 5.0, nl, paramtype=torch.float32, seed=seed)
    return nf.realnvp(nf.MvNormal(d), hd, nl, paramtype=torch.float32, seed=seed)


def make_target(nf, name, d):
    """(device target, oracle target tuple)"""
    if name == "banana":
        return nf.BananaTarget(d, 1.0, 100.0), ("banana", 1.0, 100.0)
    if name == "banana_b03":
        return nf.BananaTarget(d, 0.3, 4.0), ("banana", 0.3, 4.0)
    if name == "funnel":
        return nf.FunnelTarget(d, 0.3, 2.0), ("funnel", 0.3, 2.0)
    if name == "warped":
        return nf.WarpedGaussTarget(1.0, 0.12), ("warped", 1.0, 0.12)
    if name == "cross":
        return nf.CrossTarget(2.0, 0.15), ("cross", 2.0, 0.15)
    rng = np.random.default_rng(0)
    mu, var = rng.standard_normal(d).astype(np.float32), (rng.uniform(size=d) + 0.5).astype(np.float32)
    return nf.DiagGaussTarget(torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda")), ("diaggauss", mu.astype(np.float64), var.astype(np.float64))


def split_steps(nf, flow, tgt, n, seed, nsteps, ctx):
    """nsteps of nf_elbo_value_and_grad + nf_adam_update (tests/test_gpu_tape.py::_split_reference_steps)"""
    lib = nf.load_library()
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    stats = []
    for step in range(nsteps):
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, 0, vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        stats.append((float(out[flow.P]), float(gn)))
    return th, m, v, stats


def one_call_step(nf, ctx, flow, tgt, th, m, v, n, seed, step, want=True):
    lib = nf.load_library()
    loss, gn = C.c_double(0), C.c_double(0)
    nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS,
                                   C.byref(loss) if want else None, C.byref(gn) if want else None))
    return loss.value, gn.value


def launches(nf, ctx, run):
    lib = nf.load_library()
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
    run()
    torch.cuda.synchronize()
    counts = {}
    for name in PROF_NAMES:
        a, c = C.c_double(0.0), C.c_int64(0)
        lib.nf_prof_read(ctx.ptr, name.encode(), C.byref(a), C.byref(c))
        counts[name] = c.value
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
    return counts


# ---- 1. the graph form exists ----------------------------------------------------------------------------------------------
GRAPH_CASES = {
    # name: (kind, d, hdims, nlayers, K, target, n)
    "realnvp_d2_banana": ("realnvp", 2, (16, 16), 3, 0, "banana", 16),
    "nsf_d9_k10_funnel": ("nsf", 9, (24, 32), 2, 10, "funnel", 333),
    "nsf_d32_k8_diaggauss": ("nsf", 32, (32, 32), 3, 8, "diaggauss", 2055),
}


@pytest.mark.parametrize("case", list(GRAPH_CASES))
def test_step_with_device_counter_replays_as_a_graph(nf, case):
    """nf_elbo_step_enqueue on a RealNVP flow with the Banana target and on spline flows (Funnel; the diagonal Gaussian: the
    spline graph form by itself) returns 0, is captured once after one eager call and replayed five times: theta and m of
    the eager split calls bit for bit, the device counter at 6, [loss ; norm(g)] of the last step to float rounding."""
    kind, d, hd, nl, K, tname, n = GRAPH_CASES[case]
    flow = make_flow(nf, kind, d, hd, nl, K)
    tgt, _ = make_target(nf, tname, d)
    lib = nf.load_library()
    ctx_b = new_ctx(nf)
    th_b, m_b, v_b, stats_b = split_steps(nf, flow, tgt, n, 5, 6, ctx_b)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    stat = torch.zeros(2, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    ctx_a = nf.Context(0, side.cuda_stream)

    def enqueue():
        st = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 5, vp(counter),
                                      LR, B1, B2, EPS, vp(stat))
        assert st == 0, st

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
    assert torch.equal(th, th_b) and torch.equal(m, m_b)
    assert float(stat[0]) == pytest.approx(stats_b[5][0], rel=1e-6) and float(stat[1]) == pytest.approx(stats_b[5][1], rel=1e-6)
    ctx_a.close()
    ctx_b.close()


# ---- 2. launch structure ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["banana", "funnel", "warped", "cross"])
def test_fused_realnvp_step_launches(nf, tname):
    """One nf_elbo_step on a stashing RealNVP flow: no target, Adam, sampler or layout-conversion launch, the slab reduction
    only inside the fused epilogue, exactly one k_affine_chain_tgt launch and one reverse launch per stash chunk -- and no
    launch of the diagonal-Gaussian forward.  (Several chunks: test_step_equals_split_calls_in_stash_chunks.)"""
    lib = nf.load_library()
    d = 2 if tname in ("warped", "cross") else 20
    flow = make_flow(nf, "realnvp", d, (32, 32), 2)
    tgt, _ = make_target(nf, tname, d)
    n = 777
    ctx = new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    one_call_step(nf, ctx, flow, tgt, th, m, v, n, 77, 0)  # warm-up (workspace, attributes)
    got = launches(nf, ctx, lambda: one_call_step(nf, ctx, flow, tgt, th, m, v, n, 77, 1, want=False))
    assert got == {"layout_convert": 0, "target": 0, "reduce_slabs": 1, "adam": 0, "base_sample": 0, "affine_chain": 0,
                   "affine_chain_tgt": 1, "rqs_chain": 0, "rqs_chain_tgt": 0, "affine_bwd": 1, "rqs_bwd": 0}, got
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")

    def split():
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), None, n, n, 77, 0, 2, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, 0, vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, 3, vp(gn)))

    got = launches(nf, ctx, split)  # the split calls share the forward, and run the reduction and Adam as launches of their own
    assert got["affine_chain_tgt"] == 1 and got["target"] == 0 and got["adam"] == 1 and got["affine_chain"] == 0, got
    ctx.close()


@pytest.mark.parametrize("tname", ["banana", "funnel", "warped", "cross"])
def test_fused_spline_step_launches(nf, tname):
    """The spline step likewise: one k_rqs_chain_tgt launch, one reverse launch per coupling, the fused epilogue."""
    d, nl = (2, 2) if tname in ("warped", "cross") else (32, 3)
    flow = make_flow(nf, "nsf", d, (32, 32), nl, 8)
    tgt, _ = make_target(nf, tname, d)
    n = 519
    ctx = new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    one_call_step(nf, ctx, flow, tgt, th, m, v, n, 77, 0)
    got = launches(nf, ctx, lambda: one_call_step(nf, ctx, flow, tgt, th, m, v, n, 77, 1, want=False))
    assert got == {"layout_convert": 0, "target": 0, "reduce_slabs": 1, "adam": 0, "base_sample": 0, "affine_chain": 0,
                   "affine_chain_tgt": 0, "rqs_chain": 0, "rqs_chain_tgt": 1, "affine_bwd": 0, "rqs_bwd": 2 * nl}, got
    ctx.close()


# ---- 4. bit for bit against the split calls ----------------------------------------------------------------------------------
BIT_FLOWS = {
    # name: (kind, d, hdims, nlayers, K, n)
    "realnvp_d64_h64_nl4": ("realnvp", 64, (64, 64), 4, 0, 4101),
    "realnvp_d20_h32_nl2": ("realnvp", 20, (32, 32), 2, 0, 777),
    "nsf_d32_k8_nl3": ("nsf", 32, (32, 32), 3, 8, 2055),
    "realnvp_d2_h32": ("realnvp", 2, (32, 32), 2, 0, 515),
    "nsf_d2_k8": ("nsf", 2, (32, 32), 2, 8, 515),
}
BIT_CASES = [(f, t) for f in ("realnvp_d64_h64_nl4", "realnvp_d20_h32_nl2", "nsf_d32_k8_nl3") for t in ("banana", "funnel")] + \
            [(f, t) for f in ("realnvp_d2_h32", "nsf_d2_k8") for t in ("warped", "cross")]


def _five_steps_equal_split(nf, flow, tgt, n, cache, prepare=None):
    lib = nf.load_library()
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    keep = [prepare(c) for c in (ctx_a, ctx_b)] if prepare else None
    if cache:
        nf._lib.check(lib.nf_ctx_set_weight_cache(ctx_a.ptr, 1))
    th_b, m_b, v_b, stats_b = split_steps(nf, flow, tgt, n, 77, 5, ctx_b)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(5):
        want = step in (0, 4)  # steps 1..3 without a host readback
        loss, gn = one_call_step(nf, ctx_a, flow, tgt, th, m, v, n, 77, step, want)
        if want:
            assert loss == pytest.approx(stats_b[step][0], rel=1e-6)
            assert gn == pytest.approx(stats_b[step][1], rel=1e-6)
    torch.cuda.synchronize()
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    assert bool(torch.isfinite(th).all())
    if prepare:
        for c in (ctx_a, ctx_b):
            nf._lib.check(lib.nf_ctx_set_arena(c.ptr, None, 0))
    del keep
    ctx_a.close()
    ctx_b.close()


@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("fname,tname", BIT_CASES)
def test_step_equals_split_calls_over_consecutive_steps(nf, fname, tname, cache):
    """Five consecutive nf_elbo_step calls against nf_elbo_value_and_grad + nf_adam_update on another context: theta, m, v
    bit for bit, loss and norm(g) to float rounding; with and without the weight cache."""
    kind, d, hd, nl, K, n = BIT_FLOWS[fname]
    flow = make_flow(nf, kind, d, hd, nl, K)
    tgt, _ = make_target(nf, tname, d)
    _five_steps_equal_split(nf, flow, tgt, n, cache)


@pytest.mark.parametrize("tname", ["banana", "funnel"])
def test_step_equals_split_calls_in_stash_chunks(nf, tname):
    """The d = 64 case under a 1.5 MB stash budget (chunks of 128 samples): both sides run the per-chunk launches."""
    kind, d, hd, nl, K, n = BIT_FLOWS["realnvp_d64_h64_nl4"]
    flow = make_flow(nf, kind, d, hd, nl, K)
    tgt, _ = make_target(nf, tname, d)
    lib = nf.load_library()

    def prepare(ctx):
        nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, 3 << 19))

    ctx = new_ctx(nf)
    prepare(ctx)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    one_call_step(nf, ctx, flow, tgt, th, m, v, n, 77, 0)
    got = launches(nf, ctx, lambda: one_call_step(nf, ctx, flow, tgt, th, m, v, n, 77, 1, want=False))
    assert got["affine_chain_tgt"] == (n + 127) // 128 and got["target"] == 0, got
    ctx.close()
    _five_steps_equal_split(nf, flow, tgt, n, False, prepare)


@pytest.mark.parametrize("fname,tname", [("realnvp_d64_h64_nl4", "banana"), ("nsf_d32_k8_nl3", "funnel")])
def test_step_equals_split_calls_inside_a_caller_arena(nf, fname, tname):
    """Both contexts on a caller arena of nf_workspace_bytes(desc, N): enough for the new route, nothing allocated."""
    kind, d, hd, nl, K, n = BIT_FLOWS[fname]
    flow = make_flow(nf, kind, d, hd, nl, K)
    tgt, _ = make_target(nf, tname, d)
    lib = nf.load_library()

    def prepare(ctx):
        need = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), n))
        arena = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
        nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, C.c_void_p((arena.data_ptr() + 255) // 256 * 256), need))
        return arena

    _five_steps_equal_split(nf, flow, tgt, n, False, prepare)


# ---- 5. parity against the float64 oracle ----------------------------------------------------------------------------------
ORACLE_CASES = {
    # name: (kind, d, hdims, nlayers, K, B, target, n, init seed)
    "realnvp_d2_h16_nl3_banana": ("realnvp", 2, (16, 16), 3, 0, 0.0, "banana", 16, 3),
    "realnvp_d20_h32_nl2_funnel": ("realnvp", 20, (32, 32), 2, 0, 0.0, "funnel", 777, 3),
    "realnvp_d2_h32_nl2_warped": ("realnvp", 2, (32, 32), 2, 0, 0.0, "warped", 515, 3),
    "realnvp_d2_h64_nl2_cross": ("realnvp", 2, (64, 64), 2, 0, 0.0, "cross", 515, 3),
    # init seed 3 puts one leaky-ReLU kink inside the float32 rounding of this flow (float32 oracle alone: 1.27e-4); seed 5 does not
    "realnvp_d64_h64_nl4_banana_b03": ("realnvp", 64, (64, 64), 4, 0, 0.0, "banana_b03", 1029, 5),
    "nsf_d2_k10_nl2_banana": ("nsf", 2, (32, 32), 2, 10, 5.0, "banana", 333, 3),
    "nsf_d32_k8_nl3_funnel": ("nsf", 32, (32, 32), 3, 8, 5.0, "funnel", 519, 3),
    "nsf_d2_k8_nl2_cross": ("nsf", 2, (32, 32), 2, 8, 5.0, "cross", 515, 3),
    "nsf_d2_k8_nl2_warped": ("nsf", 2, (32, 32), 2, 8, 5.0, "warped", 515, 3),
}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_step_gradient_loss_and_forward_against_the_oracle(nf, case):
    """nf_elbo_value_and_grad (the step's forward and reverse pass) and nf_elbo_batch_rng against
    oracle.neg_elbo_value_and_grad on the regenerated draws (seed 77, offset 0, stream 0), at parity.py's own tolerances.
    The float32 oracle's error on the same inputs is asserted to be at most a tenth of the plain gradient tolerance, so the
    floor clause does not carry the case."""
    kind, d, hd, nl, K, B, tname, n, iseed = ORACLE_CASES[case]
    spec = o.FlowSpec(kind, d, nl, hd, K, B)
    th64 = o.init_params(spec, np.random.default_rng(iseed)).astype(np.float32).astype(np.float64)
    flow = nf.Flow(kind, nf.MvNormal(d), nl, hd, K, B, dtype=torch.float32, device="cuda", theta=torch.tensor(th64, dtype=torch.float32, device="cuda"))
    tgt, otgt = make_target(nf, tname, d)
    xs = o.base_sample(d, n, 77, 0, 0)
    l_ref, g_ref = o.neg_elbo_value_and_grad(spec, th64, otgt, xs)
    l32, g32 = o.neg_elbo_value_and_grad(spec, P.f32(th64), P.f32(otgt), P.f32(xs))
    scale = np.abs(g_ref).max()
    floor = float(np.abs(np.asarray(g32, dtype=np.float64) - g_ref).max() / scale)
    P.record(f"elbo targets {case}: float32 oracle alone [max abs err / |g|inf]", floor)
    assert floor <= 0.1 * P.GRAD_RTOL, f"{case}: the float32 oracle alone is at {floor:.2e} of |g|inf: pick other parameters"
    assert abs(float(l32) - l_ref) <= 0.1 * P.LOSS_RTOL * abs(l_ref)
    lib, ctx = nf.load_library(), new_ctx(nf)
    out = torch.empty(flow.P + 1, device="cuda")
    nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta), None, n, n, 77, 0, 0, vp(out)))
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    print(f"{case}: loss {got[-1]!r} oracle {l_ref!r}; grad err / |g|inf {np.abs(got[:-1] - g_ref).max() / scale:.3e} (float32 oracle {floor:.3e})")
    P.gradient(f"elbo targets {case}: grad", got[:-1], g_ref, floor=g32)
    P.scalar(f"elbo targets {case}: loss", got[-1], l_ref)
    elbo = C.c_double(0)
    nf._lib.check(lib.nf_elbo_batch_rng(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta), n, 77, 0, 0, C.byref(elbo)))
    print(f"{case}: nf_elbo_batch_rng {elbo.value!r} oracle {-l_ref!r}")
    P.scalar(f"elbo targets {case}: nf_elbo_batch_rng", elbo.value, -l_ref)
    ctx.close()


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
def test_train_flow_on_the_banana_demo_equals_the_split_loop(nf):
    """train_flow(elbo_batch, realnvp(q0, [16, 16], 3), Banana(2, 1, 100), 16) -- example/demo_RealNVP.jl as written -- returns
    the theta, Adam state and stat tuples of `optimize` over value_and_gradient + update, also when continued from `st`."""
    from normalizingflows_jl_amd import objectives as ob

    flow = nf.realnvp(nf.MvNormal(2), (16, 16), 3, paramtype=torch.float32, seed=5)
    tgt, n = nf.BananaTarget(2, 1.0, 100.0), 16
    seen = []

    def cb(i, stats, re, theta):
        seen.append(theta.clone())
        return {"extra": i}

    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(9), None, {})
    fa, sa, sta = nf.train_flow(nf.PhiloxRNG(9), nf.elbo_batch, flow, tgt, n, max_iters=20, optimiser=nf.Adam(2e-3), callback=cb)
    seen_a, seen = seen, []
    theta0, re = flow.destructure()
    rng_b = nf.PhiloxRNG(9)
    tb, sb, stb = nf.optimize(lambda th: nf.value_and_gradient(nf.elbo_batch, re(th), tgt, n, rng_b), theta0, re, max_iters=20,
                              optimiser=nf.Adam(2e-3), callback=cb)
    assert torch.equal(fa.theta, tb) and torch.equal(sta.m, stb.m) and torch.equal(sta.v, stb.v) and sta.t == stb.t == 20
    assert len(sa) == len(sb) == 20
    for a, b in zip(sa, sb):
        assert a["iteration"] == b["iteration"] and a["extra"] == b["extra"]
        assert a["loss"] == pytest.approx(b["loss"], rel=1e-6) and a["gradient_norm"] == pytest.approx(b["gradient_norm"], rel=1e-6)
    assert all(torch.equal(x, y) for x, y in zip(seen_a, seen)) and torch.equal(seen_a[0], theta0)
    rng_c = nf.PhiloxRNG(9)
    f8, _, st8 = nf.train_flow(rng_c, nf.elbo_batch, flow, tgt, n, max_iters=8, optimiser=nf.Adam(2e-3))
    f20, _, st20 = nf.train_flow(rng_c, nf.elbo_batch, f8, tgt, n, max_iters=12, optimiser=nf.Adam(2e-3), state=st8)
    assert st20.t == 20 and torch.equal(f20.theta, tb)


# ---- 7. refusals stay loud ---------------------------------------------------------------------------------------------------
def _refused(nf, name):
    """(flow, target, n, code nf_elbo_step_enqueue returns, code nf_elbo_step returns)"""
    if name == "warped_d4":
        return make_flow(nf, "realnvp", 4, (32, 32), 2), nf.WarpedGaussTarget(1.0, 0.12), 300, NF_ERR_UNSUPPORTED, NF_ERR_ARG
    if name == "cross_d6_nsf":
        return make_flow(nf, "nsf", 6, (32, 32), 2, 8), nf.CrossTarget(2.0, 0.15), 300, NF_ERR_UNSUPPORTED, NF_ERR_ARG
    if name == "realnvp_f64":
        return nf.realnvp(nf.MvNormal(5), (32, 32), 2, paramtype=torch.float64, seed=2), nf.BananaTarget(5, 1.0, 100.0), 97, NF_ERR_UNSUPPORTED, 0
    if name == "deep_3hidden":
        return nf.realnvp(nf.MvNormal(9), (32, 32, 32), 2, paramtype=torch.float32, seed=2), nf.FunnelTarget(9, 0.3, 2.0), 300, NF_ERR_UNSUPPORTED, 0
    return nf.realnvp(nf.MvNormal(96), (128, 100), 1, paramtype=torch.float32, seed=2), nf.BananaTarget(96, 1.0, 100.0), 300, NF_ERR_UNSUPPORTED, 0


@pytest.mark.parametrize("name", ["warped_d4", "cross_d6_nsf", "realnvp_f64", "deep_3hidden", "wide_streaming"])
def test_flows_and_targets_without_the_fused_form_are_refused_by_the_graph_form(nf, name):
    """WarpedGauss / Cross with d != 2, a Float64 flow, a three-hidden-layer and a weight-streaming flow: nf_elbo_step_enqueue
    answers NF_ERR_UNSUPPORTED as before; nf_elbo_step on the valid ones equals the split calls bit for bit, and on a
    two-dimensional target at another d both nf_elbo_step and nf_elbo_value_and_grad still answer NF_ERR_ARG."""
    lib = nf.load_library()
    flow, tgt, n, code_enqueue, code_step = _refused(nf, name)
    dt = flow.theta.dtype
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 77, vp(counter), LR, B1, B2, EPS, None)
    assert st == code_enqueue
    torch.cuda.synchronize()
    assert torch.equal(th, flow.theta) and int(counter[0]) == 0
    if code_step:
        st = lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 77, 0, LR, B1, B2, EPS, None, None)
        assert st == code_step
        out = torch.empty(flow.P + 1, dtype=dt, device="cuda")
        st = lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), None, n, n, 77, 0, 0, vp(out))
        assert st == code_step
        elbo = C.c_double(0)
        assert lib.nf_elbo_batch_rng(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), n, 77, 0, 0, C.byref(elbo)) == code_step
    else:
        out, gn = torch.empty(flow.P + 1, dtype=dt, device="cuda"), torch.empty(1, dtype=dt, device="cuda")
        th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        for step in range(2):
            loss, gnorm = C.c_double(0), C.c_double(0)
            nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 77, step, LR, B1, B2, EPS,
                                           C.byref(loss), C.byref(gnorm)))
            nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, 77, 0, step, vp(out)))
            nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0 if dt == torch.float32 else 1, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2,
                                             EPS, step + 1, vp(gn)))
            assert loss.value == float(out[flow.P]) and gnorm.value == float(gn)
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    ctx_a.close()
    ctx_b.close()


def test_spline_graph_form_is_refused_under_a_communicator(nf):
    """The spline step is a one-rank step: on a context that holds a communicator nf_elbo_step_enqueue answers
    NF_ERR_UNSUPPORTED for a spline flow, and nf_elbo_step runs the generic sequence with the split calls' bits."""
    lib = nf.load_library()
    flow = make_flow(nf, "nsf", 9, (24, 32), 2, 10)
    tgt, n = nf.FunnelTarget(9, 0.3, 2.0), 333
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    arr = (C.c_void_p * 1)(ctx_a.ptr)
    st = lib.nf_comm_init_all(arr, 1)
    if st == NF_ERR_NO_RCCL:
        ctx_a.close()
        ctx_b.close()
        pytest.skip("librccl.so.1 is not available")
    nf._lib.check(st)
    try:
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 77, vp(counter), LR, B1, B2, EPS, None)
        assert st == NF_ERR_UNSUPPORTED
        th_b, m_b, v_b, stats_b = split_steps(nf, flow, tgt, n, 77, 2, ctx_b)
        for step in range(2):
            one_call_step(nf, ctx_a, flow, tgt, th, m, v, n, 77, step)
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    finally:
        nf._lib.check(lib.nf_comm_destroy(ctx_a.ptr))
        ctx_a.close()
        ctx_b.close()
