"""GPU tests of the fused ELBO step of planar, radial and mean-field flows (nf_elbo_step / nf_elbo_step_enqueue: the step
launch, k_simple_epilogue, k_finish_sum).  The reference for every number is the split sequence nf_elbo_value_and_grad +
nf_adam_update on another context: theta, m and v must match it bit for bit; loss and norm(g) to rounding -- Float32 rel 1e-6
(the suite's convention for fused steps), Float64 rel 1e-12 (at most nf_simple_elbo_max_partials = 16 x 256 CUs = 4096 partials
per launch, times 2^-52; the norm's terms are non-negative, and every case's split loss is asserted to be above 0.1 in
magnitude so that cancellation does not enter)."""
import ctypes as C

import pytest

from __graft_entry__ import load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
NF_ERR_ARG, NF_ERR_UNSUPPORTED, NF_ERR_NO_RCCL, NF_ERR_WORKSPACE = -1, -2, -5, -7
SEED = 77
PROF_NAMES = ("adam", "simple_finalize", "simple_epilogue", "simple_step", "planar_step", "radial_step")
F32, F64 = "f32", "f64"

CASES = {
    # name: (kind, d, nlayers, dtype, N, target)                      kernel reached
    "planar_d2x10_f64_banana": ("planar", 2, 10, F64, 37, "banana"),      # k_simple_step<double>, 3 blocks, ragged
    "planar_d2x12_f64_funnel": ("planar", 2, 12, F64, 16, "funnel"),      # the layer cap of step_nlmax, one block
    "radial_d5x10_f64_diag": ("radial", 5, 10, F64, 257, "diaggauss"),    # k_simple_step<double> radial
    "meanfield_d4_f64_diag": ("meanfield", 4, 1, F64, 33, "diaggauss"),   # shift / scale branches
    "planar_d6x5_f32_diag": ("planar", 6, 5, F32, 1000, "diaggauss"),     # k_planar_step
    "planar_d64x10_f32_banana": ("planar", 64, 10, F32, 1000, "banana"),  # k_planar_step, full width
    "planar_d100x4_f32_diag": ("planar", 100, 4, F32, 100, "diaggauss"),  # k_simple_step<float>, 8 dims per lane
    "radial_d16x4_f32_funnel": ("radial", 16, 4, F32, 257, "funnel"),     # k_radial_step
    "radial_d5x10_f32_banana": ("radial", 5, 10, F32, 257, "banana"),     # k_simple_step<float> radial
}
GRAPH_CASES = ["planar_d2x10_f64_banana", "planar_d64x10_f32_banana", "radial_d16x4_f32_funnel", "meanfield_d4_f64_diag"]


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def vp(t):
    return C.c_void_p(t.data_ptr())


def new_ctx(nf):
    return nf.Context(0, torch.cuda.current_stream().cuda_stream)


def tdt(code):
    return torch.float32 if code == F32 else torch.float64


def rtol(dt):
    return 1e-6 if dt == torch.float32 else 1e-12


def make_flow(nf, kind, d, nl, dt, seed=3):
    q0 = nf.MvNormal(d)
    if kind == "meanfield":
        return nf.meanfield(q0, paramtype=dt)
    f = (nf.planarflow if kind == "planar" else nf.radialflow)(q0, nl, paramtype=dt, seed=seed)
    return f.with_theta(f.theta * 0.3)  # as the existing planar cases: losses stay finite


def make_target(nf, name, d, dt):
    if name == "banana":
        return nf.BananaTarget(d, 1.0, 10.0)
    if name == "funnel":
        return nf.FunnelTarget(d, 0.3, 2.0)
    gen = torch.Generator().manual_seed(d)
    mu = torch.randn(d, generator=gen, dtype=torch.float64)
    var = torch.rand(d, generator=gen, dtype=torch.float64) + 0.5
    return nf.DiagGaussTarget(mu.to(dt).cuda(), var.to(dt).cuda())


def make_case(nf, name):
    kind, d, nl, dc, n, tname = CASES[name]
    dt = tdt(dc)
    return make_flow(nf, kind, d, nl, dt), make_target(nf, tname, d, dt), n


def dcode(flow):
    return 0 if flow.theta.dtype == torch.float32 else 1


def split_steps(nf, flow, tgt, n, nsteps, ctx, seed=SEED, snap_at=None, snaps=None):
    """nsteps of nf_elbo_value_and_grad + nf_adam_update on `ctx` (from flow.theta, zero moments); a copy of (theta, m, v)
    after `snap_at` steps is appended to `snaps`"""
    lib = nf.load_library()
    dt = flow.theta.dtype
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, dtype=dt, device="cuda"), torch.empty(1, dtype=dt, device="cuda")
    stats = []
    for step in range(nsteps):
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, dcode(flow), vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        stats.append((float(out[flow.P]), float(gn)))
        if snap_at == step + 1:
            snaps.append((th.clone(), m.clone(), v.clone()))
    return th, m, v, stats


_SPLIT = {}


def split_reference(nf, name):
    """six split steps of a case, computed once and shared (read-only) by the tests that need them:
    ((theta, m, v) after five steps, (theta, m, v) after six, [(loss, norm)] of the six)"""
    if name not in _SPLIT:
        flow, tgt, n = make_case(nf, name)
        ctx = new_ctx(nf)
        snaps = []
        th, m, v, stats = split_steps(nf, flow, tgt, n, 6, ctx, snap_at=5, snaps=snaps)
        torch.cuda.synchronize()
        ctx.close()
        _SPLIT[name] = (snaps[0], (th, m, v), stats)
    return _SPLIT[name]


def one_call_step(nf, ctx, flow, tgt, th, m, v, n, step, want=True, seed=SEED):
    lib = nf.load_library()
    loss, gn = C.c_double(0), C.c_double(0)
    nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS,
                                   C.byref(loss) if want else None, C.byref(gn) if want else None))
    return loss.value, gn.value


def enqueue_code(nf, ctx, flow, tgt, th, m, v, n, counter, stat=None, seed=SEED):
    lib = nf.load_library()
    return lib.nf_elbo_step_enqueue(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS,
                                    vp(stat) if stat is not None else None)


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


def fresh(flow):
    return flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)


# ---- 1. fused equals split -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_step_equals_split_calls_over_consecutive_steps(nf, name):
    """Five consecutive nf_elbo_step calls against the split calls on another context: theta, m, v bit for bit, loss and
    norm(g) to rounding (steps 1-3 without a host readback)."""
    flow, tgt, n = make_case(nf, name)
    (th_b, m_b, v_b), _, stats_b = split_reference(nf, name)
    tol = rtol(flow.theta.dtype)
    ctx = new_ctx(nf)
    th, m, v = fresh(flow)
    for step in range(5):
        want = step in (0, 4)
        loss, gn = one_call_step(nf, ctx, flow, tgt, th, m, v, n, step, want)
        if want:
            print(f"{name} step {step}: loss {loss!r} split {stats_b[step][0]!r}; norm {gn!r} split {stats_b[step][1]!r}")
            assert abs(stats_b[step][0]) > 0.1, "pick another seed: the split loss is too close to zero for a relative bound"
            assert loss == pytest.approx(stats_b[step][0], rel=tol)
            assert gn == pytest.approx(stats_b[step][1], rel=tol)
    torch.cuda.synchronize()
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    assert bool(torch.isfinite(th).all())
    ctx.close()


# ---- 2. graph replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPH_CASES)
def test_step_with_device_counter_replays_as_a_graph(nf, name):
    """nf_elbo_step_enqueue: one eager warm-up call, one captured call, five replays -- the counter reads 6, theta, m and v are
    those of six split steps bit for bit, out_loss_gnorm_device (the flow's element type) holds step 5's loss and norm."""
    flow, tgt, n = make_case(nf, name)
    dt = flow.theta.dtype
    _, (th_b, m_b, v_b), stats_b = split_reference(nf, name)
    th, m, v = fresh(flow)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    stat = torch.zeros(2, dtype=dt, device="cuda")
    side = torch.cuda.Stream()
    ctx = nf.Context(0, side.cuda_stream)

    def enqueue():
        st = enqueue_code(nf, ctx, flow, tgt, th, m, v, n, counter, stat)
        assert st == 0, st

    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()  # step 0, eager: sizes the workspace, sets kernel attributes
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
    print(f"{name}: [loss ; norm] {stat.tolist()!r} split {stats_b[5]!r}")
    assert abs(stats_b[5][0]) > 0.1
    assert float(stat[0]) == pytest.approx(stats_b[5][0], rel=rtol(dt)) and float(stat[1]) == pytest.approx(stats_b[5][1], rel=rtol(dt))
    del graph
    ctx.close()


# ---- 3. launch counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar_d2x10_f64_banana", "planar_d64x10_f32_banana", "radial_d16x4_f32_funnel", "meanfield_d4_f64_diag"])
def test_fused_step_launches(nf, name):
    """A fused step: no Adam launch, no k_simple_finalize launch, one k_simple_epilogue and one step launch.  The split calls on
    the same context run k_simple_finalize and Adam as launches of their own."""
    lib = nf.load_library()
    flow, tgt, n = make_case(nf, name)
    ctx = new_ctx(nf)
    th, m, v = fresh(flow)
    one_call_step(nf, ctx, flow, tgt, th, m, v, n, 0)  # warm-up (workspace, attributes)
    got = launches(nf, ctx, lambda: one_call_step(nf, ctx, flow, tgt, th, m, v, n, 1, want=False))
    assert got["adam"] == 0 and got["simple_finalize"] == 0 and got["simple_epilogue"] == 1, got
    assert got["simple_step"] + got["planar_step"] + got["radial_step"] == 1, got
    out = torch.empty(flow.P + 1, dtype=flow.theta.dtype, device="cuda")
    gn = torch.empty(1, dtype=flow.theta.dtype, device="cuda")

    def split():
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), None, n, n, SEED, 0, 2, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, dcode(flow), vp(th), vp(out), vp(m), vp(v), flow.P, LR, B1, B2, EPS, 3, vp(gn)))

    got = launches(nf, ctx, split)
    assert got["adam"] == 1 and got["simple_finalize"] == 1 and got["simple_epilogue"] == 0, got
    ctx.close()


# ---- 4. caller arena -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar_d2x10_f64_banana", "planar_d64x10_f32_banana", "radial_d5x10_f32_banana", "meanfield_d4_f64_diag"])
def test_caller_arena_runs_step_and_enqueue(nf, name):
    """An arena of nf_workspace_bytes(desc, N) runs a step and an enqueue at N = 1, 17 and 1000 without NF_ERR_WORKSPACE and
    with the owned arena's bits."""
    lib = nf.load_library()
    flow, tgt, _ = make_case(nf, name)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(ctx, n):
        th, m, v = fresh(flow)
        nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, SEED, 0, LR, B1, B2, EPS, None, None))
        counter.fill_(1)
        st = enqueue_code(nf, ctx, flow, tgt, th, m, v, n, counter)
        assert st == 0, st
        torch.cuda.synchronize()
        assert int(counter[0]) == 2
        return th, m, v

    for n in (1, 17, 1000):
        ctx_ref = new_ctx(nf)
        ref = run(ctx_ref, n)
        ctx = new_ctx(nf)
        need = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), n))
        arena = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
        try:
            nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, C.c_void_p((arena.data_ptr() + 255) // 256 * 256), need))
            got = run(ctx, n)
            assert all(torch.equal(a, b) for a, b in zip(ref, got)), n
        finally:
            nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, None, 0))
        ctx.close()
        ctx_ref.close()


# ---- 5. refusals stay loud -----------------------------------------------------------------------------------------------------
def _refused(nf, name):
    """(flow, target, n, code nf_elbo_step_enqueue returns, code nf_elbo_step returns)"""
    if name == "planar_d200x30_f32":  # beyond nf_simple_step_supported
        f = nf.planarflow(nf.MvNormal(200), 30, paramtype=torch.float32, seed=2)
        return f.with_theta(f.theta * 0.05), make_target(nf, "diaggauss", 200, torch.float32), 300, NF_ERR_UNSUPPORTED, 0
    if name == "hamiltonian":
        tgt = make_target(nf, "diaggauss", 3, torch.float64)
        return nf.hamiltonianflow(3, 2, 3, tgt, paramtype=torch.float64), tgt, 64, NF_ERR_UNSUPPORTED, 0
    if name == "planar_general_base":
        mu = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64, device="cuda")
        var = torch.tensor([0.8, 1.3, 1.1], dtype=torch.float64, device="cuda")
        f = nf.planarflow(nf.MvNormal(mu, var), 4, paramtype=torch.float64, seed=2)
        return f.with_theta(f.theta * 0.3), nf.BananaTarget(3, 1.0, 10.0), 97, NF_ERR_UNSUPPORTED, 0
    if name == "warped_radial_d8":  # the same at a shape k_radial_step serves
        f = nf.radialflow(nf.MvNormal(8), 4, paramtype=torch.float32, seed=2)
        return f.with_theta(f.theta * 0.3), nf.WarpedGaussTarget(1.0, 0.12), 300, NF_ERR_UNSUPPORTED, NF_ERR_ARG
    f = nf.planarflow(nf.MvNormal(3), 4, paramtype=torch.float32, seed=2)  # WarpedGauss is two-dimensional
    return f.with_theta(f.theta * 0.3), nf.WarpedGaussTarget(1.0, 0.12), 300, NF_ERR_UNSUPPORTED, NF_ERR_ARG


@pytest.mark.parametrize("name", ["planar_d200x30_f32", "hamiltonian", "planar_general_base", "warped_planar_d3", "warped_radial_d8"])
def test_flows_and_targets_without_the_fused_form_are_refused_by_the_graph_form(nf, name):
    """A planar flow beyond the one-launch step, a Hamiltonian flow, a planar flow over a general base: nf_elbo_step_enqueue
    answers NF_ERR_UNSUPPORTED with theta untouched and the counter at 0, and nf_elbo_step equals the split calls, loss and norm
    included, bit for bit.  WarpedGauss at d = 3 (planar) and d = 8 (radial): NF_ERR_UNSUPPORTED from the graph form, NF_ERR_ARG from
    nf_elbo_step, theta untouched."""
    lib = nf.load_library()
    flow, tgt, n, code_enqueue, code_step = _refused(nf, name)
    dt = flow.theta.dtype
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = fresh(flow)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert enqueue_code(nf, ctx_a, flow, tgt, th, m, v, n, counter) == code_enqueue
    torch.cuda.synchronize()
    assert torch.equal(th, flow.theta) and int(counter[0]) == 0
    if code_step:
        st = lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, SEED, 0, LR, B1, B2, EPS, None, None)
        assert st == code_step
        assert torch.equal(th, flow.theta)
    else:
        out, gn = torch.empty(flow.P + 1, dtype=dt, device="cuda"), torch.empty(1, dtype=dt, device="cuda")
        th_b, m_b, v_b = fresh(flow)
        for step in range(2):
            loss, gnorm = one_call_step(nf, ctx_a, flow, tgt, th, m, v, n, step)
            nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, SEED, 0, step, vp(out)))
            nf._lib.check(lib.nf_adam_update(ctx_b.ptr, dcode(flow), vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
            assert loss == float(out[flow.P]) and gnorm == float(gn)
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    ctx_a.close()
    ctx_b.close()


def test_graph_form_is_refused_under_a_communicator(nf):
    """The fused step is a one-rank step: on a context that holds a communicator nf_elbo_step_enqueue answers
    NF_ERR_UNSUPPORTED for a planar flow, and nf_elbo_step runs the split sequence (its launches, its bits)."""
    lib = nf.load_library()
    name = "planar_d6x5_f32_diag"
    flow, tgt, n = make_case(nf, name)
    ctx_a = new_ctx(nf)
    arr = (C.c_void_p * 1)(ctx_a.ptr)
    st = lib.nf_comm_init_all(arr, 1)
    if st == NF_ERR_NO_RCCL:
        ctx_a.close()
        pytest.skip("librccl.so.1 is not available")
    nf._lib.check(st)
    try:
        th, m, v = fresh(flow)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert enqueue_code(nf, ctx_a, flow, tgt, th, m, v, n, counter) == NF_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.equal(th, flow.theta) and int(counter[0]) == 0
        one_call_step(nf, ctx_a, flow, tgt, th, m, v, n, 0)
        got = launches(nf, ctx_a, lambda: one_call_step(nf, ctx_a, flow, tgt, th, m, v, n, 1, want=False))
        assert got["adam"] == 1 and got["simple_finalize"] == 1 and got["simple_epilogue"] == 0, got
        ctx_b = new_ctx(nf)
        th_b, m_b, v_b, _ = split_steps(nf, flow, tgt, n, 2, ctx_b)
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
        ctx_b.close()
    finally:
        nf._lib.check(lib.nf_comm_destroy(ctx_a.ptr))
        ctx_a.close()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_train_flow_on_the_radial_demo_equals_the_split_loop(nf):
    """train_flow(elbo_batch, radialflow(q0, 10) (Float64), Banana(2, 1, 10), 32) -- the shape of example/demo_radial_flow.jl --
    returns the theta and Adam state of `optimize` over value_and_gradient + update bit for bit, and its stats to rounding."""
    from normalizingflows_jl_amd import objectives as ob

    flow = nf.radialflow(nf.MvNormal(2), 10, paramtype=torch.float64, seed=5)
    flow = flow.with_theta(flow.theta * 0.3)
    tgt, n = nf.BananaTarget(2, 1.0, 10.0), 32
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(9), None, {})
    fa, sa, sta = nf.train_flow(nf.PhiloxRNG(9), nf.elbo_batch, flow, tgt, n, max_iters=6, optimiser=nf.Adam(2e-3))
    theta0, re = flow.destructure()
    rng_b = nf.PhiloxRNG(9)
    tb, sb, stb = nf.optimize(lambda th: nf.value_and_gradient(nf.elbo_batch, re(th), tgt, n, rng_b), theta0, re, max_iters=6,
                              optimiser=nf.Adam(2e-3))
    assert torch.equal(fa.theta, tb) and torch.equal(sta.m, stb.m) and torch.equal(sta.v, stb.v) and sta.t == stb.t == 6
    assert len(sa) == len(sb) == 6
    for a, b in zip(sa, sb):
        print(f"iteration {a['iteration']}: loss {a['loss']!r} split {b['loss']!r}; norm {a['gradient_norm']!r} split {b['gradient_norm']!r}")
        assert a["iteration"] == b["iteration"] and abs(b["loss"]) > 0.1
        assert a["loss"] == pytest.approx(b["loss"], rel=1e-12) and a["gradient_norm"] == pytest.approx(b["gradient_norm"], rel=1e-12)
