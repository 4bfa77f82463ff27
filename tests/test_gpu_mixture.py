"""GPU tests of the Gaussian-mixture target (NF_TARGET_GAUSSMIX, MixtureTarget): nf_target_logp (flat kernel, both element
types), RealNVP / NSF flows (the tiled MFMA kernel, and the flat one on the Float64 path), nf_elbo_step, determinism, the
refusals, the closure route of the flows that evaluate their target in their own kernels, and train_flow.

Reference values are the numpy closed form of tests/test_mixture_cpu.py (dtype-generic, written on the packed parameters
the device reads); whole-flow references compose it with oracle.nf_oracle (flow_fwd(keep) -> logp / score -> flow_bwd) as
neg_elbo_value_and_grad does.  Tolerances are tests/parity.py's; every Float32 check passes `floor=`: the same formula
evaluated in numpy float32.

Inputs: Sigma_k = Q diag(lambda) Q' with lambda in [0.5, 2], means 3 randn(d) / sqrt(d), weights uniform in [0.5, 1.5] and
normalised; samples of the nf_target_logp tests are drawn around the components' own means in turn, so every component is
the largest term for some sample and the running maximum of the single-pass log-sum-exp changes at every loop position."""
import ctypes as C

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from __graft_entry__ import load_package
from test_mixture_cpu import cast_pack, cross_params, mixture_logp_score, random_mixture, target_pack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NF_ERR_ARG, NF_ERR_UNSUPPORTED = -1, -2
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
NAMES = ("target_mixture", "target_linpred", "target")
ONE_MIXTURE_LAUNCH = {"target_mixture": 1, "target_linpred": 0, "target": 0}


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def vp(t):
    return C.c_void_p(t.data_ptr())


def new_ctx(nf):
    return nf.Context(0, torch.cuda.current_stream().cuda_stream)


def tdt(f64):
    return torch.float64 if f64 else torch.float32


def tag(f64):
    return "f64" if f64 else "f32"


def to_dev(a, f64):
    """(d, N) numpy -> the package's column-major batch on the device"""
    return torch.tensor(np.ascontiguousarray(a.T), dtype=tdt(f64), device="cuda").t()


def build_target(nf, pi, mus, Sig, f64):
    dt = tdt(f64)
    tgt = nf.MixtureTarget(torch.tensor(pi, dtype=dt, device="cuda"), torch.tensor(mus, dtype=dt, device="cuda"),
                           torch.tensor(Sig, dtype=dt, device="cuda"))
    pack = target_pack(tgt)  # float64 copies of the values the device reads
    pack32 = cast_pack(pack, np.float32)

    def ref(y):
        return mixture_logp_score(y, *(pack32 if y.dtype == np.float32 else pack))

    return tgt, ref, pack


_MADE = {}


def make_mixture(nf, d, K, f64):
    key = (d, K, f64)
    if key not in _MADE:
        pi, mus, Sig = random_mixture(d, K)
        _MADE[key] = build_target(nf, pi, mus, Sig, f64) + ((pi, mus, Sig),)
    return _MADE[key]


def samples_around_the_means(mus, Sig, n, f64, seed=1):
    """sample j is drawn from component j mod K"""
    K, d = mus.shape
    rng = np.random.default_rng(seed + 10 * d + K + n)
    L = np.linalg.cholesky(Sig)
    ys = np.stack([mus[j % K] + L[j % K] @ rng.standard_normal(d) for j in range(n)], axis=1)
    return ys if f64 else ys.astype(np.float32).astype(np.float64)


def device_logp(nf, tgt, ys64, f64):
    lp, sc = nf.target_logp(tgt, to_dev(ys64, f64), with_grad=True)
    lp_only = nf.target_logp(tgt, to_dev(ys64, f64))
    torch.cuda.synchronize()
    lp, sc = lp.double().cpu().numpy(), sc.double().cpu().numpy()
    assert np.array_equal(lp, lp_only.double().cpu().numpy())  # the value does not depend on whether the score is asked for
    return lp, sc


def check_against(key, lp, sc, lr, sr, f64, l32=None, s32=None):
    assert np.isfinite(lp).all() and np.isfinite(sc).all(), key
    print(f"{key}: logp err {np.abs(lp - lr).max():.3e} of max |logp| {np.abs(lr).max():.3e}; score err {np.abs(sc - sr).max():.3e} "
          f"of max |score| {np.abs(sr).max():.3e}")
    if f64:
        P.elementwise(key + ": logp", lp, lr, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": score", sc, sr, P.F64_RTOL, 1e-12)
    else:
        P.elementwise(key + ": logp", lp, lr, floor=l32)
        P.elementwise(key + ": score", sc, sr, floor=s32)


def check_logp(nf, key, tgt, ref, ys64, f64):
    lp, sc = device_logp(nf, tgt, ys64, f64)
    lr, sr = ref(ys64)
    l32, s32 = (None, None) if f64 else ref(ys64.astype(np.float32))
    check_against(key, lp, sc, lr, sr, f64, l32, s32)
    return lp, sc


# ---- 1. nf_target_logp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("d,K", [(2, 4), (5, 1), (5, 3), (5, 9), (33, 5), (64, 9)])
def test_target_logp(nf, d, K, f64):
    """value and score at N = 1 and 37 (three blocks, the last ragged); K = 1 also against MvNormalTarget of the same (mu, Sigma)"""
    tgt, ref, _, (pi, mus, Sig) = make_mixture(nf, d, K, f64)
    for n in (1, 37):
        ys = samples_around_the_means(mus, Sig, n, f64)
        key = f"mixture logp d={d} K={K} N={n} {tag(f64)}"
        lp, sc = check_logp(nf, key, tgt, ref, ys, f64)
        if n == 37:  # every component is the largest term of some sample
            u = np.einsum("kij,jn->kin", target_pack(tgt)[3], ys - target_pack(tgt)[0][:, None]) - target_pack(tgt)[1][:, :, None]
            q = target_pack(tgt)[2][:, None] - 0.5 * (u * u).sum(1)
            assert set(q.argmax(0)) == set(range(K)), key
        if K == 1:
            dt = tdt(f64)
            mv = nf.MvNormalTarget(torch.tensor(mus[0], dtype=dt, device="cuda"), torch.tensor(Sig[0], dtype=dt, device="cuda"))
            lg, sg = device_logp(nf, mv, ys, f64)
            # two Float32 device results: the floor is the float32 closed form's own error, carried over to this reference
            fl = (None, None) if f64 else tuple(g + (a - b) for g, a, b in zip((lg, sg), ref(ys.astype(np.float32)), ref(ys)))
            check_against(key + " vs MvNormalTarget", lp, sc, lg, sg, f64, *fl)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_cross_parameters_against_the_cross_target(nf, f64):
    """MixtureTarget at Cross(2, 0.15)'s components (cross.jl's vectors are standard deviations) against CrossTarget evaluated
    on the device in Float64"""
    pi, mus, Sig = cross_params(2.0, 0.15)
    tgt, ref, _ = build_target(nf, pi, mus, Sig, f64)
    ys = samples_around_the_means(mus, Sig, 37, f64, seed=3)
    lc, sc_c = device_logp(nf, nf.CrossTarget(2.0, 0.15), ys, True)
    lp, sc = device_logp(nf, tgt, ys, f64)
    lr, sr = ref(ys)
    l32, s32 = (None, None) if f64 else ref(ys.astype(np.float32))
    check_against(f"mixture cross {tag(f64)}", lp, sc, lr, sr, f64, l32, s32)
    if f64:  # (a Float32 target holds rounded parameters: its closed form is not Cross(2, 0.15) to 1e-10)
        P.elementwise("mixture cross: closed form vs CrossTarget f64 logp", lr, lc, P.F64_RTOL, 1e-12)
    check_against(f"mixture cross {tag(f64)} vs CrossTarget", lp, sc, lc, sc_c, f64, l32, s32)


# ---- 2. stability --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_far_samples_stay_finite(nf, f64):
    """samples at least 40 standard deviations from every component: finite log p and score, at the usual tolerances"""
    d, K = 5, 3
    tgt, ref, pack, (pi, mus, Sig) = make_mixture(nf, d, K, f64)
    rng = np.random.default_rng(8)
    dirs = rng.standard_normal((d, 37))
    ys = mus.mean(0)[:, None] + 150.0 * dirs / np.linalg.norm(dirs, axis=0)
    ys = ys if f64 else ys.astype(np.float32).astype(np.float64)
    mbar, b, c, W = pack
    u = np.einsum("kij,jn->kin", W, ys - mbar[:, None]) - b[:, :, None]
    assert np.sqrt((u * u).sum(1)).min() >= 40.0
    check_logp(nf, f"mixture far samples {tag(f64)}", tgt, ref, ys, f64)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_an_underflowing_component_leaves_the_other_gaussian(nf, f64):
    """two components 30 apart, samples sitting on either: the far component's weight underflows (Float32: exp(-400) = 0), the
    result is the near component's dense Gaussian plus log pi_k"""
    d = 5
    pi, mus, Sig = random_mixture(d, 2, seed=5)
    mus[1] = mus[0] + 30.0 * np.eye(d)[0]
    tgt, ref, (mbar, b, c, W) = build_target(nf, pi, mus, Sig, f64)
    ys = samples_around_the_means(mus, Sig, 37, f64, seed=2)

    def near_gauss(y, pk):  # c_k already holds log pi_k
        m_, b_, c_, W_ = pk
        out_l, out_s = np.empty(y.shape[1], y.dtype), np.empty_like(y)
        for j in range(y.shape[1]):
            k = j % 2
            u = W_[k] @ (y[:, j] - m_) - b_[k]
            out_l[j], out_s[:, j] = c_[k] - y.dtype.type(0.5) * (u * u).sum(), -(W_[k].T @ u)
        return out_l, out_s

    lr, sr = near_gauss(ys, (mbar, b, c, W))
    lp, sc = device_logp(nf, tgt, ys, f64)
    l32, s32 = (None, None) if f64 else near_gauss(ys.astype(np.float32), cast_pack((mbar, b, c, W), np.float32))
    check_against(f"mixture underflowing component {tag(f64)}", lp, sc, lr, sr, f64, l32, s32)


# ---- 3. through a flow -----------------------------------------------------------------------------------------------------------
def composed_neg_elbo(spec, theta, ref, xs):
    """oracle.neg_elbo_value_and_grad with the target's closed form in place of oracle.target_logp / target_grad"""
    n = xs.shape[1]
    ys, ladj, states = o.flow_fwd(spec, theta, xs, keep=True)
    lp, sc = ref(ys)
    elbos = lp - o.std_normal_logpdf(xs) + ladj
    ybar = (-sc / n).astype(xs.dtype)
    lbar = np.full(n, -1.0 / n, dtype=xs.dtype)
    _, grad = o.flow_bwd(spec, theta, states, ybar, lbar)
    return -elbos.mean(), grad


def prof_counts(nf, ctx, run, names=NAMES):
    lib = nf.load_library()
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
    out = run()
    torch.cuda.synchronize()
    counts = {}
    for name in names:
        a, c = C.c_double(0.0), C.c_int64(0)
        lib.nf_prof_read(ctx.ptr, name.encode(), C.byref(a), C.byref(c))
        counts[name] = c.value
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
    return out, counts


FLOW_CASES = {
    # name: (kind, d, hdims, nblocks, K, B, f64, mixture components)
    "realnvp_d5_K1": ("realnvp", 5, (32, 32), 2, 0, 0.0, False, 1),    # three idle waves
    "realnvp_d5_K3": ("realnvp", 5, (32, 32), 2, 0, 0.0, False, 3),    # one idle wave
    "realnvp_d5_K4": ("realnvp", 5, (32, 32), 2, 0, 0.0, False, 4),    # exactly one round
    "realnvp_d5_K5": ("realnvp", 5, (32, 32), 2, 0, 0.0, False, 5),    # a ragged second round
    "realnvp_d5_K9": ("realnvp", 5, (32, 32), 2, 0, 0.0, False, 9),    # three rounds on wave 0
    "realnvp_d33_K5": ("realnvp", 33, (64, 64), 2, 0, 0.0, False, 5),  # a second row block of one row; components unaligned to 32
    "realnvp_d64_K9": ("realnvp", 64, (64, 64), 2, 0, 0.0, False, 9),
    "nsf_d6_K3": ("nsf", 6, (32, 32), 2, 8, 5.0, False, 3),
    "realnvp_d5_f64_K3": ("realnvp", 5, (32, 32), 2, 0, 0.0, True, 3),  # flat kernel, Float64 coupling path
}


def make_flow_case(nf, name):
    kind, d, hd, nl, K, B, f64, Kmix = FLOW_CASES[name]
    spec = o.FlowSpec(kind, d, nl, hd, K, B)
    th = o.init_params(spec, np.random.default_rng(3))
    if not f64:
        th = th.astype(np.float32).astype(np.float64)
    flow = nf.Flow(kind, nf.MvNormal(d), nl, hd, K, B, dtype=tdt(f64), device="cuda", theta=torch.tensor(th, dtype=tdt(f64), device="cuda"))
    tgt, ref, _, _ = make_mixture(nf, d, Kmix, f64)
    return spec, th, flow, tgt, ref, f64


def check_flow_case(nf, key, spec, th, flow, tgt, ref, f64, n, xs=None):
    if xs is None:
        xs = o.base_sample(spec.d, n, 77, 0, 0)
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, f64)))
    assert counts == ONE_MIXTURE_LAUNCH, counts
    print(f"{key}: loss {loss!r} oracle {l_ref!r}; grad err / |g|inf {np.abs(g.double().cpu().numpy() - g_ref).max() / np.abs(g_ref).max():.3e}")
    assert 0.5 < abs(l_ref) < 500.0
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": grad", g, g_ref, P.F64_GRAD)
    else:
        l32, g32 = composed_neg_elbo(spec, P.f32(th), ref, P.f32(xs))
        P.record(key + ": loss, float32 oracle [rel err]", abs(float(l32) - l_ref) / abs(l_ref))
        P.scalar(key + ": loss", loss, l_ref)
        P.gradient(key + ": grad", g, g_ref, floor=g32)
    return xs


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_value_and_gradient_through_a_coupling_flow(nf, name):
    """value_and_gradient(elbo_batch, flow, target, xs) on caller-supplied draws at N = 33 and 97 (ragged tiles) against the
    composed oracle; exactly one "target_mixture" launch and no "target" / "target_linpred" launch per call; batched_elbos per sample."""
    spec, th, flow, tgt, ref, f64 = make_flow_case(nf, name)
    for n in (33, 97):
        key = f"mixture flow {name} N={n}"
        xs = check_flow_case(nf, key, spec, th, flow, tgt, ref, f64, n)
        elbos = nf.batched_elbos(flow, tgt, to_dev(xs, f64))
        ys, ladj, _ = o.flow_fwd(spec, th, xs, keep=True)
        e_ref = ref(ys)[0] - o.std_normal_logpdf(xs) + ladj
        if f64:
            P.elementwise(key + ": elbos", elbos, e_ref, P.F64_RTOL, 1e-12)
        else:
            xs32, th32 = P.f32(xs), P.f32(th)
            y32, l32_, _ = o.flow_fwd(spec, th32, xs32, keep=True)
            P.elementwise(key + ": elbos", elbos, e_ref, floor=ref(y32)[0] - o.std_normal_logpdf(xs32) + l32_)


def waves_running_maximum_moves_everywhere(q, waves=4):
    """q (K, N): per-component terms.  True when, for every wave w and every position p >= 1 of its component list
    k = w, w + 4, ..., some sample has q[k_p] above all the wave's earlier terms (the running maximum M changes there, so S and G
    are rescaled by a factor other than 1), and some sample has it below (the other branch)."""
    K = q.shape[0]
    for w in range(min(waves, K)):
        ks = list(range(w, K, waves))
        for p in range(1, len(ks)):
            before = q[ks[:p]].max(0)
            if not ((q[ks[p]] > before).any() and (q[ks[p]] < before).any()):
                return False
    return True


@pytest.mark.parametrize("d,hd", [(5, (32, 32)), (64, (64, 64))], ids=["d5", "d64"])
def test_tiled_kernel_on_samples_around_every_component(nf, d, hd):
    """The tiled kernel with K = 9 (three rounds on wave 0) on draws steered to the components: a RealNVP flow at theta = 0 is the
    identity, so the caller-supplied draws ARE the target's arguments; they are drawn around the components' own means in turn.
    Checked on the oracle's flow output: in every wave the running maximum moves at every loop position for some sample and
    stays for another, and every component is the largest term somewhere."""
    K, n = 9, 97
    spec = o.FlowSpec("realnvp", d, 2, hd, 0, 0.0)
    th = np.zeros_like(o.init_params(spec, np.random.default_rng(3)))
    flow = nf.Flow("realnvp", nf.MvNormal(d), 2, hd, 0, 0.0, dtype=torch.float32, device="cuda", theta=torch.tensor(th, dtype=torch.float32, device="cuda"))
    tgt, ref, (mbar, b, c, W), (pi, mus, Sig) = make_mixture(nf, d, K, False)
    xs = samples_around_the_means(mus, Sig, n, False, seed=4)
    ys, _, _ = o.flow_fwd(spec, th, xs, keep=True)
    assert np.array_equal(ys, xs)
    u = np.einsum("kij,jn->kin", W, ys - mbar[:, None]) - b[:, :, None]
    q = c[:, None] - 0.5 * (u * u).sum(1)
    assert set(q.argmax(0)) == set(range(K)) and waves_running_maximum_moves_everywhere(q)
    key = f"mixture tiled steered d={d} K={K} N={n}"
    check_flow_case(nf, key, spec, th, flow, tgt, ref, False, n, xs=xs)
    elbos = nf.batched_elbos(flow, tgt, to_dev(xs, False))
    e_ref = ref(ys)[0] - o.std_normal_logpdf(xs)
    x32 = P.f32(xs)
    P.elementwise(key + ": elbos", elbos, e_ref, floor=ref(x32)[0] - o.std_normal_logpdf(x32))


# ---- 4. the step -----------------------------------------------------------------------------------------------------------------
def test_elbo_step_equals_the_split_calls_and_the_graph_form_refuses(nf):
    """two consecutive nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit;
    nf_elbo_step_enqueue answers NF_ERR_UNSUPPORTED and leaves theta and the counter alone."""
    lib = nf.load_library()
    flow = nf.realnvp(nf.MvNormal(5), (32, 32), 2, paramtype=torch.float32, seed=2)
    tgt = make_mixture(nf, 5, 3, False)[0]
    n, seed = 97, 77
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert code == NF_ERR_UNSUPPORTED and torch.equal(th, flow.theta) and int(counter[0]) == 0
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    for step in range(2):
        loss, gnorm = C.c_double(0), C.c_double(0)
        _, counts = prof_counts(nf, ctx_a, lambda: nf._lib.check(lib.nf_elbo_step(
            ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS, C.byref(loss), C.byref(gnorm))))
        assert counts == ONE_MIXTURE_LAUNCH, counts
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert loss.value == float(out[flow.P]) and gnorm.value == float(gn), (step, loss.value, float(out[flow.P]), gnorm.value, float(gn))
        assert np.isfinite(loss.value) and abs(loss.value) > 0.1
    assert not torch.equal(th, flow.theta)
    ctx_a.close()
    ctx_b.close()


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["realnvp_d5_K9", "realnvp_d64_K9"])
def test_the_same_call_twice_is_bit_identical(nf, name):
    lib = nf.load_library()
    _, _, flow, tgt, _, _ = make_flow_case(nf, name)
    ctx = new_ctx(nf)
    outs = [torch.zeros(flow.P + 1, device="cuda") for _ in range(2)]
    for out in outs:
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta), None, 97, 97, 5, 0, 0, vp(out)))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all()) and bool(outs[0].any())
    ctx.close()


# ---- 6. refusals and the closure route ---------------------------------------------------------------------------------------------
def refused_everywhere_and_nothing_touched(nf, lib, ctx, flow, tgt, f64):
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out = torch.full((flow.P + 1,), 7.0, dtype=tdt(f64), device="cuda")
    xs = torch.zeros(flow.desc.d * 16, dtype=tdt(f64), device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    val = C.c_double(123.0)
    d = C.byref(flow.desc)
    assert lib.nf_elbo_value_and_grad(ctx.ptr, d, C.byref(tgt.c), vp(th), None, 16, 16, 1, 0, 0, vp(out)) == NF_ERR_UNSUPPORTED
    assert lib.nf_elbo_batch(ctx.ptr, d, C.byref(tgt.c), vp(th), vp(xs), 16, None, C.byref(val)) == NF_ERR_UNSUPPORTED
    assert lib.nf_elbo_batch_rng(ctx.ptr, d, C.byref(tgt.c), vp(th), 16, 1, 0, 0, C.byref(val)) == NF_ERR_UNSUPPORTED
    assert lib.nf_elbo_step(ctx.ptr, d, C.byref(tgt.c), vp(th), vp(m), vp(v), 16, 1, 0, LR, B1, B2, EPS, None, None) == NF_ERR_UNSUPPORTED
    assert lib.nf_elbo_step_enqueue(ctx.ptr, d, C.byref(tgt.c), vp(th), vp(m), vp(v), 16, 1, vp(counter), LR, B1, B2, EPS, None) == NF_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert val.value == 123.0 and bool((out == 7.0).all()) and torch.equal(th, flow.theta) and not bool(m.any()) and not bool(v.any())
    assert int(counter[0]) == 0


def test_flows_with_in_kernel_targets_refuse_and_touch_nothing(nf):
    lib = nf.load_library()
    ctx = new_ctx(nf)
    cases = [(nf.planarflow(nf.MvNormal(5), 4, paramtype=torch.float32, seed=1), False),
             (nf.radialflow(nf.MvNormal(5), 4, paramtype=torch.float32, seed=1), False),
             (nf.meanfield(nf.MvNormal(5), paramtype=torch.float64), True)]
    for flow, f64 in cases:
        refused_everywhere_and_nothing_touched(nf, lib, ctx, flow, make_mixture(nf, 5, 3, f64)[0], f64)
    # a Hamiltonian flow: neither as its score nor as the ELBO target of its joint density
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    g2 = make_mixture(nf, 2, 4, False)[0]
    diag = nf.DiagGaussTarget(torch.zeros(2, device="cuda"), torch.ones(2, device="cuda"))
    buf = torch.zeros(64, device="cuda")
    for score, target in ((g2.c, diag.c), (diag.c, g2.c)):
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
        hd.score = C.cast(C.pointer(score), C.c_void_p)
        assert lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(hd), C.byref(target), vp(buf), None, 16, 16, 1, 0, 0, vp(buf)) == NF_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(buf.any())
    ctx.close()


def test_bad_target_arguments_are_argument_errors(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx = new_ctx(nf)
    flow = nf.realnvp(nf.MvNormal(5), (32, 32), 2, paramtype=torch.float32, seed=2)
    p = torch.zeros(64, device="cuda")
    y = torch.zeros(5 * 8, device="cuda")
    out = torch.empty(flow.P + 1, device="cuda")
    lp = torch.empty(8, device="cuda")
    a = p.data_ptr()
    for t in [Target(8, 0, a, 2.0, 0.0), Target(8, a, 0, 2.0, 0.0), Target(8, a, a, 0.0, 0.0), Target(8, a, a, 2.5, 0.0), Target(8, a, a, 2.0, 1.0)]:
        assert lib.nf_target_logp(ctx.ptr, 0, C.byref(t), 5, 8, vp(y), vp(lp), None) == NF_ERR_ARG, (t.p0, t.p1, t.s0, t.s1)
        assert lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(t), vp(flow.theta), None, 8, 8, 1, 0, 0, vp(out)) == NF_ERR_ARG
    torch.cuda.synchronize()
    ctx.close()


def test_planar_float64_takes_the_tape_route(nf):
    d, nl, n = 2, 10, 37
    flow = nf.planarflow(nf.MvNormal(d), nl, paramtype=torch.float64, seed=3)
    flow = flow.with_theta(flow.theta * 0.3)
    tgt, ref, _, _ = make_mixture(nf, d, 4, True)
    xs = o.base_sample(d, n, 77, 0, 0)
    spec, th = o.FlowSpec("planar", d, nl), flow.theta.cpu().numpy()
    l_ref, g_ref = composed_neg_elbo(spec, th, ref, xs)
    (loss, g), counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, to_dev(xs, True)))
    assert counts == ONE_MIXTURE_LAUNCH, counts  # the device score, through the target's autograd node
    P.scalar("mixture tape planar d2x10 f64: loss", loss, l_ref, P.F64_RTOL)
    P.gradient("mixture tape planar d2x10 f64: grad", g, g_ref, P.F64_GRAD)


# ---- 7. beyond the tiled kernel's d = 64 -------------------------------------------------------------------------------------------
def test_wide_float32_coupling_flow_is_refused_and_nothing_is_touched(nf):
    """64 < d on a Float32 coupling flow (RealNVP d = 70, hidden (128, 100): a weight-streaming shape): there is no chunked form
    of the tiled kernel; every ELBO entry point answers NF_ERR_UNSUPPORTED before any launch."""
    lib = nf.load_library()
    ctx = new_ctx(nf)
    flow = nf.realnvp(nf.MvNormal(70), (128, 100), 2, paramtype=torch.float32, seed=2)
    tgt = make_mixture(nf, 70, 2, False)[0]
    refused_everywhere_and_nothing_touched(nf, lib, ctx, flow, tgt, False)
    ctx.close()


def test_wide_float32_coupling_flow_takes_the_closure_route_in_python(nf):
    """The same flow through value_and_gradient: the library would refuse, so the Python mirror takes the closure route -- library
    forward that keeps its tape, ONE "target_mixture" launch of the flat kernel behind the target's autograd node, library
    pullback -- and matches the composed oracle."""
    d, hd, n = 70, (128, 100), 33
    spec = o.FlowSpec("realnvp", d, 2, hd, 0, 0.0)
    th = o.init_params(spec, np.random.default_rng(3)).astype(np.float32).astype(np.float64)
    flow = nf.Flow("realnvp", nf.MvNormal(d), 2, hd, 0, 0.0, dtype=torch.float32, device="cuda", theta=torch.tensor(th, dtype=torch.float32, device="cuda"))
    tgt, ref, _, _ = make_mixture(nf, d, 2, False)
    check_flow_case(nf, f"mixture closure route realnvp d=70 K=2 N={n}", spec, th, flow, tgt, ref, False, n)


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------
def test_train_flow_on_a_coupling_flow_equals_the_split_loop(nf):
    """train_flow(elbo_batch, realnvp, MixtureTarget, 64) runs nf_elbo_step per iteration and returns the theta and Adam state of
    `optimize` over value_and_gradient + update bit for bit, stats within rel 1e-6."""
    from normalizingflows_jl_amd import objectives as ob

    flow = nf.realnvp(nf.MvNormal(5), (32, 32), 2, paramtype=torch.float32, seed=2)
    tgt, n = make_mixture(nf, 5, 3, False)[0], 64
    assert ob._fused_steps_apply(nf.elbo_batch, flow, [tgt, n], nf.PhiloxRNG(9), None, {})
    fa, sa, sta = nf.train_flow(nf.PhiloxRNG(9), nf.elbo_batch, flow, tgt, n, max_iters=5, optimiser=nf.Adam(2e-3))
    theta0, re = flow.destructure()
    rng_b = nf.PhiloxRNG(9)
    tb, sb, stb = nf.optimize(lambda th: nf.value_and_gradient(nf.elbo_batch, re(th), tgt, n, rng_b), theta0, re, max_iters=5,
                              optimiser=nf.Adam(2e-3))
    assert torch.equal(fa.theta, tb) and torch.equal(sta.m, stb.m) and torch.equal(sta.v, stb.v) and sta.t == stb.t == 5
    assert len(sa) == len(sb) == 5
    for a, b in zip(sa, sb):
        assert a["iteration"] == b["iteration"] and abs(b["loss"]) > 0.1
        assert a["loss"] == pytest.approx(b["loss"], rel=1e-6) and a["gradient_norm"] == pytest.approx(b["gradient_norm"], rel=1e-6)
