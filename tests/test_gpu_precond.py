"""GPU parity of the preconditioned coupling flow (NF_KIND_PRECOND: y = mu + L T(x), T a RealNVP / NSF chain) against the
numpy reference tests/precond_ref.py (validated against central differences in test_precond_cpu.py), on the cases of
precond_ref.CASES: one per tape kind of the inner flow, the envelope, the standard-layout Float32 route, Float64, the loop
over tiles and a single sample.  The strict upper triangle of L is NaN wherever a test does not run Adam: it is never read.
The two arms of the full-rank layer's reverse pass (one launch; the two launches of NF_KIND_FULLRANK) must agree bit for bit:
NF_PRECOND_BWD_SPLIT=0 / 1 force one or the other at every d, each in a process of its own, next to the default dispatch (the
two launches at d <= 32, where the one launch measured slower; the one launch beyond)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fullrank_cases as fc
import nf_oracle as o
import parity as P
import precond_ref as pr
from __graft_entry__ import ROOT, load_package
from test_gpu_fullrank import bits, device_target, host, tag, vec
from test_gpu_linpred import new_ctx, prof_counts, tdt, to_dev, vp

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
TILED = ["stash", "spline", "recompute", "wide"]  # Float32, inner flow on the matrix-pipe kernels: one per tape kind
F64_CASES = ["stash", "wide"]  # 5 x 70 and 70 x 40 in Float64


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def spec_n(name):
    if name == "grid-stride":
        return pr.GRID_STRIDE_SPEC, 32 * torch.cuda.get_device_properties(0).multi_processor_count + 33
    return pr.CASES[name]


def make_flow(nf, spec, theta, f64):
    q0 = nf.MvNormal(spec.d)
    if spec.kind == "realnvp":
        inner = nf.realnvp(q0, spec.hdims, spec.nlayers, paramtype=tdt(f64))
    else:
        inner = nf.nsf(q0, spec.hdims, spec.K, spec.B, spec.nlayers, paramtype=tdt(f64))
    flow = nf.preconditioned(inner)
    assert flow.P == theta.size
    return flow.with_theta(vec(theta, f64))


_CASES = {}


def case(nf, name, f64, nan_upper=True):
    """(spec, n, theta, x, flow, xs) -- computed once per (case, element type) and left unchanged"""
    key = (name, f64, nan_upper)
    if key not in _CASES:
        spec, n = spec_n(name)
        theta, x = pr.inputs(spec, n, f64, nan_upper=nan_upper)
        _CASES[key] = (spec, n, theta, x, make_flow(nf, spec, theta, f64), to_dev(x, f64))
    return _CASES[key]


def ids(names_f64):
    return [f"{n}-{tag(f)}" for n, f in names_f64]


def cases(names32, with_f64=True):
    out = [(n, False) for n in names32] + ([(n, True) for n in F64_CASES] if with_f64 else [])
    return pytest.mark.parametrize("name,f64", out, ids=ids(out))


def f32(*a):
    return tuple(v.astype(np.float32) for v in a)


# ---- 1. forward, inverse, layers, rand, logpdf -------------------------------------------------------------------------------------
@cases(TILED + ["flat32", "single"])
def test_forward_inverse_layers_rand_logpdf(nf, name, f64):
    spec, n, theta, x, flow, xs = case(nf, name, f64)
    key = f"precond {name} {tag(f64)}"
    y, ladj = nf.with_logabsdet_jacobian(flow.transform, xs)
    torch.cuda.synchronize()
    y_ref, l_ref = pr.fwd(spec, theta, x)
    assert np.isfinite(host(y)).all() and np.isfinite(host(ladj)).all(), key
    t32, x32 = f32(theta, x)
    if f64:
        P.elementwise(key + ": y", y, y_ref, P.F64_RTOL, 1e-12)
        P.elementwise(key + ": ladj", ladj, l_ref, P.F64_RTOL, 1e-12)
    else:
        y32, l32 = pr.fwd(spec, t32, x32)
        P.elementwise(key + ": y", y, y_ref, floor=y32)
        P.elementwise(key + ": ladj", ladj, l_ref, floor=l32)
    # round trip, norm-wise at the inner kind's tolerance, and ladj_inv = -ladj
    xr, lr = nf.with_logabsdet_jacobian(nf.inverse(flow.transform), y)
    if f64:
        P.isapprox(key + ": round trip x", xr, x, P.F64_GRAD)
        P.isapprox(key + ": round trip ladj", lr, -host(ladj), P.F64_GRAD)
    else:
        xr32, lr32 = pr.inv(spec, t32, y32)
        P.isapprox(key + ": round trip x", xr, x, P.INV_RTOL[spec.kind], floor_err=P.relerr(xr32, x))
        P.isapprox(key + ": round trip ladj", lr, -host(ladj), P.INV_RTOL[spec.kind], floor_err=P.relerr(lr32, -l32.astype(np.float64)))
    # single bijectors in flat order: 0 = Shift, 1 = Scale, 2 = the outermost coupling
    for i in (0, 1, 2):
        yi, li = nf.with_logabsdet_jacobian(nf.layer(flow, i), xs)
        yi_ref, li_ref = pr.layer(spec, theta, i, x)
        if f64:
            P.elementwise(f"{key}: layer {i} y", yi, yi_ref, P.F64_RTOL, 1e-12)
            P.elementwise(f"{key}: layer {i} ladj", li, li_ref, P.F64_RTOL, 1e-12)
        else:
            yi32, li32 = pr.layer(spec, t32, i, x32)
            P.elementwise(f"{key}: layer {i} y", yi, yi_ref, floor=yi32)
            P.elementwise(f"{key}: layer {i} ladj", li, li_ref, floor=li32)
    # rand: the forward of the base draws, bit for bit
    ys = nf.rand(flow, n, nf.PhiloxRNG(9))
    xd = nf.device_specific_rand(nf.PhiloxRNG(9), flow.dist, n, dtype=tdt(f64))
    yd, _ = nf.with_logabsdet_jacobian(flow.transform, xd)
    torch.cuda.synchronize()
    assert bits(ys) == bits(yd) and np.isfinite(host(ys)).all(), key
    # logpdf(flow, y) at the flow's own outputs (as the device holds them)
    yh = host(y)
    lp = nf.logpdf(flow, y)
    lp_ref = pr.logpdf(spec, theta, yh)
    if f64:
        P.elementwise(key + ": logpdf", lp, lp_ref, P.F64_RTOL, 1e-12)
    else:
        P.elementwise(key + ": logpdf", lp, lp_ref, floor=pr.logpdf(spec, t32, yh.astype(np.float32)))


# ---- 2. the tape pair ----------------------------------------------------------------------------------------------------------------
@cases(TILED + ["envelope", "grid-stride"])
def test_tape_pullback(nf, name, f64):
    spec, n, theta, x, flow, xs = case(nf, name, f64)
    d = spec.d
    key = f"precond pullback {name} {tag(f64)}"
    rng = np.random.default_rng(8)
    ybar64, lbar64 = fc.rounded(rng.standard_normal((d, n)), f64), fc.rounded(rng.standard_normal(n), f64)
    ybar, lbar = to_dev(ybar64, f64), vec(lbar64, f64)
    (y, ladj), pullback = nf.rrule_with_logabsdet_jacobian(flow.transform, xs)
    xbar, g = pullback(ybar, lbar)
    torch.cuda.synchronize()
    _, _, tape = pr.fwd(spec, theta, x, keep=True)
    xbar_ref, g_ref = pr.bwd(spec, theta, tape, ybar64, lbar64)
    up = pr.upper_mask(spec)
    g_ref = np.where(up, 0.0, g_ref)  # (NaN inputs above the diagonal: the reference's zeros there)
    if f64:
        P.gradient(key + ": xbar", xbar, xbar_ref, P.F64_GRAD)
        P.gradient(key + ": gtheta", g, g_ref, P.F64_GRAD)
    else:
        t32, x32, yb32, lb32 = f32(theta, x, ybar64, lbar64)
        _, _, tape32 = pr.fwd(spec, t32, x32, keep=True)
        xb32, g32 = pr.bwd(spec, t32, tape32, yb32, lb32)
        P.gradient(key + ": xbar", xbar, xbar_ref, floor=xb32)
        P.gradient(key + ": gtheta", g, g_ref, floor=np.where(up, 0.0, g32))
    upt = torch.tensor(up, device="cuda")
    assert bool((g[upt] == 0.0).all()), key  # exactly 0.0 above the diagonal
    # zeros in place of the NaNs: no bit changes
    flow0 = flow.with_theta(vec(pr.zero_upper(spec, theta), f64))
    (y0, l0), pullback0 = nf.rrule_with_logabsdet_jacobian(flow0.transform, xs)
    xbar0, g0 = pullback0(ybar, lbar)
    torch.cuda.synchronize()
    assert bits(y0) == bits(y) and bits(l0) == bits(ladj) and bits(xbar0) == bits(xbar) and bits(g0) == bits(g), key
    # a second pullback from the same tape: the same bits
    xbar2, g2 = pullback(ybar, lbar)
    assert bits(xbar2) == bits(xbar) and bits(g2) == bits(g), key


# ---- 3. ELBO value and gradient: caller's draws and in-library draws ----------------------------------------------------------------
def check_vg(nf, key, spec, theta, x, flow, xs, tgt, ref, f64, loss, grad):
    l_ref, g_ref = pr.neg_elbo_value_and_grad(spec, theta, x, ref)
    up = pr.upper_mask(spec)
    g_ref = np.where(up, 0.0, g_ref)
    assert np.isfinite(loss) and np.isfinite(host(grad)).all(), key
    if f64:
        P.scalar(key + ": loss", loss, l_ref, P.F64_RTOL)
        P.gradient(key + ": gradient", grad, g_ref, P.F64_GRAD)
    else:
        l32, g32 = pr.neg_elbo_value_and_grad(spec, *f32(theta, x), ref)
        P.scalar(key + ": loss", loss, l_ref, floor=l32)
        P.gradient(key + ": gradient", grad, g_ref, floor=np.where(up, 0.0, g32))
    assert bool((grad[torch.tensor(up, device="cuda")] == 0.0).all()), key


def targets_of(name, d):
    extra = ["glm_poisson", "funnel"] + (["mixture3"] if d <= 64 else [])
    return ["diaggauss"] + (extra if name in ("stash", "spline", "wide") else [])


@cases(TILED + ["envelope", "flat32", "grid-stride", "single"])
def test_elbo_value_and_gradient(nf, name, f64):
    spec, n, theta, x, flow, xs = case(nf, name, f64)
    for tname in targets_of(name, spec.d):
        tgt, ref = device_target(nf, tname, spec.d, f64)
        key = f"precond vg {name} {tname} {tag(f64)}"
        loss, grad = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
        torch.cuda.synchronize()
        check_vg(nf, key + " xs", spec, theta, x, flow, xs, tgt, ref, f64, loss, grad)
        # per-sample terms and the value-only entry points
        e = nf.batched_elbos(flow, tgt, xs)
        e_ref = pr.elbos(spec, theta, x, ref)
        if f64:
            P.elementwise(key + ": elbo terms", e, e_ref, P.F64_RTOL, 1e-12)
        else:
            P.elementwise(key + ": elbo terms", e, e_ref, floor=pr.elbos(spec, *f32(theta, x), ref))
        # in-library draws: the reference on the same draws
        seed = 41
        l_rng, g_rng = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
        xd = nf.device_specific_rand(nf.PhiloxRNG(seed), flow.dist, n, dtype=tdt(f64))
        torch.cuda.synchronize()
        check_vg(nf, key + " rng", spec, theta, host(xd), flow, xd, tgt, ref, f64, l_rng, g_rng)


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------
@cases(["stash", "wide"])
def test_two_shards_sum_to_the_whole_batch(nf, name, f64):
    spec, n, theta, x, flow, _ = case(nf, name, f64)
    tgt, _ = device_target(nf, "diaggauss", spec.d, f64)
    key = f"precond shards {name} {tag(f64)}"
    seed = 43
    l_all, g_all = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(seed))
    n_a = (2 * n) // 3
    l_a, g_a = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n_a, rng=nf.PhiloxRNG(seed), n_global=n)
    l_b, g_b = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n - n_a, rng=nf.PhiloxRNG(seed, sample_offset=n_a), n_global=n)
    P.scalar(key + ": loss", l_a + l_b, l_all, P.F64_RTOL if f64 else P.LOSS_RTOL)
    P.gradient(key + ": gradient", g_a + g_b, host(g_all), P.F64_GRAD if f64 else P.GRAD_RTOL)


# ---- 5. the two arms of the full-rank layer's reverse pass ------------------------------------------------------------------------
ARM_CASES = ["stash", "wide", "envelope", "grid-stride"]
ARM_LABELS = ("layout_convert", "fr_gemm", "fr_bwd_x", "fr_bwd", "target")


def arm_digests(nf):
    """sha256 of loss and gradient of nf_elbo_value_and_grad (in-library draws and the caller's) and of the tape pullback per
    case, and the launch counts of one in-library-draws call -- whatever arm this process runs"""
    out = {}
    for name in ARM_CASES:
        spec, n, theta, x, flow, xs = case(nf, name, False)
        tgt, _ = device_target(nf, "diaggauss", spec.d, False)
        l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(5))
        l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
        rng = np.random.default_rng(8)
        ybar, lbar = to_dev(rng.standard_normal((spec.d, n)), False), vec(rng.standard_normal(n), False)
        _, pullback = nf.rrule_with_logabsdet_jacobian(flow.transform, xs)
        xbar, g3 = pullback(ybar, lbar)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (g1, g2, xbar, g3):
            h.update(bits(t))
        h.update(np.array([l1, l2]).tobytes())
        _, counts = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(5)), ARM_LABELS)
        out[name] = {"sha": h.hexdigest(), "counts": counts}
    return out


_ARM_SNIPPET = r"""
import json, os, sys
root = os.environ["NF_ROOT"]
for p in (root, os.path.join(root, "tests"), os.path.join(root, "oracle")):
    sys.path.insert(0, p)
from __graft_entry__ import load_package
import test_gpu_precond as t
print(json.dumps(t.arm_digests(load_package())))
"""


FUSED = {"layout_convert": 0, "fr_gemm": 1, "fr_bwd_x": 1, "fr_bwd": 0, "target": 1}
SPLIT = {"layout_convert": 0, "fr_gemm": 2, "fr_bwd_x": 0, "fr_bwd": 1, "target": 1}


def default_arm(d):
    """the measured dispatch: the two launches where there is one 32-feature block, the one launch beyond"""
    return SPLIT if d <= 32 else FUSED


def test_the_two_reverse_arms_agree_bit_for_bit(nf):
    assert os.environ.get("NF_PRECOND_BWD_SPLIT") is None, "this process must run the default dispatch"
    here = arm_digests(nf)
    forced = {}
    for arm in ("0", "1"):
        e = dict(os.environ, NF_ROOT=ROOT, NF_PRECOND_BWD_SPLIT=arm)
        p = subprocess.run([sys.executable, "-c", _ARM_SNIPPET], env=e, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        forced[arm] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    for name in ARM_CASES:
        assert forced["0"][name]["counts"] == FUSED, (name, forced["0"][name])
        assert forced["1"][name]["counts"] == SPLIT, (name, forced["1"][name])
        assert here[name]["counts"] == default_arm(spec_n(name)[0].d), (name, here[name])
        assert forced["0"][name]["sha"] == forced["1"][name]["sha"] == here[name]["sha"], name


# ---- 6. launch shape: the tiled Float32 sequence never leaves the tile layout ------------------------------------------------------
@pytest.mark.parametrize("name", TILED)
def test_launch_shape_of_the_tiled_sequence(nf, name):
    spec, n, theta, x, flow, xs = case(nf, name, False)
    tgt, _ = device_target(nf, "diaggauss", spec.d, False)
    _, c = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(3)), ARM_LABELS)
    assert c == default_arm(spec.d), (name, c)
    _, c = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs), ARM_LABELS)
    assert c == dict(default_arm(spec.d), layout_convert=1), (name, c)
    if name in ("stash", "wide"):  # a linear-predictor target has a launch of its own
        glm, _ = device_target(nf, "glm_poisson", spec.d, False)
        _, c = prof_counts(nf, flow.ctx, lambda: nf.value_and_gradient(nf.elbo_batch, flow, glm, n, rng=nf.PhiloxRNG(3)),
                           ARM_LABELS + ("target_linpred",))
        assert c["layout_convert"] == 0 and c["fr_bwd_x"] == default_arm(spec.d)["fr_bwd_x"] and c["target_linpred"] + c["target"] == 1, (name, c)


# ---- 7. the step -------------------------------------------------------------------------------------------------------------------
@cases(["stash", "spline"])
def test_elbo_step_equals_the_split_calls(nf, name, f64):
    """two nf_elbo_step calls == nf_elbo_value_and_grad + nf_adam_update on a second context, bit for bit in theta, m, v; the
    upper triangle (zeros here) stays exactly zero; the graph form refuses and touches nothing"""
    lib = nf.load_library()
    spec, n, theta, x, flow, _ = case(nf, name, f64, nan_upper=False)
    tgt, _ = device_target(nf, "glm_poisson" if name == "stash" else "diaggauss", spec.d, f64)
    seed, dt = 77, 1 if f64 else 0
    ctx_a, ctx_b = new_ctx(nf), new_ctx(nf)
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = lib.nf_elbo_step_enqueue(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, vp(counter), LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert code == -2 and torch.equal(th, flow.theta) and int(counter[0]) == 0
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, dtype=tdt(f64), device="cuda"), torch.empty(1, dtype=tdt(f64), device="cuda")
    up = torch.tensor(pr.upper_mask(spec), device="cuda")
    for step in range(2):
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, seed, step, LR, B1, B2, EPS,
                                       C.byref(loss), C.byref(gnorm)))
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, seed, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, dt, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), step
        assert loss.value == float(out[flow.P]) and gnorm.value == float(gn), step
        assert np.isfinite(loss.value)
        assert bool((th[up] == 0.0).all()) and bool((m[up] == 0.0).all()) and bool((v[up] == 0.0).all()), step
    assert not torch.equal(th, flow.theta)
    ctx_a.close()
    ctx_b.close()


# ---- 8. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stash", "wide", "grid-stride"])
def test_two_calls_give_the_same_bits(nf, name):
    spec, n, theta, x, flow, xs = case(nf, name, False)
    tgt, _ = device_target(nf, "diaggauss", spec.d, False)
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(11))
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(11))
    assert l1 == l2 and bits(g1) == bits(g2), name
    l3, g3 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    l4, g4 = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs)
    assert l3 == l4 and bits(g3) == bits(g4), name


# ---- 9. training and the identity preconditioner ----------------------------------------------------------------------------------
def test_training_from_a_fullrank_warm_start(nf):
    d = 5
    tgt, _ = device_target(nf, "glm_poisson", d, False)
    q0 = nf.MvNormal(d)
    fr_flow, _, _ = nf.train_flow(nf.elbo_batch, nf.fullrank(q0, paramtype=torch.float32), tgt, 1024, max_iters=5, optimiser=nf.Adam(0.05))
    flow = nf.preconditioned(nf.realnvp(q0, (32, 32), 2, paramtype=torch.float32), init=fr_flow)
    assert bits(flow.theta[: d + d * d]) == bits(fr_flow.theta)
    trained, stats, _ = nf.train_flow(nf.elbo_batch, flow, tgt, 1024, max_iters=5, optimiser=nf.Adam(0.05))
    losses = [s["loss"] for s in stats]
    print(f"precond training: losses {losses}")
    assert trained.kind == "preconditioned" and len(stats) == 5 and all(np.isfinite(l) for l in losses)
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("name", ["stash", "spline", "wide"])
def test_identity_preconditioner_equals_the_inner_flow(nf, name):
    spec, n, theta, x, flow, xs = case(nf, name, False)
    inner = flow.inner.with_theta(flow.theta[pr.head(spec.d):].clone())
    ident = nf.preconditioned(inner)
    y, ladj = nf.with_logabsdet_jacobian(ident.transform, xs)
    y0, l0 = nf.with_logabsdet_jacobian(inner.transform, xs)
    P.elementwise(f"precond identity {name}: y", y, host(y0))
    P.elementwise(f"precond identity {name}: ladj", ladj, host(l0))
    lp, lp0 = nf.logpdf(ident, y0), nf.logpdf(inner, y0)
    P.elementwise(f"precond identity {name}: logpdf", lp, host(lp0))


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_refusals_raise(nf, f64):
    spec, n, theta, x, flow, xs = case(nf, "stash", f64)
    with pytest.raises(nf.NFHipError):
        nf.loglikelihood_value_and_gradient(flow, xs)
    with pytest.raises(nf.NFHipError):
        nf.train_flow(nf.loglikelihood, flow, xs, max_iters=1)
    with pytest.raises(nf.NFHipError):
        nf.create_flow([flow, nf.planarflow(nf.MvNormal(spec.d), 2, paramtype=tdt(f64))], nf.MvNormal(spec.d))
    assert np.isfinite(nf.loglikelihood(None, flow, xs))  # the value is served
