"""The activation stash without u = x1 exp(s) (nf_coupling.hip, the comment above StashGeo).

Only flat coupling ncoup - 1 writes the UV region of its stash slot; every other coupling's reverse pass takes x1 (forward-KL
direction: w1) from the XT region of slot k + 1 and forms u itself.  The slot keeps its size, so the UV region of the other
slots is a hole that nobody may read:

1. the hole is never read -- the tape pullback (and the forward-KL step) give the same bits whatever the caller's buffer held
   before the forward ran (0.0f against 1.0f in every word);
2. the stashed pullback equals the recompute pullback of the same library (nf_ctx_set_stash_budget(0)) at the gradient
   tolerance of tests/parity.py;
3. (no GPU) the phase barrier of the six-term stashing forward, which waits with vmcnt(60) instead of draining the stash
   stores, still has 61 stores behind every image request: StashStores' counts, re-derived here from the geometry, and the
   static_assert that the build exercises.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from __graft_entry__ import ROOT, load_package

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def cm(a, dt=None, dev="cuda"):
    return torch.tensor(np.ascontiguousarray(a.T), dtype=dt or torch.float32, device=dev).t()


# (d, hdims, N): four couplings each (nlayers = 2) -- one without a neighbour, three with
HOLE_SHAPES = [
    (64, (64, 64), 64),        # k_affine_bwd_pair, FULL, one tile per pair
    (64, (64, 64), 32 * 40),   # FULL, 40 tiles: with few workgroups some pairs get a second, parked tile
    (8, (32, 32), 64),         # the one-wavefront kernel k_affine_bwd_stashed
    (8, (32, 32), 32 * 40),
]
GRAD_SHAPES = HOLE_SHAPES + [
    (64, (64, 64), 45),        # a ragged tile
    (63, (64, 64), 64),        # the non-FULL form, c != m
]


def make(nf, d, hd, n, seed=11):
    spec = o.FlowSpec("realnvp", d, 2, hd)
    rng = np.random.default_rng(seed + d + n)
    th = (o.init_params(spec, rng) + 0.03 * rng.standard_normal(o.param_count(spec))).astype(np.float32)
    flow = nf.Flow("realnvp", nf.MvNormal(d), 2, hd, 0, 0.0, dtype=torch.float32, device="cuda", theta=torch.tensor(th, device="cuda"))
    xs = rng.standard_normal((d, n)).astype(np.float32)
    ybar = (rng.standard_normal((d, n)) / n).astype(np.float32)
    lbar = (rng.standard_normal(n) / n).astype(np.float32)
    return flow, xs, ybar, lbar


def _pullback_through_prefilled_tape(nf, flow, xs, ybar, lbar, fill):
    lib, ctx = nf.load_library(), flow.ctx
    d, n = xs.shape
    nb = int(lib.nf_tape_bytes(ctx.ptr, C.byref(flow.desc), n))
    assert nb > 0 and nb % 4 == 0
    tape = torch.full((nb // 4,), fill, dtype=torch.float32, device="cuda")
    x_t, yb_t, lb_t = cm(xs), cm(ybar), torch.tensor(lbar, device="cuda")
    y = nf.new_batch(d, n, torch.float32, "cuda")
    ladj = torch.empty(n, dtype=torch.float32, device="cuda")
    nf._lib.check(lib.nf_flow_fwd_keep(ctx.ptr, C.byref(flow.desc), flow.theta.data_ptr(), x_t.data_ptr(), n, y.data_ptr(), ladj.data_ptr(),
                                       tape.data_ptr(), nb))
    xbar = nf.new_batch(d, n, torch.float32, "cuda")
    g = torch.empty(flow.P, dtype=torch.float32, device="cuda")
    nf._lib.check(lib.nf_flow_bwd_kept(ctx.ptr, C.byref(flow.desc), flow.theta.data_ptr(), tape.data_ptr(), nb, yb_t.data_ptr(), lb_t.data_ptr(),
                                       n, xbar.data_ptr(), g.data_ptr()))
    torch.cuda.synchronize()
    return xbar.clone(), g.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("d,hd,n", HOLE_SHAPES, ids=[f"d{d}_h{hd[0]}_n{n}" for d, hd, n in HOLE_SHAPES])
def test_the_hole_is_never_read(nf, d, hd, n):
    flow, xs, ybar, lbar = make(nf, d, hd, n)
    xb0, g0 = _pullback_through_prefilled_tape(nf, flow, xs, ybar, lbar, 0.0)
    xb1, g1 = _pullback_through_prefilled_tape(nf, flow, xs, ybar, lbar, 1.0)
    assert bool(torch.isfinite(xb0).all()) and bool(torch.isfinite(g0).all())
    assert float(g0.abs().max()) > 0.0
    assert torch.equal(xb0, xb1), "xbar depends on what the tape held before the forward"
    assert torch.equal(g0, g1), "gtheta depends on what the tape held before the forward"


@pytest.mark.gpu
@pytest.mark.parametrize("d,hd,n", HOLE_SHAPES, ids=[f"d{d}_h{hd[0]}_n{n}" for d, hd, n in HOLE_SHAPES])
def test_the_hole_is_never_read_in_the_inverse_direction(nf, d, hd, n):
    """Forward-KL: the inverse chain's stash lives in the context's arena; here the caller owns the arena and prefills it.  Both the
    split sequence (nf_loglikelihood_value_and_grad) and the fused step (nf_loglikelihood_step) run on it."""
    flow, xs, _, _ = make(nf, d, hd, n)
    lib = nf.load_library()
    ys = torch.tensor(np.ascontiguousarray(xs.T), device="cuda").t()  # d x N, column-major
    res = []
    for fill in (0.0, 1.0):
        ctx = nf.Context(0, torch.cuda.current_stream().cuda_stream)
        ws = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), n))
        arena = torch.full((ws // 4 + 64,), fill, dtype=torch.float32, device="cuda")
        nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, arena.data_ptr(), ws))
        out = torch.empty(flow.P + 1, dtype=torch.float32, device="cuda")
        nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx.ptr, C.byref(flow.desc), flow.theta.data_ptr(), ys.data_ptr(), n, n, out.data_ptr()))
        torch.cuda.synchronize()
        out = out.clone()
        arena.fill_(fill)
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
        st = lib.nf_loglikelihood_step(ctx.ptr, C.byref(flow.desc), th.data_ptr(), m.data_ptr(), v.data_ptr(), ys.data_ptr(), n, n, 0,
                                       1e-3, 0.9, 0.999, 1e-8, None, None)
        nf._lib.check(st)
        torch.cuda.synchronize()
        nf._lib.check(lib.nf_ctx_set_arena(ctx.ptr, None, 0))
        ctx.close()
        res.append((out, th, m, v))
    for a, b in zip(*res):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, b), "the forward-KL gradient depends on what the arena held before the step"
    assert float(res[0][2].abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("d,hd,n", GRAD_SHAPES, ids=[f"d{d}_h{hd[0]}_n{n}" for d, hd, n in GRAD_SHAPES])
def test_same_gradient_as_the_recompute_path(nf, d, hd, n):
    flow, xs, ybar, lbar = make(nf, d, hd, n)
    lib, ctx = nf.load_library(), flow.ctx
    x_t, yb_t, lb_t = cm(xs), cm(ybar), torch.tensor(lbar, device="cuda")
    _, pullback = nf.flows.rrule_with_logabsdet_jacobian(flow.transform, x_t)
    xbar, g = pullback(yb_t, lb_t)
    try:
        nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, 0))
        _, pullback0 = nf.flows.rrule_with_logabsdet_jacobian(flow.transform, x_t)
        xbar0, g0 = pullback0(yb_t, lb_t)
    finally:
        nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, -1))
    key = f"stash without u d{d} h{hd[0]} n{n}: stashed against recompute pullback"
    P.gradient(key + " gtheta", g, g0, P.GRAD_RTOL)
    P.gradient(key + " xbar", xbar, xbar0, P.GRAD_RTOL)


# ---- 3. bookkeeping (no GPU) ---------------------------------------------------------------------------------

def _stash_stores(mb, h1b, h2b, cb, slim):
    """Store instructions per wave and phase of a coupling that does not keep UV, from what each phase stores: element stores for
    the T-layout arrays (16 per 32-feature block), 16-byte stores for the lane-layout ones (4 per block), one mask word."""
    act = (0 if slim else h1b * 16) + h2b * 16 + 1
    return mb * 16 + (mb * 4 if slim else 0) + act, act + cb * 4


def test_phase_barrier_keeps_61_stores_behind_every_image_request():
    src = open(os.path.join(ROOT, "normalizingflows.jl_amd", "csrc", "nf_coupling.hip")).read()
    # the constants the source exposes are the formulas re-derived above ...
    m = re.search(r"struct StashStores \{(.*?)\};", src, re.S)
    assert m, "StashStores is gone"
    body = re.sub(r"\s+", " ", m.group(1))
    assert "ACT = (SLIM ? 0 : G::H1B * 16) + G::H2B * 16 + 1;" in body
    assert "S_NET = G::MB * 16 + (SLIM ? G::MB * 4 : 0) + ACT;" in body
    assert "T_NET = ACT + G::CB * 4;" in body
    # ... the kernel asserts on them where it waits with vmcnt(60) ...
    assert re.search(r"static_assert\(!STASH \|\| StashStores<G, SLIM>::S_NET \+ StashStores<G, SLIM>::T_NET >= 61,", src)
    assert "__builtin_amdgcn_s_waitcnt(0xC07C);  // vmcnt(60) lgkmcnt(0)" in src
    # ... and every geometry that takes this path has them: an image is requested two phases (one s net, one t net) ahead
    for name, geo, slim in (("hidden 64", (1, 2, 2, 1), False), ("hidden 32", (1, 1, 1, 1), False), ("hidden 64, SLIM", (1, 2, 2, 1), True)):
        s_net, t_net = _stash_stores(*geo, slim)
        assert s_net + t_net >= 61, (name, s_net, t_net)
    assert _stash_stores(1, 2, 2, 1, False) == (81, 69)  # hidden 64 has the margin in either phase alone
    # the build compiles the static_assert in every stashing instantiation
    import __graft_entry__ as ge

    ge.build()
    assert os.path.exists(ge.LIB)
