"""GPU tests of the cotangent-resident reverse pass (k_affine_bwd_pair, nf_coupling.hip) and of the two removals that came with it.

The producer wave of a pair keeps a tile's cotangent in registers between the two phases of a coupling for the first two tiles it
owns per phase and sends the tiles beyond through memory as before; the coupling processed last skips its input-cotangent work
when the caller is a training step; the stashing fused forward of a training step does not write the flow output.  So:

* loss and gradient of the cfg-2 flow (RealNVP d = 64, 8 couplings, hidden [64, 64]) against the float64 oracle at batch sizes
  that give a pair 1, 2, 3 and 5 tiles per phase ON THE DEVICE AT HAND (the reverse launch uses min(ceil(tiles / 4), CUs)
  workgroups of four pairs), and at one ragged batch (partial last tile, pairs without a tile in the last round) -- both KL
  directions, the suite's tolerances (parity.py: LOSS_RTOL, GRAD_RTOL; no floor);
* the one-call steps equal to the split calls bit for bit at three tiles per pair (parked and unparked tiles);
* callers that DO read the buffers the training steps no longer fill: the pullback's input cotangent (nf_flow_bwd_kept after
  nf_flow_fwd_keep), nf_flow_fwd's y and nf_elbo_batch_rng's value, against the oracle.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from __graft_entry__ import load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

D, HD, NL = 64, (64, 64), 4  # cfg 2's flow: 2 * NL = 8 couplings
TILE = 32
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def vp(t):
    return C.c_void_p(t.data_ptr())


def cm(a, dt=None):
    return torch.tensor(np.ascontiguousarray(a.T), dtype=dt or torch.float32, device="cuda").t()


def rounds_of(n):
    """tiles per pair and phase of the reverse launch for a batch of n (nf_affine_bwd_grid; k_affine_bwd_pair's `rounds`)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ntiles = -(-n // TILE)
    grid = max(1, min(-(-ntiles // 4), cus))
    return -(-ntiles // (4 * grid))


def batch_for(rounds):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = rounds * 4 * cus * TILE
    assert rounds_of(n) == rounds
    return n


def ragged_batch():
    """two rounds, the second with a quarter of the workgroups' pairs idle, the last tile 13 samples short"""
    n = batch_for(2) - (batch_for(1) // 4 // TILE) * TILE - 13
    assert rounds_of(n) == 2 and n % TILE != 0
    return n


SIZES = {"1_tile": lambda: batch_for(1), "2_tiles": lambda: batch_for(2), "3_tiles": lambda: batch_for(3), "5_tiles": lambda: batch_for(5),
         "ragged": ragged_batch}


def make_flow(nf, seed=3):
    flow = nf.realnvp(nf.MvNormal(D), HD, NL, paramtype=torch.float32, seed=seed)
    return flow, o.FlowSpec("realnvp", D, NL, HD), flow.theta.double().cpu().numpy()


def make_target(nf):
    rng = np.random.default_rng(0)
    mu, var = rng.standard_normal(D).astype(np.float32), (rng.uniform(size=D) + 0.5).astype(np.float32)
    tgt = nf.DiagGaussTarget(torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda"))
    return tgt, ("diaggauss", mu.astype(np.float64), var.astype(np.float64))


@pytest.mark.parametrize("size", list(SIZES))
def test_elbo_step_gradient_against_oracle(nf, size):
    """nf_elbo_value_and_grad with in-library draws: fused forward with the stash (no y written), reverse pass from it."""
    n = SIZES[size]()
    flow, spec, th = make_flow(nf)
    tgt, otgt = make_target(nf)
    xs = nf.device_specific_rand(nf.PhiloxRNG(11), flow.dist, n)
    loss, g = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(11))
    lo, go = o.neg_elbo_value_and_grad(spec, th, otgt, xs.double().cpu().numpy())
    print(f"elbo {size}: n = {n}, rounds = {rounds_of(n)}, loss {loss!r} oracle {lo!r}, "
          f"grad err / |g|inf = {np.abs(g.double().cpu().numpy() - go).max() / np.abs(go).max():.3e}")
    P.scalar(f"cotangent residency elbo {size}: loss", loss, lo)
    P.gradient(f"cotangent residency elbo {size}: grad", g, go)


def oracle_fkl(spec, th, ys64, tmp_path):
    """oracle.neg_loglik_value_and_grad over the batch, in chunks on the host's cores (tests/oracle_pool.py, its own process)"""
    fin, fout = os.path.join(tmp_path, "fkl_in.npz"), os.path.join(tmp_path, "fkl_out.npz")
    np.savez(fin, kind=spec.kind, d=spec.d, nlayers=spec.nlayers, hdims=np.asarray(spec.hdims), theta=th, ys=ys64)
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle_pool.py"), fin, fout],
                       capture_output=True, text=True, timeout=3000)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(fout)
    return float(z["loss"]), z["grad"]


@pytest.mark.parametrize("size", list(SIZES))
def test_forward_kl_gradient_against_oracle(nf, size, tmp_path):
    """nf_loglikelihood_value_and_grad: the inverse chain's stash and its reverse pass (the last coupling without dX1)."""
    n = SIZES[size]()
    flow, spec, th = make_flow(nf)
    ys = np.random.default_rng(5).standard_normal((D, n)).astype(np.float32)
    loss, g = nf.value_and_gradient(nf.loglikelihood, flow, None, cm(ys))
    lo, go = oracle_fkl(spec, th, ys.astype(np.float64), str(tmp_path))
    print(f"forward KL {size}: n = {n}, rounds = {rounds_of(n)}, loss {loss!r} oracle {lo!r}, "
          f"grad err / |g|inf = {np.abs(g.double().cpu().numpy() - go).max() / np.abs(go).max():.3e}")
    P.scalar(f"cotangent residency forward KL {size}: loss", loss, lo)
    P.gradient(f"cotangent residency forward KL {size}: grad", g, go)


def test_fused_elbo_step_equals_split_calls_bit_for_bit(nf):
    """nf_elbo_step against nf_elbo_value_and_grad + nf_adam_update on another context at three tiles per pair, two steps."""
    n = batch_for(3)
    flow, _, _ = make_flow(nf)
    tgt, _ = make_target(nf)
    lib = nf.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    ctx_a, ctx_b = nf.Context(0, stream), nf.Context(0, stream)
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(2):
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, 77, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 77, step, LR, B1, B2, EPS,
                                       C.byref(loss), C.byref(gnorm)))
        assert loss.value == pytest.approx(float(out[flow.P]), rel=1e-6) and gnorm.value == pytest.approx(float(gn), rel=1e-6)
    torch.cuda.synchronize()
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    ctx_a.close()
    ctx_b.close()


def test_fused_forward_kl_step_equals_split_calls_bit_for_bit(nf):
    n = batch_for(3)
    flow, _, _ = make_flow(nf)
    ys = cm(np.random.default_rng(5).standard_normal((D, n)))
    lib = nf.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    ctx_a, ctx_b = nf.Context(0, stream), nf.Context(0, stream)
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(2):
        nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx_b.ptr, C.byref(flow.desc), vp(th_b), vp(ys), n, n, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        nf._lib.check(lib.nf_loglikelihood_step(ctx_a.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(ys), n, n, step, LR, B1, B2, EPS,
                                                None, None))
    torch.cuda.synchronize()
    assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b)
    ctx_a.close()
    ctx_b.close()


def test_pullback_input_cotangent_and_forward_outputs_against_oracle(nf):
    """The callers that read what the training steps skip: nf_flow_bwd_kept's xbar (three tiles per pair, random cotangents of y
    and of log|det J|), nf_flow_fwd's y and ladj, and nf_elbo_batch_rng's value on the same draws."""
    n = batch_for(3)
    flow, spec, th = make_flow(nf)
    rng = np.random.default_rng(9)
    xs = rng.standard_normal((D, n)).astype(np.float32).astype(np.float64)
    ybar = (rng.standard_normal((D, n)) / n).astype(np.float32).astype(np.float64)
    lbar = (rng.standard_normal(n) / n).astype(np.float32).astype(np.float64)
    x_t = cm(xs)
    (y, ladj), pullback = nf.flows.rrule_with_logabsdet_jacobian(flow.transform, x_t)
    xbar, g = pullback(cm(ybar), torch.tensor(lbar, dtype=torch.float32, device="cuda"))
    y_ref, l_ref, states = o.flow_fwd(spec, th, xs, keep=True)
    xbar_ref, g_ref = o.flow_bwd(spec, th, states, ybar, lbar)
    th32, xs32, yb32, lb32 = P.f32(th, xs, ybar, lbar)
    y32, l32, st32 = o.flow_fwd(spec, th32, xs32, keep=True)
    fl = o.flow_bwd(spec, th32, st32, yb32, lb32)
    P.gradient("cotangent residency: pullback gtheta", g, g_ref, floor=fl[1])
    P.gradient("cotangent residency: pullback xbar", xbar, xbar_ref, floor=fl[0])
    P.elementwise("cotangent residency: keep-forward ys", y, y_ref, floor=y32)
    y0, l0 = nf.with_logabsdet_jacobian(flow.transform, x_t)
    P.elementwise("cotangent residency: nf_flow_fwd ys", y0, y_ref, floor=y32)
    P.elementwise("cotangent residency: nf_flow_fwd ladj", l0, l_ref, floor=l32)
    tgt, otgt = make_target(nf)
    xr = nf.device_specific_rand(nf.PhiloxRNG(21), flow.dist, n)
    val = nf.elbo_batch(nf.PhiloxRNG(21), flow, tgt, n)
    P.scalar("cotangent residency: nf_elbo_batch_rng", val, o.elbo_batch(spec, th, otgt, xr.double().cpu().numpy()))
