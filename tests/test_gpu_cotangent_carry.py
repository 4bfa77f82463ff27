"""GPU tests of the cotangent carry across coupling boundaries (k_affine_bwd_pair, nf_coupling.hip) and of the B6T images the
fused epilogue writes (k_affine_epilogue, nf_pack.h).

The producer wave of a pair keeps the conditioner half's outgoing cotangent of a coupling in registers and uses it as the
transformed half's cotangent of the coupling it processes next, for the first two tiles it owns per phase; slot 0 no longer
stores that half between couplings.  A flow of four couplings has three boundaries (carry -> park -> carry), so:

* loss and gradient of nf_elbo_value_and_grad (in-library draws) and the pullback nf_flow_fwd_keep + nf_flow_bwd_kept -- whose
  input cotangent is what the coupling processed last stores -- against the float64 oracle at 1, 2 and 3 tiles per pair and phase
  ON THE DEVICE AT HAND and at one ragged batch, and at d = 62 (the form with feature masks) with 2 tiles; the suite's tolerances
  (parity.py: LOSS_RTOL, GRAD_RTOL; no floor);
* nf_elbo_step / nf_loglikelihood_step under nf_ctx_set_weight_cache(ctx, 1), three consecutive steps at three tiles per pair,
  equal bit for bit in theta, m and v to the split calls from the same start: steps 2 and 3 of the fused form run their reverse
  pass on the triples the epilogue wrote, the split calls on converted ones.  (The epilogue's triples were measured and not
  shipped; the comparison stands for whatever writes the images.)

The float64 oracle is a reference only away from the kinks of the leaky-ReLU hidden units: a sample with a hidden pre-activation
within float32 rounding of zero may take the other slope on the device, which changes that sample's derivatives by a finite
amount (measured on an MI355X, this library and the commit before alike: of 32 768 samples the two with |z| = 1.9e-08 and 4.3e-08
carry input-cotangent errors of 0.8e-2 and 1.2e-2 of the largest element while every other sample is within 6.5e-07, and the
ELBO gradient's error is 1.096e-04 of |g|inf with all draws and 9.3e-08 without the 35 draws that have a |z| < 1e-06).  So the
comparisons are made where the reference is one: KINK_MARGIN bounds the device's pre-activation error from above (a 64-term
float32 dot product of O(1) terms: 64 * 2^-23 = 0.8e-05), and samples with a hidden |z| below it, by the ORACLE's forward pass,
are kept out -- the pullback draws its inputs without them; the ELBO call, whose draws are the library's, is compared on the
rest of its batch: its gradient minus the device's own gradient of the near-kink draws alone (a per-sample computation, so the
same slopes), against the oracle's gradient of the other draws, in units of the whole batch's |g|inf.  Bounds, batch sizes and
calls are unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from gradient_floors import min_abs_preact
from __graft_entry__ import load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HD, NL = (64, 64), 2  # four couplings: three boundaries
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


# (features, batch): d = 62 takes the kernel's form with sample / feature masks at a whole number of tiles
CASES = {"1_tile": (64, lambda: batch_for(1)), "2_tiles": (64, lambda: batch_for(2)), "3_tiles": (64, lambda: batch_for(3)),
         "ragged": (64, ragged_batch), "d62_2_tiles": (62, lambda: batch_for(2))}


def make_flow(nf, d, seed=3):
    flow = nf.realnvp(nf.MvNormal(d), HD, NL, paramtype=torch.float32, seed=seed)
    return flow, o.FlowSpec("realnvp", d, NL, HD), flow.theta.double().cpu().numpy()


KINK_MARGIN = 1e-5


def make_target(nf, d):
    rng = np.random.default_rng(0)
    mu, var = rng.standard_normal(d).astype(np.float32), (rng.uniform(size=d) + 0.5).astype(np.float32)
    tgt = nf.DiagGaussTarget(torch.tensor(mu, device="cuda"), torch.tensor(var, device="cuda"))
    return tgt, ("diaggauss", mu.astype(np.float64), var.astype(np.float64))


@pytest.mark.parametrize("case", list(CASES))
def test_elbo_gradient_against_oracle(nf, case):
    d, size = CASES[case]
    n = size()
    flow, spec, th = make_flow(nf, d)
    tgt, otgt = make_target(nf, d)
    xs = nf.device_specific_rand(nf.PhiloxRNG(11), flow.dist, n)
    loss, g = nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(11))
    x64 = xs.double().cpu().numpy()
    lo, go = o.neg_elbo_value_and_grad(spec, th, otgt, x64)
    near = min_abs_preact(spec, th, x64) < KINK_MARGIN
    k = int(near.sum())
    g_rest, go_rest = g.double().cpu().numpy(), go
    if k:  # the near-kink draws' share of the mean, taken out on both sides
        _, g_near = nf.value_and_gradient(nf.elbo_batch, flow, tgt, cm(x64[:, near]))
        _, go_near = o.neg_elbo_value_and_grad(spec, th, otgt, x64[:, near])
        g_rest, go_rest = g_rest - (k / n) * g_near.double().cpu().numpy(), go - (k / n) * go_near
    scale = np.abs(go).max()
    err_all, err = np.abs(g.double().cpu().numpy() - go).max() / scale, np.abs(g_rest - go_rest).max() / scale
    print(f"carry elbo {case}: d = {d}, n = {n}, rounds = {rounds_of(n)}, loss {loss!r} oracle {lo!r}, near-kink draws {k}, "
          f"grad err / |g|inf = {err:.3e} (with the near-kink draws {err_all:.3e})")
    P.scalar(f"cotangent carry elbo {case}: loss", loss, lo, rtol=P.LOSS_RTOL)
    P.record(f"cotangent carry elbo {case}: grad [max abs err / |g|inf]", err)
    assert err <= P.GRAD_RTOL, f"gradient error {err:.3e} of |g|inf > {P.GRAD_RTOL:.3e}"


@pytest.mark.parametrize("case", list(CASES))
def test_pullback_against_oracle(nf, case):
    """nf_flow_fwd_keep + nf_flow_bwd_kept: the parameter gradient and the input cotangent, whose two halves are the last processed
    coupling's stores (its x1bar and its closing value).  The cotangents have one sign per feature (|normal| / n, alternating by
    feature) and lbar is negative throughout, as a mean objective's are: a parameter gradient is a sum over the batch, and with
    zero-mean random cotangents that sum cancels to ~ 1 / sqrt(n) of its terms, so that float32 rounding of the terms alone exceeds
    GRAD_RTOL of the result whatever the kernel does.  The inputs are standard normal draws without those that the oracle finds
    within KINK_MARGIN of a hidden unit's kink (about one in a hundred)."""
    d, size = CASES[case]
    n = size()
    flow, spec, th = make_flow(nf, d)
    rng = np.random.default_rng(9)
    cand = rng.standard_normal((d, n + n // 16 + 256)).astype(np.float32).astype(np.float64)
    xs = cand[:, min_abs_preact(spec, th, cand) >= KINK_MARGIN][:, :n]
    assert xs.shape[1] == n
    sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)[:, None]
    ybar = (sign * np.abs(rng.standard_normal((d, n))) / n).astype(np.float32).astype(np.float64)
    lbar = (-(0.5 + rng.uniform(size=n)) / n).astype(np.float32).astype(np.float64)
    _, pullback = nf.flows.rrule_with_logabsdet_jacobian(flow.transform, cm(xs))
    xbar, g = pullback(cm(ybar), torch.tensor(lbar, dtype=torch.float32, device="cuda"))
    _, _, states = o.flow_fwd(spec, th, xs, keep=True)
    xbar_ref, g_ref = o.flow_bwd(spec, th, states, ybar, lbar)
    print(f"carry pullback {case}: d = {d}, n = {n}, rounds = {rounds_of(n)}, "
          f"gtheta err / |g|inf = {np.abs(g.double().cpu().numpy() - g_ref).max() / np.abs(g_ref).max():.3e}, "
          f"xbar err / |xbar|inf = {np.abs(xbar.double().cpu().numpy() - xbar_ref).max() / np.abs(xbar_ref).max():.3e}")
    P.gradient(f"cotangent carry pullback {case}: gtheta", g, g_ref, rtol=P.GRAD_RTOL)
    P.gradient(f"cotangent carry pullback {case}: xbar", xbar, xbar_ref, rtol=P.GRAD_RTOL)


def test_fused_elbo_steps_equal_split_calls_bit_for_bit(nf):
    n = batch_for(3)
    flow, _, _ = make_flow(nf, 64)
    tgt, _ = make_target(nf, 64)
    lib = nf.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    ctx_a, ctx_b = nf.Context(0, stream), nf.Context(0, stream)
    nf._lib.check(lib.nf_ctx_set_weight_cache(ctx_a.ptr, 1))
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(3):
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx_b.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, 77, 0, step, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx_a.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 77, step, LR, B1, B2, EPS,
                                       C.byref(loss), C.byref(gnorm)))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), f"step {step + 1}"
    ctx_a.close()
    ctx_b.close()


def test_fused_forward_kl_steps_equal_split_calls_bit_for_bit(nf):
    n = batch_for(3)
    flow, _, _ = make_flow(nf, 64)
    ys = cm(np.random.default_rng(5).standard_normal((64, n)))
    lib = nf.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    ctx_a, ctx_b = nf.Context(0, stream), nf.Context(0, stream)
    nf._lib.check(lib.nf_ctx_set_weight_cache(ctx_a.ptr, 1))
    th_b, m_b, v_b = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    out, gn = torch.empty(flow.P + 1, device="cuda"), torch.empty(1, device="cuda")
    th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
    for step in range(3):
        nf._lib.check(lib.nf_loglikelihood_value_and_grad(ctx_b.ptr, C.byref(flow.desc), vp(th_b), vp(ys), n, n, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx_b.ptr, 0, vp(th_b), vp(out), vp(m_b), vp(v_b), flow.P, LR, B1, B2, EPS, step + 1, vp(gn)))
        nf._lib.check(lib.nf_loglikelihood_step(ctx_a.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(ys), n, n, step, LR, B1, B2, EPS,
                                                None, None))
        torch.cuda.synchronize()
        assert torch.equal(th, th_b) and torch.equal(m, m_b) and torch.equal(v, v_b), f"step {step + 1}"
    ctx_a.close()
    ctx_b.close()
