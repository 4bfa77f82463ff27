"""GPU parity of the Hamiltonian flow's three kernels (nf_hamiltonian.hip: k_hf_apply, k_hf_bwd, k_hf_bwd_inv) and of the joint
branch of k_target, off the one-partial-wave geometry of tests/test_gpu_parity.py: several gradient slabs, the grid-stride
loop, full waves and a single sample, L = 1 and L = HF_MAXL, D = 1 and D = HF_MAXD, forty blocks, the tape pullback with a
per-sample log-det cotangent and its xbar, shards, in-library draws, and a gradient row beyond the default 64 KiB of LDS.

Reference: oracle/nf_oracle.py in float64 on the same inputs (hflow_fwd, hflow_inv, hflow_bwd, hflow_neg_elbo_value_and_grad,
hflow_nll_value_and_grad -- each pinned by finite differences in tests/test_oracle.py).  Every flow is
`hamiltonianflow(D, n, L, target)` at its default log eps0 = log 0.05 with theta perturbed by 0.1 * standard normal; the
Float32 runs round theta and every input through float32 first.  A larger step size is NOT a harder test: at log 0.2 with
D = 32, L = 16 the Banana oracle overflows and parity measures the chaos of the dynamics, not the kernels.

Tolerances are tests/parity.py's.  Float32 checks pass `floor=` the oracle evaluated in float32 on the same arrays.  Float64
checks use F64_RTOL (z, ladj, loss; element-wise with an absolute term in the proportion Y_ATOL / Y_RTOL of the float32
tolerance) and F64_GRAD (gradients, round trip); where one misses, the oracle is evaluated in np.longdouble on the same
inputs and the accepted error is max(stated, 3 x the float64 oracle's own distance from it) by the same measure, both
recorded.  Every check covers every sample and every parameter."""
import ctypes as C
import functools

import numpy as np
import pytest

import nf_oracle as o
import parity as P
from __graft_entry__ import load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
F64_ATOL = P.F64_RTOL * P.Y_ATOL / P.Y_RTOL

# id: (D, n, L, N)
SHAPES = {
    "maxD_maxL": (32, 2, 16, 200),    # every private array full; 4 workgroups, the last with 8 valid lanes; k_target joint at d = 64
    "L1": (32, 1, 1, 130),            # empty middle loops, V(L-1) = V(0); 3 workgroups
    "stride": (2, 3, 2, 2048 * 64 + 65),  # grid-stride: workgroups 0 and 1 take a second tile, workgroup 1's has one valid lane
    "deep": (5, 40, 3, 100),          # P = 620, 40 remembered block inputs per sample
    "full_N1": (3, 2, 2, 1),          # a single sample
    "full_N64": (3, 2, 2, 64),        # one full wave, no idle lane
    "full_N128": (3, 2, 2, 128),      # two full waves
    "D1": (1, 2, 3, 70),              # smallest joint (diagonal Gaussian only)
    "lds70k": (32, 90, 1, 70),        # gradient row of 8 768 doubles = 70 144 bytes: above the default 64 KiB of dynamic LDS
}
TARGETS = ("funnel", "banana", "diaggauss")
DTYPES = ("float64", "float32")
CASES = [(s, t, dt) for s in SHAPES if s not in ("D1", "lds70k") for t in TARGETS for dt in DTYPES] \
    + [("D1", "diaggauss", dt) for dt in DTYPES]
TAPE_CASES = [c for c in CASES if c[0] in ("maxD_maxL", "L1", "stride", "D1")]
MAXD_CASES = [c for c in CASES if c[0] == "maxD_maxL"]
STRIDE_CASES = [c for c in CASES if c[0] == "stride"]
LDS_CASE = ("lds70k", "diaggauss", "float64")


def _ids(cases):
    return ["-".join(c) for c in cases]


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


def cm(a, dt):
    return torch.tensor(np.ascontiguousarray(np.asarray(a).T), dtype=dt, device=DEV).t()


def _cast(dtype, *arrays):
    """copies in `dtype` (tuples, i.e. oracle targets, element by element)"""
    out = []
    for a in arrays:
        if isinstance(a, tuple):
            out.append(tuple(np.asarray(x, dtype=dtype) if isinstance(x, np.ndarray) else x for x in a))
        else:
            out.append(np.asarray(a, dtype=dtype))
    return out[0] if len(out) == 1 else out


class Case:
    """One (shape, target, dtype): the device flow, its inputs in float64 (float32-representable in the Float32 runs) and
    the oracle's results on them, each evaluated once per element type and shared by the tests."""

    def __init__(self, nf, shape, tname, dtn):
        self.shape, self.tname, self.dtn = shape, tname, dtn
        self.f32 = dtn == "float32"
        self.dt = torch.float32 if self.f32 else torch.float64
        self.tag = f"hf {shape} {tname} {'f32' if self.f32 else 'f64'}"
        D, n, L, N = self.geo = SHAPES[shape]
        rng = np.random.default_rng(11)
        r = (lambda a: a.astype(np.float32).astype(np.float64)) if self.f32 else (lambda a: a)
        if tname == "funnel":
            self.tgt, self.otgt = nf.FunnelTarget(D, -2.0, 3.0), ("funnel", -2.0, 3.0)
        elif tname == "banana":
            self.tgt, self.otgt = nf.BananaTarget(D, 1.0, 10.0), ("banana", 1.0, 10.0)
        else:
            mu, var = r(rng.standard_normal(D)), r(rng.uniform(size=D) + 0.5)
            self.tgt = nf.DiagGaussTarget(torch.tensor(mu, dtype=self.dt, device=DEV), torch.tensor(var, dtype=self.dt, device=DEV))
            self.otgt = ("diaggauss", mu, var)
        flow = nf.hamiltonianflow(D, n, L, self.tgt, paramtype=self.dt)
        assert flow.P == o.hflow_param_count(D, n)
        self.th = r(flow.theta.cpu().numpy().astype(np.float64) + 0.1 * rng.standard_normal(flow.P))
        self.flow = flow.with_theta(torch.tensor(self.th, dtype=self.dt, device=DEV))
        self.x0 = r(rng.standard_normal((2 * D, N)))
        self.us = r(0.7 * rng.standard_normal((2 * D, N)))
        self.ybar = r(rng.standard_normal((2 * D, N)) / N)
        self.lbar = r(rng.standard_normal(N) / N)
        self._memo = {}

    def oracle(self, what, dtype=np.float64):
        """what: fwd -> (z, ladj); inv -> (x, ladj_inv) of us; rt -> (x, ladj_inv) of the oracle's own z; elbo / nll -> (loss, grad);
        bwd -> (xbar, gtheta)"""
        key = (what, np.dtype(dtype).name)
        if key not in self._memo:
            D, n, L, _ = self.geo
            th, tg, x0, us, yb, lb = _cast(dtype, self.th, self.otgt, self.x0, self.us, self.ybar, self.lbar)
            if what == "fwd":
                v = o.hflow_fwd(D, n, L, th, tg, x0)
            elif what == "inv":
                v = o.hflow_inv(D, n, L, th, tg, us)
            elif what == "rt":
                v = o.hflow_inv(D, n, L, th, tg, self.oracle("fwd", dtype)[0])
            elif what == "elbo":
                v = o.hflow_neg_elbo_value_and_grad(D, n, L, th, tg, x0)
            elif what == "nll":
                v = o.hflow_nll_value_and_grad(D, n, L, th, tg, us)
            else:
                v = o.hflow_bwd(D, n, L, th, tg, x0, yb, lb)
            self._memo[key] = v
        return self._memo[key]


@functools.lru_cache(maxsize=None)
def _case(nf, shape, tname, dtn):
    return Case(nf, shape, tname, dtn)


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


# the four measures of tests/parity.py, in the widest type of their arguments (the longdouble comparison needs more than _np keeps)
def _m_elementwise(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def _m_gradient(got, ref):
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _m_norm(a, b):
    a, b = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(b, dtype=np.longdouble).ravel()
    den = max(np.sqrt((a * a).sum()), np.sqrt((b * b).sum()))
    return float(np.sqrt(((a - b) ** 2).sum()) / den)


def _m_scalar(got, ref):
    return float(abs(np.longdouble(got) - np.longdouble(ref)) / abs(np.longdouble(ref)))


def _f64_fallback(key, plain, err, dist, stated):
    """Float64: the stated tolerance, or -- where the check misses it -- max(stated, 3 x the float64 oracle's distance from the
    longdouble one) by the same measure (`dist()` evaluates the longdouble oracle only then); both figures are recorded."""
    try:
        plain()
    except AssertionError:
        d, e = dist(), err()
        P.record(key + " [float64 oracle vs longdouble oracle, same measure]", d)
        P.record(key + " [device vs float64 oracle, same measure]", e)
        assert e <= max(stated, P.CFLOOR * d), f"{key}: {e:.3e} > max({stated:.1e}, {P.CFLOOR} x {d:.3e})"


def check_elementwise(c, key, got, what, idx):
    ref = c.oracle(what)[idx]
    if c.f32:
        return P.elementwise(f"{c.tag}: {key}", got, ref, P.Y_RTOL, P.Y_ATOL, floor=c.oracle(what, np.float32)[idx])
    _f64_fallback(f"{c.tag}: {key}", lambda: P.elementwise(f"{c.tag}: {key}", got, ref, P.F64_RTOL, F64_ATOL),
                  lambda: _m_elementwise(_host(got), ref, P.F64_RTOL, F64_ATOL),
                  lambda: _m_elementwise(ref, c.oracle(what, np.longdouble)[idx], P.F64_RTOL, F64_ATOL), 1.0)


def check_gradient(c, key, got, what, idx, rtol64=P.F64_GRAD):
    ref = c.oracle(what)[idx]
    if c.f32:
        return P.gradient(f"{c.tag}: {key}", got, ref, P.GRAD_RTOL, floor=c.oracle(what, np.float32)[idx])
    _f64_fallback(f"{c.tag}: {key}", lambda: P.gradient(f"{c.tag}: {key}", got, ref, rtol64), lambda: _m_gradient(_host(got), ref),
                  lambda: _m_gradient(ref, c.oracle(what, np.longdouble)[idx]), rtol64)


def check_loss(c, key, got, what):
    ref = c.oracle(what)[0]
    if c.f32:
        # (the floor matters where one sample carries the mean: at `deep` the Funnel's inverse chain sends one of the 100 data
        # points to |x0| = 207, 231 of the loss of 272, and the float32 oracle itself is 1.0e-5 off)
        return P.scalar(f"{c.tag}: {key}", got, ref, P.LOSS_RTOL, floor=c.oracle(what, np.float32)[0])
    _f64_fallback(f"{c.tag}: {key}", lambda: P.scalar(f"{c.tag}: {key}", got, ref, P.F64_RTOL), lambda: _m_scalar(got, ref),
                  lambda: _m_scalar(ref, c.oracle(what, np.longdouble)[0]), P.F64_RTOL)


# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,tname,dtn", CASES, ids=_ids(CASES))
def test_forward(nf, shape, tname, dtn):
    """z and ladj of with_logabsdet_jacobian against hflow_fwd."""
    c = _case(nf, shape, tname, dtn)
    z, ladj = nf.with_logabsdet_jacobian(c.flow.transform, cm(c.x0, c.dt))
    assert z.shape == c.x0.shape and ladj.shape == (c.geo[3],)
    check_elementwise(c, "z", z, "fwd", 0)
    check_elementwise(c, "ladj", ladj, "fwd", 1)


@pytest.mark.parametrize("shape,tname,dtn", CASES, ids=_ids(CASES))
def test_inverse(nf, shape, tname, dtn):
    """The inverse chain on data `us` against hflow_inv (x and ladj_inv), and the round trip inverse(forward(x0)) = x0,
    norm-wise as the reference's own invertibility tests, with ladj_inv = -ladj."""
    c = _case(nf, shape, tname, dtn)
    inv = nf.inverse(c.flow.transform)
    x, li = nf.with_logabsdet_jacobian(inv, cm(c.us, c.dt))
    check_elementwise(c, "inverse x", x, "inv", 0)
    check_elementwise(c, "ladj_inv", li, "inv", 1)
    z, ladj = nf.with_logabsdet_jacobian(c.flow.transform, cm(c.x0, c.dt))
    xr, lr = nf.with_logabsdet_jacobian(inv, z)
    if c.f32:
        floor = P.relerr(c.oracle("rt", np.float32)[0], c.x0)
        P.isapprox(f"{c.tag}: round trip x", xr, c.x0, P.INV_RTOL["hamiltonian"], floor_err=floor)
    else:
        key = f"{c.tag}: round trip x"
        _f64_fallback(key, lambda: P.isapprox(key, xr, c.x0, P.F64_GRAD), lambda: _m_norm(_host(xr), c.x0),
                      lambda: _m_norm(c.oracle("rt")[0], c.oracle("rt", np.longdouble)[0]), P.F64_GRAD)
    # lj_bwd = -lj_fwd through the oracle's value, element-wise: the log-det is a sum of 4D + Dn terms log|scale| of either sign
    # that may cancel to anything (2.4e-3 from 220 terms of size 0.1 at `deep`), so only an absolute bound says something
    check_elementwise(c, "round trip ladj_inv", lr, "rt", 1)
    check_elementwise(c, "round trip ladj", ladj, "fwd", 1)


@pytest.mark.parametrize("shape,tname,dtn", CASES, ids=_ids(CASES))
def test_layers_chain_to_the_whole_map(nf, shape, tname, dtn):
    """nf.layer(flow, l) for l = n (the reference map), n-1, ..., 0 chained equals the whole forward -- z bit for bit (the same
    arithmetic on the same values), ladj to the tolerance (the partial log-dets are added in another order) -- and the
    inverse layers in the opposite order equal the whole inverse."""
    c = _case(nf, shape, tname, dtn)
    n = c.geo[1]
    x_t = cm(c.x0, c.dt)
    z, ladj = nf.with_logabsdet_jacobian(c.flow.transform, x_t)
    w, lsum = x_t, torch.zeros_like(ladj)
    for l in range(n, -1, -1):
        w, ll = nf.with_logabsdet_jacobian(nf.layer(c.flow, l), w)
        lsum = lsum + ll
    assert torch.equal(w, z), "layer by layer, the forward differs from the whole map"
    check_elementwise(c, "ladj, layer by layer", lsum, "fwd", 1)
    u_t = cm(c.us, c.dt)
    x, li = nf.with_logabsdet_jacobian(nf.inverse(c.flow.transform), u_t)
    w, lsum = u_t, torch.zeros_like(li)
    for l in range(0, n + 1):
        w, ll = nf.with_logabsdet_jacobian(nf.inverse(nf.layer(c.flow, l)), w)
        lsum = lsum + ll
    assert torch.equal(w, x), "layer by layer, the inverse differs from the whole map"
    check_elementwise(c, "ladj_inv, layer by layer", lsum, "inv", 1)


def _elbo(nf, c):
    return nf.value_and_gradient(nf.elbo_batch, c.flow, c.tgt, cm(c.x0, c.dt))


def _fkl(nf, c):
    return nf.loglikelihood_value_and_gradient(c.flow, cm(c.us, c.dt))


def check_elbo_and_fkl(nf, c):
    loss, g = _elbo(nf, c)
    check_loss(c, "elbo loss", loss, "elbo")
    check_gradient(c, "elbo grad", g, "elbo", 1)
    loss, g = _fkl(nf, c)
    check_loss(c, "fkl loss", loss, "nll")
    check_gradient(c, "fkl grad", g, "nll", 1)


@pytest.mark.parametrize("shape,tname,dtn", CASES, ids=_ids(CASES))
def test_elbo_loss_and_gradient(nf, shape, tname, dtn):
    """value_and_gradient(elbo_batch) on supplied draws against hflow_neg_elbo_value_and_grad: k_hf_apply, k_target's joint
    branch, k_hf_bwd with the constant log-det cotangent, the slab reduction."""
    c = _case(nf, shape, tname, dtn)
    loss, g = _elbo(nf, c)
    check_loss(c, "elbo loss", loss, "elbo")
    check_gradient(c, "elbo grad", g, "elbo", 1)


@pytest.mark.parametrize("shape,tname,dtn", CASES, ids=_ids(CASES))
def test_forward_kl_loss_and_gradient(nf, shape, tname, dtn):
    """loglikelihood_value_and_gradient on data `us` against hflow_nll_value_and_grad: k_hf_bwd_inv."""
    c = _case(nf, shape, tname, dtn)
    loss, g = _fkl(nf, c)
    check_loss(c, "fkl loss", loss, "nll")
    check_gradient(c, "fkl grad", g, "nll", 1)


def flow_bwd_from_x(nf, flow, x_t, y, yb_t, lb_t):
    """nf_flow_bwd through the C ABI: (xbar, gtheta) from x alone"""
    lib, ctx = nf.load_library(), flow.ctx
    d, n = x_t.shape
    xb = nf.new_batch(d, n, x_t.dtype, DEV)
    g = torch.empty(flow.P, dtype=x_t.dtype, device=DEV)
    nf._lib.check(lib.nf_flow_bwd(ctx.ptr, C.byref(flow.desc), flow.theta.data_ptr(), x_t.data_ptr(), y.data_ptr(), yb_t.data_ptr(),
                                  lb_t.data_ptr(), n, xb.data_ptr(), g.data_ptr()))
    return xb, g


@pytest.mark.parametrize("shape,tname,dtn", TAPE_CASES, ids=_ids(TAPE_CASES))
def test_tape_pullback(nf, shape, tname, dtn):
    """rrule(with_logabsdet_jacobian) for a random output cotangent and a random PER-SAMPLE log-det cotangent: the forward
    values are the plain forward's, (xbar, gtheta) match hflow_bwd, a second pullback returns the same bits, and nf_flow_bwd
    (from x alone) returns the same two arrays."""
    c = _case(nf, shape, tname, dtn)
    x_t, yb_t = cm(c.x0, c.dt), cm(c.ybar, c.dt)
    lb_t = torch.tensor(c.lbar, dtype=c.dt, device=DEV)
    (y, ladj), pullback = nf.flows.rrule_with_logabsdet_jacobian(c.flow.transform, x_t)
    y0, l0 = nf.with_logabsdet_jacobian(c.flow.transform, x_t)
    assert torch.equal(y, y0) and torch.equal(ladj, l0), "keep-forward and plain forward disagree"
    xbar, g = pullback(yb_t, lb_t)
    check_gradient(c, "pullback gtheta", g, "bwd", 1)
    check_gradient(c, "pullback xbar", xbar, "bwd", 0)
    xbar2, g2 = pullback(yb_t, lb_t)
    assert torch.equal(g, g2) and torch.equal(xbar, xbar2), "second pullback differs: the tape was modified"
    assert torch.equal(yb_t, cm(c.ybar, c.dt)), "the pullback wrote into the caller's cotangent"
    xb3, g3 = flow_bwd_from_x(nf, c.flow, x_t, y, yb_t, lb_t)
    check_gradient(c, "nf_flow_bwd gtheta", g3, "bwd", 1)
    check_gradient(c, "nf_flow_bwd xbar", xb3, "bwd", 0)
    assert torch.equal(g3, g) and torch.equal(xb3, xbar), "nf_flow_bwd and the tape pullback disagree"


@pytest.mark.parametrize("shape,tname,dtn", MAXD_CASES, ids=_ids(MAXD_CASES))
def test_shards_add_up_to_the_full_batch(nf, shape, tname, dtn):
    """Shards of 137 and 63 of the 200 samples, each with n_global = 200: the two ELBO gradients and the two forward-KL
    gradients (and losses) add up to the full batch's."""
    c = _case(nf, shape, tname, dtn)
    N = c.geo[3]
    cut = 137
    tol = P.GRAD_RTOL if c.f32 else 1e-12
    for name, arr, full, part in (
            ("elbo", c.x0, _elbo, lambda a: nf.value_and_gradient(nf.elbo_batch, c.flow, c.tgt, cm(a, c.dt), n_global=N)),
            ("fkl", c.us, _fkl, lambda a: nf.loglikelihood_value_and_gradient(c.flow, cm(a, c.dt), n_global=N))):
        lf, gf = full(nf, c)
        la, ga = part(arr[:, :cut])
        lb, gb = part(arr[:, cut:])
        P.gradient(f"{c.tag}: {name} grad, shards 137 + 63 vs whole", ga.double() + gb.double(), gf.double(), tol)
        P.scalar(f"{c.tag}: {name} loss, shards 137 + 63 vs whole", la + lb, lf, P.LOSS_RTOL if c.f32 else 1e-12)


@pytest.mark.parametrize("shape,tname,dtn", MAXD_CASES, ids=_ids(MAXD_CASES))
def test_draws_made_in_the_library(nf, shape, tname, dtn):
    """The rng form of the ELBO value and gradient equals the supplied-draw form on the draws the base sampler returns for
    the same seed and stream: the same draws go through the same kernels, so the gradient has the same bits (the base
    log-density is summed by another kernel: the loss to rounding)."""
    c = _case(nf, shape, tname, dtn)
    N = c.geo[3]
    l1, g1 = nf.value_and_gradient(nf.elbo_batch, c.flow, c.tgt, N, rng=nf.PhiloxRNG(9))
    xs = nf.device_specific_rand(nf.PhiloxRNG(9), c.flow.dist, N, dtype=c.dt)
    assert xs.shape == (2 * c.geo[0], N)
    l2, g2 = nf.value_and_gradient(nf.elbo_batch, c.flow, c.tgt, xs)
    assert torch.equal(g1, g2)
    assert l1 == pytest.approx(l2, rel=1e-6 if c.f32 else 1e-13)
    v1 = nf.elbo_batch(nf.PhiloxRNG(9), c.flow, c.tgt, N)
    assert -v1 == pytest.approx(l2, rel=1e-6 if c.f32 else 1e-13)


@pytest.mark.parametrize("shape,tname,dtn", STRIDE_CASES, ids=_ids(STRIDE_CASES))
def test_second_call_returns_the_same_bits(nf, shape, tname, dtn):
    """No atomics in the reverse kernels: with 2 048 slabs and two tiles per workgroup the ELBO and forward-KL values and
    gradients come back bit for bit."""
    c = _case(nf, shape, tname, dtn)
    for f in (_elbo, _fkl):
        l1, g1 = f(nf, c)
        l2, g2 = f(nf, c)
        assert l1 == l2 and torch.equal(g1, g2)


def test_gradient_row_beyond_64k_of_lds(nf):
    """D = 32, n = 90, L = 1, N = 70 in Float64: the LDS gradient row of the reverse kernels is 70 144 bytes, which needs the
    launch paths' opt-in (hipFuncAttributeMaxDynamicSharedMemorySize).  ELBO and forward-KL loss and gradient."""
    c = _case(nf, *LDS_CASE)
    assert o.hflow_param_count(*c.geo[:2]) * 8 == 70144
    check_elbo_and_fkl(nf, c)
