"""The five built-in targets (DiagGauss, Banana, Funnel, WarpedGauss, Cross) away from the N(0, 1) cloud, at every evaluation site.

A plain module (no pytest, no torch at import), importable from a child process: tests/test_target_cases_cpu.py holds the cases
to the conditions that keep a parity check meaningful, tests/test_gpu_target_regimes.py runs them on the device -- in process,
and once per environment switch in a child process.

A case is (target, parameter set, d, cloud, n).  A cloud is centre + scale * N(0, 1) per coordinate with a fixed seed, N = 77
columns, rounded to float32 first: the float64 reference, the float32 oracle and the device all see the same numbers.  n in
NS = (1, 33, 77) takes the first n columns (lane 0 alone, one sample past a 32-sample tile, a ragged third tile); the target's
scalar parameters are rounded to float32 as well (the Float32 kernels receive them as doubles and cast).

  Funnel      (mu, sigma) in (0.3, 2), (0, 3), (-1, 0.5); y0 centred at -12, -8, -4, 0, 4, 8, 20 with scale 0.5 (exp(-y0) from 2e-9
              to 1.6e5; the a s2 / 2 - (d - 1) / 2 balance of the score of y0), the other coordinates at scale 0.05, 1, 5
  Banana      (b, var) in (1, 100), (0.3, 4), (3, 0.25), (0.02, 1); y0 as (centre, scale) in (0, 1), (0, 10), (5, 0.3), (-20, 1)
              (b y0^2 up to a few hundred), y1 centred at 0, +30, -30 with scale 1, the rest N(0, 1)
  Cross       (mu, sigma) in (2, 0.15), (5, 0.02), (0.5, 1); on an arm ((0, mu); 0.1), on a side arm ((mu, 1); 0.1), between arms
              ((1, 1.5); 0.05), far out ((30, 30); 1: three components underflow), ((-8, 3); 2), the origin at scale 1e-3
  WarpedGauss (sigma1, sigma2) in (1, 0.12), (0.12, 1), (2, 2); the origin at scale 1, 1e-3 and 1e-6 (log r, dr / r), ((1, 0); 0.1),
              ((-1, 0); 0.05), ((6, 6); 1), ((40, -30); 3), ((-3, 1e-4); 0.5): the branch cut of atan2
  DiagGauss   two draws of (mu uniform in +-50, var log-uniform over 1e-4 ... 1e4) per d; the cloud mu + 3 sqrt(var) N(0, 1) and
              plain N(0, 1), far in the tails of the narrow coordinates

Dimensions (Funnel, Banana, DiagGauss; WarpedGauss and Cross are d = 2).  DIMS holds 2 and 3 (s2 is one term, no feature i >= 2 /
exactly one) and the smallest d on each side of every boundary of the eight sites, read off the dispatch code:
  7 | 8      radial_lane_ok (nf_simple.hip): Float32 radial flows of 8 <= d <= 64 run k_radial_step, below it k_simple_step
  8 | 9      FS = 8 feature slices of k_target_tiled (nf_elementwise.hip): from d = 9 a slice owns a second feature
  16 | 17    LPS = 16 lanes per sample of k_target (a lane's second feature) and of nf_simple.hip (dpl_for: DPL 1 | 2)
  32 | 33    DPL 2 | 4; the tile kernels' DB = 1 | 2 feature blocks (tile_step: d > 32)
  64 | 65    DPL 4 | 8; planar_mfma_ok / radial_lane_ok end at 64: k_planar_step / k_radial_step | k_simple_step
  128 | 129  DPL 8 | 16; in Float64 DPL 16 leaves a register budget of 32 / 16 = 2 layers, below step_nlmax's smallest bound: the
             split sequence simple_apply (fused target, stashing) + simple_bwd, i.e. site 3 with a gradient
3, 7, 9, 17, 33, 65 and 129 are odd (element-wise rows: vec_ok needs d % vw == 0).

How a cloud is held (the rules are computed from the two oracles alone, never from device output; TOL = 1e-6 + 1e-5 |ref|):
  an element is CONDITIONED when the float32 oracle's error on it is <= 0.25 TOL;
  a cloud is PLAIN when >= 95 % of its log-p elements and >= 95 % of its score elements are conditioned: the device is held to
  TOL (Float64: 1e-12 + F64_RTOL |ref|) with no floor on the conditioned elements, and by the gradient measure
  max |err| / |ref|inf <= GRAD_RTOL (F64_GRAD) on the whole array;
  every other cloud is NORM-WISE ONLY: the gradient measure alone, and the float32 oracle's own figure must be <= 0.1 GRAD_RTOL.
For n < 77 the gradient measure keeps the whole cloud's |ref|inf: the errors of a prefix are a subset of the whole array's.
Aggregate checks (loss, parameter gradient: parity.scalar / parity.gradient with the float32 oracle as floor) run only where the
float32 oracle's own error is <= 0.1 x the respective rtol and |loss| >= 0.1 mean |per-sample ELBO term|.

Flows of sites 2-6 (flow_theta): the family's near-identity with small non-zero parameters, so that y ~ x = the cloud and every
parameter gradient is non-trivial; the oracle evaluates the same flow, nothing depends on y = x exactly.
In-library draws (sites 7, 8): a RealNVP flow whose output-layer weights are zero and whose output biases are prescribed maps
x -> x exp(tanh b_s) + b_t on each half, per coupling; with L = 4 blocks (eight couplings, four per half) a coordinate's scale
reaches exp(+-4 x 0.9) = 0.027 ... 36 and any centre.  Reachable: every Funnel and Banana cloud, the Cross and WarpedGauss
clouds of scale >= 0.05, DiagGauss' N(0, 1) cloud and its own cloud where 3 sqrt(var) is clipped to that range (placed_theta).  Not
reachable: the scale-1e-3 and 1e-6 clouds (the origin of Cross and WarpedGauss).  NSF: with zero output weights every sample
gets the same spline, which maps [-B, B] onto itself monotonically -- it can bend the N(0, 1) draws inside the box but not carry
them to -12 or +30 at scale 0.5, so NSF runs at what biases of scale NSF_BIAS reach (|y| up to a few units); the far clouds are
not reachable there and are covered at sites 1-7.
How an ELBO term, whose log q0(x) cancels log p(y) on the far clouds, is held: term_scale -- a narrowing of the rules above for
ELBO terms and losses.  Per-sample checks reach sites 1 and 2 only; sites 3-8 return nothing per sample and are held by loss and
gradient (flow_site, placed_site).
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
if _ORACLE not in sys.path:
    sys.path.insert(0, _ORACLE)
import nf_oracle as o  # noqa: E402
import fullrank_ref as fr  # noqa: E402
from affine_cases import Checks, _cm  # noqa: E402,F401

Y_RTOL, Y_ATOL, LOSS_RTOL, GRAD_RTOL, F64_RTOL, F64_GRAD, F64_ATOL = 1e-5, 1e-6, 1e-5, 1e-4, 1e-10, 1e-9, 1e-12  # tests/parity.py's
COND, PLAIN_SHARE, FLOOR_SHARE = 0.25, 0.95, 0.1
N, NS = 77, (1, 33, 77)
TARGETS = ("funnel", "banana", "cross", "warped", "diaggauss")
D2 = ("cross", "warped")
PARAMS = {
    "funnel": ((0.3, 2.0), (0.0, 3.0), (-1.0, 0.5)),
    "banana": ((1.0, 100.0), (0.3, 4.0), (3.0, 0.25), (0.02, 1.0)),
    "cross": ((2.0, 0.15), (5.0, 0.02), (0.5, 1.0)),
    "warped": ((1.0, 0.12), (0.12, 1.0), (2.0, 2.0)),
    "diaggauss": (0, 1),  # draws of (mu, var)
}
DIMS = (2, 3, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)
TERM_ULPS = int(np.ceil(np.log2(max(DIMS))))  # 8: see term_scale
FD_DIMS = (2, 3, 9)  # where the oracle's scores are checked against finite differences of its log p

Cloud = namedtuple("Cloud", "name centre scale")


def _f32r(a):
    """float64 array of float32-representable values"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def dims_of(target):
    return (2,) if target in D2 else DIMS


def params(target, pi):
    """the parameter set as the oracle's tuple tail, rounded to float32"""
    return tuple(float(np.float32(v)) for v in PARAMS[target][pi])


@functools.lru_cache(maxsize=None)
def diag_params(pi, d):
    rng = np.random.default_rng([11, PARAMS["diaggauss"][pi], d])
    mu, var = _f32r(rng.uniform(-50.0, 50.0, d)), _f32r(10.0 ** rng.uniform(-4.0, 4.0, d))
    mu.setflags(write=False)
    var.setflags(write=False)
    return mu, var


def otarget(target, pi, d, dt=np.float64):
    """the oracle's target tuple in dtype dt"""
    if target == "diaggauss":
        mu, var = diag_params(pi, d)
        return ("diaggauss", mu.astype(dt), var.astype(dt))
    return (target,) + tuple(dt(v) for v in params(target, pi))


def _vec(d, first, rest):
    v = np.full(d, float(rest))
    v[:len(first)] = first
    return v


@functools.lru_cache(maxsize=None)
def clouds(target, pi, d):
    out = []
    if target == "funnel":
        for c0 in (-12.0, -8.0, -4.0, 0.0, 4.0, 8.0, 20.0):
            for s in (0.05, 1.0, 5.0):
                out.append(Cloud(f"y0@{c0:g} rest x{s:g}", _vec(d, (c0,), 0.0), _vec(d, (0.5,), s)))
    elif target == "banana":
        for c0, s0 in ((0.0, 1.0), (0.0, 10.0), (5.0, 0.3), (-20.0, 1.0)):
            for c1 in (0.0, 30.0, -30.0):
                out.append(Cloud(f"y0@{c0:g}x{s0:g} y1@{c1:g}", _vec(d, (c0, c1), 0.0), _vec(d, (s0,), 1.0)))
    elif target == "cross":
        mu = params(target, pi)[0]
        for name, c, s in (("arm", (0.0, mu), 0.1), ("side arm", (mu, 1.0), 0.1), ("between arms", (1.0, 1.5), 0.05), ("(30,30)", (30.0, 30.0), 1.0),
                           ("(-8,3)", (-8.0, 3.0), 2.0), ("origin x1e-3", (0.0, 0.0), 1e-3)):
            out.append(Cloud(name, np.array(c), np.full(2, s)))
    elif target == "warped":
        for name, c, s in (("origin x1", (0.0, 0.0), 1.0), ("origin x1e-3", (0.0, 0.0), 1e-3), ("origin x1e-6", (0.0, 0.0), 1e-6), ("(1,0)", (1.0, 0.0), 0.1),
                           ("(-1,0)", (-1.0, 0.0), 0.05), ("(6,6)", (6.0, 6.0), 1.0), ("(40,-30)", (40.0, -30.0), 3.0), ("branch cut", (-3.0, 1e-4), 0.5)):
            out.append(Cloud(name, np.array(c), np.full(2, s)))
    else:
        mu, var = diag_params(pi, d)
        out.append(Cloud("own 3 sigma", mu.copy(), 3.0 * np.sqrt(var)))
        out.append(Cloud("N(0,1)", np.zeros(d), np.ones(d)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def points(target, pi, d, ci):
    """the cloud's (d, N) points, float32-representable"""
    c = clouds(target, pi, d)[ci]
    rng = np.random.default_rng([23, TARGETS.index(target), pi, d, ci, 0])
    y = _f32r(c.centre[:, None] + c.scale[:, None] * rng.standard_normal((d, N)))
    y.setflags(write=False)
    return y


def all_clouds(target, dims=None):
    return [(pi, d, ci) for pi in range(len(PARAMS[target])) for d in (dims or dims_of(target)) for ci in range(len(clouds(target, pi, d)))]


def n_of(pi, ci):
    """the batch size a flow case takes of cloud ci (site 1 runs all of NS)"""
    return NS[(ci + ci // 3 + pi) % 3]


def tol32(ref):
    return Y_ATOL + Y_RTOL * np.abs(ref)


Ref = namedtuple("Ref", "lp64 g64 lp32 g32 cond_lp cond_g plain floor_lp floor_g")


def classify(r64, r32):
    """(conditioned mask, share conditioned, float32 oracle's max |err| / |ref|inf)"""
    err = np.abs(r32.astype(np.float64) - r64)
    cond = err <= COND * tol32(r64)
    return cond, float(cond.mean()), float(err.max() / max(np.abs(r64).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def reference(target, pi, d, ci):
    y = points(target, pi, d, ci)
    with np.errstate(all="ignore"):
        t64, t32 = otarget(target, pi, d), otarget(target, pi, d, np.float32)
        lp64, g64 = o.target_logp(t64, y), o.target_grad(t64, y)
        y32 = y.astype(np.float32)
        lp32, g32 = o.target_logp(t32, y32), o.target_grad(t32, y32)
    cl, sl, fl = classify(lp64, lp32)
    cg, sg, fg = classify(g64, g32)
    return Ref(lp64, g64, lp32, g32, cl, cg, sl >= PLAIN_SHARE and sg >= PLAIN_SHARE, fl, fg)


# ----------------------------------------------------------------------------------------------------------------------
# holding a device array to the rules above
# ----------------------------------------------------------------------------------------------------------------------
def _rec(P, key, value):
    """the parity table keeps the WORST figure of a group (site, dtype, target, d): one row per group, not one per cloud"""
    P.MEASURED[key] = max(P.MEASURED.get(key, 0.0), float(value))


def hold(chk, group, detail, got, r64, r32, f64, plain=None, cond=None, scale=None, terms=None):
    """got against r64 under the module docstring's rules; r32 is the float32 oracle on the same inputs.  `plain` / `cond` / `scale`
    (the whole cloud's |ref|inf) are passed where they were decided on more than this array.  `terms`: see term_scale.  Figures are
    recorded under `group` (worst of the group), failures name `detail` too.  Returns the device's worst ratio."""
    P = chk.P
    key = f"{group} ({detail})"
    got = got.detach().cpu().numpy().astype(np.float64) if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    assert got.shape == r64.shape, (key, got.shape, r64.shape)
    ferr = np.abs(np.asarray(r32, dtype=np.float64) - r64)
    if cond is None:
        cond = ferr <= COND * tol32(r64)
        if terms is not None:
            cond &= TERM_ULPS * 2.0 ** -24 * np.abs(terms) <= tol32(r64)
    if plain is None:
        plain = cond.mean() >= PLAIN_SHARE
    if scale is None:
        scale = max(float(np.abs(r64).max()), 1e-300)
    floor = float(ferr.max() / scale)
    how = "max abs err / |ref|inf"
    if terms is not None and floor > FLOOR_SHARE * GRAD_RTOL:
        scale = max(float(np.abs(terms).max()), 1e-300)
        floor = float(ferr.max() / scale)
        how = "max abs err / largest term"
    err = np.abs(got - r64)
    if not np.isfinite(got).all():
        chk.failed.append(f"{key}: the device returned a non-finite value")
        return float("inf")
    worst = 0.0
    if plain and cond.any():
        tol = (F64_ATOL + F64_RTOL * np.abs(r64)) if f64 else tol32(r64)
        worst = float((err / tol)[cond].max())
        _rec(P, group + " [conditioned elements: err / (atol + rtol|ref|)]", worst)
        if not f64:
            _rec(P, group + " [conditioned elements: fp32-oracle floor / (atol + rtol|ref|)]", float((ferr / tol)[cond].max()))
        if worst > 1.0:
            chk.failed.append(f"{key}: a conditioned element is {worst:.2f}x the plain tolerance (float32 oracle: {float((ferr / tol32(r64))[cond].max()):.2f}x)")
    gm = float(err.max() / scale)
    _rec(P, group + f" [{how}]", gm)
    _rec(P, group + f" [fp32-oracle floor, {how}]", floor)
    if floor <= FLOOR_SHARE * GRAD_RTOL:
        if gm > (F64_GRAD if f64 else GRAD_RTOL):
            chk.failed.append(f"{key}: {how} = {gm:.3e} (float32 oracle: {floor:.3e})")
    else:  # plain or not: the gradient measure is asserted on every array, so an array it cannot be asserted on fails its case
        chk.failed.append(f"{key}: not norm-wise conditioned (float32 oracle {floor:.3e}, {how}): a defect of the case")
    return worst


def aggregate(chk, fn, group, detail, *args, **kw):
    """parity.scalar / parity.gradient under `group`, keeping the group's worst figures; a failure names `detail`"""
    P = chk.P
    before = {k: v for k, v in P.MEASURED.items() if k.startswith(group + " [")}
    try:
        getattr(P, fn)(group, *args, **kw)
    except AssertionError as e:
        chk.failed.append(f"({detail}) {e}")
    for k, v in before.items():
        P.MEASURED[k] = max(P.MEASURED[k], v)


def device_target(nf, torch, target, pi, d, dt):
    if target == "diaggauss":
        mu, var = diag_params(pi, d)
        return nf.DiagGaussTarget(torch.tensor(mu, dtype=dt, device="cuda"), torch.tensor(var, dtype=dt, device="cuda"))
    a, b = params(target, pi)
    return {"funnel": lambda: nf.FunnelTarget(d, a, b), "banana": lambda: nf.BananaTarget(d, a, b), "cross": lambda: nf.CrossTarget(a, b),
            "warped": lambda: nf.WarpedGaussTarget(a, b)}[target]()


PROF_NAMES = ("target", "layout_convert", "affine_chain", "affine_chain_tgt", "rqs_chain", "rqs_chain_tgt", "affine_apply", "simple_apply", "simple_bwd",
              "simple_step", "planar_step", "radial_step", "fr_apply_flat", "fr_grad_flat", "fr_gemm", "g64_apply")


def launched(nf, ctx, run):
    """{profiler name: launches} of PROF_NAMES while `run()` executes"""
    import ctypes as C

    import torch

    lib = nf.load_library()
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
    try:
        run()
        torch.cuda.synchronize()
        ran = {}
        for name in PROF_NAMES:
            a, k = C.c_double(0.0), C.c_int64(0)
            lib.nf_prof_read(ctx.ptr, name.encode(), C.byref(a), C.byref(k))
            ran[name] = int(k.value)
    finally:
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
    return ran


def only(ran, **want):
    """the launches named in `want` ran that often (True: at least once) and no other target-evaluating launch ran at all"""
    evaluators = ("target", "affine_chain_tgt", "rqs_chain_tgt", "simple_apply", "simple_step", "planar_step", "radial_step")
    for name, k in want.items():
        if (ran[name] < 1) if k is True else (ran[name] != k):
            return False
    return not any(ran[name] for name in evaluators if name not in want)


def site1(nf, target, pi, d, f64, chk=None, ns=NS):
    """k_target<float / double>: nf.target_logp with its gradient on every cloud of (target, parameter set, d), every n of `ns`"""
    import torch

    chk = chk or Checks()
    dt = torch.float64 if f64 else torch.float32
    tgt = device_target(nf, torch, target, pi, d, dt)
    for ci, c in enumerate(clouds(target, pi, d)):
        R, y = reference(target, pi, d, ci), points(target, pi, d, ci)
        sl, sg = max(float(np.abs(R.lp64).max()), 1e-300), max(float(np.abs(R.g64).max()), 1e-300)
        for n in ns:
            group = f"target regimes: site 1 {'f64' if f64 else 'f32'} {target} d={d}: "
            detail = f"{params(target, pi) if target != 'diaggauss' else 'draw ' + str(pi)} {c.name} n={n}"
            lp, g = nf.target_logp(tgt, _cm(torch, y[:, :n], dt), with_grad=True)
            hold(chk, group + "log p", detail, lp, R.lp64[:n], R.lp32[:n], f64, R.plain, R.cond_lp[:n], sl)
            hold(chk, group + "score", detail, g, R.g64[:, :n], R.g32[:, :n], f64, R.plain, R.cond_g[:, :n], sg)
    return chk


# ----------------------------------------------------------------------------------------------------------------------
# sites 2-6: supplied draws xs = the cloud through a near-identity flow
# ----------------------------------------------------------------------------------------------------------------------
FLOW_KINDS = ("realnvp", "fullrank", "meanfield", "planar", "radial")
HDIMS, SIMPLE_NL = (32, 32), 2


def dpl_for(d):
    need, dpl = (d + 15) // 16, 1
    while dpl < need:
        dpl *= 2
    return dpl


def train_launch(kind, f64, d, nl=None, no_tile=False):
    """profiler name of the launch that evaluates the target in nf_elbo_value_and_grad with supplied draws (the module docstring's
    reading of nf_simple.hip and nf_api.hip); "split" = simple_apply + simple_bwd.  no_tile: under NF_PLANAR_NO_MFMA / NF_RADIAL_NO_LANE"""
    if kind in ("realnvp", "fullrank"):
        return "target"
    nl = nl or SIMPLE_NL
    if kind == "planar" and not f64 and 2 <= d <= 64 and nl <= 16 and not no_tile:
        return "planar_step"
    if kind == "radial" and not f64 and 8 <= d <= 64 and nl <= 16 and not no_tile:
        return "radial_step"
    if kind == "meanfield":
        return "simple_step"
    budget = (32 if f64 else 64) // dpl_for(d)  # step_nlmax
    return "simple_step" if nl <= (12 if budget >= 12 else 10 if budget >= 10 else 4 if budget >= 4 else 0) else "split"


# (kind, Float64, layers, dims): every d of DIMS where the site's own code changes with d, a few elsewhere.
# nf.batched_elbos of a simple flow runs k_simple_apply WITHOUT the fused target and then k_target (site 1 once more, behind a flow);
# the fused target of k_simple_apply (site 3) runs in the training forward of flows beyond k_simple_step's register budget: the
# split sequence simple_apply + simple_bwd.  With SIMPLE_NL = 2 layers that is Float64 at DPL 16 only, so the rows with 5 and 13
# layers put every other DPL there (step_nlmax: 12 layers at DPL 1 and 2 in Float64, 4 at DPL 4 and 8, 4 at DPL 8 and 16 in Float32);
# a mean-field flow has two layers and never splits.
FLOW_CASES = (
    ("realnvp", False, None, (2, 3, 8, 9, 32, 33, 64)),    # site 2 (k_target_tiled: FS = 8 slices), LDS-resident NetGeo RealNVP
    ("fullrank", False, None, (2, 3, 9, 32, 33, 65)),    # site 2 behind the tiled full-rank family
    ("meanfield", False, None, DIMS), ("planar", False, 2, DIMS), ("radial", False, 2, DIMS),   # sites 4 (d > 64; radial d < 8; mean-field), 5, 6
    ("meanfield", True, None, (2, 3, 17, 33, 65, 129)), ("planar", True, 2, (2, 3, 17, 33, 65, 129)), ("radial", True, 2, (2, 3, 17, 33, 65, 129)),  # site 4; 129: 3
    ("planar", False, 5, (65, 128, 129)), ("radial", False, 5, (65, 129)),      # site 3, Float32 DPL 8 and 16
    ("planar", True, 5, (33, 64, 65)), ("radial", True, 5, (33, 65)),           # site 3, Float64 DPL 4 and 8
    ("planar", True, 13, (2, 3, 17)), ("radial", True, 13, (2, 16, 17)),        # site 3, Float64 DPL 1 and 2
    ("radial", False, 13, (2, 3)), ("planar", False, 17, (2,)),                 # site 3, Float32 DPL 1 (d = 2: Cross and WarpedGauss): radial below
    #                                                                             the lane kernel's d = 8, planar beyond the tile kernel's 16 layers
)
SWITCH_ROWS = {"NF_PLANAR_NO_MFMA": ("planar", (2, 3, 17, 33, 64)), "NF_RADIAL_NO_LANE": ("radial", (8, 17, 33, 64))}  # site 4's two switch arms


def flow_spec(kind, d, nl=None):
    if kind == "realnvp":
        return o.FlowSpec("realnvp", d, 1, HDIMS)
    if kind == "meanfield":
        return o.FlowSpec("meanfield", d, 1)
    return o.FlowSpec(kind, d, nl or SIMPLE_NL)


@functools.lru_cache(maxsize=None)
def flow_theta(kind, d, nl=None):
    nl = nl or SIMPLE_NL
    rng = np.random.default_rng([31, FLOW_KINDS.index(kind), d, nl])
    if kind == "meanfield":
        th = np.concatenate([0.01 * rng.standard_normal(d), 1.0 + 0.01 * rng.standard_normal(d)])
    elif kind == "fullrank":
        th = fr.join(0.01 * rng.standard_normal(d), np.eye(d) + 0.01 * np.tril(rng.standard_normal((d, d))))
    elif kind == "planar":
        # |w| = 1: u_hat = u + (softplus(w'u) - 1 - w'u) w / |w|^2, and with a small w that correction is 0.3 / |w| -- at |w| = 0.03 the
        # "near-identity" carried y0 from -11.4 to -7.4 and cancelled u against it; at |w| = 1 it is 0.3 along w, y within 0.4 of x
        def layer(k):
            w = rng.standard_normal(d)
            return np.concatenate([w / np.linalg.norm(w), 0.05 * rng.standard_normal(d) / np.sqrt(d), [0.1 * (-1) ** k]])

        th = np.concatenate([layer(k) for k in range(nl)])
    elif kind == "radial":
        alpha = np.log(2.0)  # softplus(0)
        th = np.concatenate([np.concatenate([[0.0, np.log(np.expm1(alpha + 0.02 * (k + 1)))], 0.1 * rng.standard_normal(d)]) for k in range(nl)])
    else:
        th = 0.05 * o.init_params(flow_spec(kind, d), rng)
        th = np.where(th == 0.0, 0.01 * rng.standard_normal(th.shape), th)  # the biases
    th = _f32r(th)
    th.setflags(write=False)
    return th


def flow_oracle(kind, d, ot, xs, dt, nl=None):
    """per-sample ELBO terms, loss and parameter gradient of the near-identity flow in dtype dt"""
    th, xs = flow_theta(kind, d, nl).astype(dt), xs.astype(dt)
    ot = tuple(v.astype(dt) if isinstance(v, np.ndarray) else (dt(v) if not isinstance(v, str) else v) for v in ot)
    with np.errstate(all="ignore"):
        if kind == "fullrank":
            tf = lambda y: (o.target_logp(ot, y), o.target_grad(ot, y))  # noqa: E731
            e = fr.elbos(th, xs, tf)
            loss, g = fr.neg_elbo_value_and_grad(th, xs, tf)
        else:
            spec = flow_spec(kind, d, nl)
            e = o.batched_elbos(spec, th, ot, xs)
            loss, g = o.neg_elbo_value_and_grad(spec, th, ot, xs)
    return e, float(loss), g


def term_scale(e64, xs):
    """|log p(y) + ladj| + |log q0(x)| per sample, the magnitude of what an ELBO term log p(y) - log q0(x) + ladj is assembled from.
    With the cloud as the draws log q0(x) = -|x|^2 / 2 - ... is as large as log p(y) on the far clouds and cancels most of it
    (Banana's y1 at 30 under var = 1: -450 against -450, a term of a few units).  log p, log q0 and ladj are three separately
    rounded float32 sums over d features; a pairwise sum over d <= 129 features is a tree of ceil(log2 129) = 8 roundings, each at
    most half a unit in the last place of a partial sum no larger than the whole.  So ANY float32 evaluation may be off by
    TERM_ULPS x 2^-24 x terms, however exact its arithmetic, and one evaluation (the float32 oracle's) that happens to land within
    0.25 TOL of the difference says nothing about another's.  Two rules follow, both from the oracles and the inputs alone:
      an ELBO-term element counts as conditioned only if, besides the float32 oracle's error, that bound fits its tolerance:
        TERM_ULPS x 2^-24 x terms <= TOL;
      an ELBO-term array whose float32-oracle figure by |ref|inf exceeds 0.1 GRAD_RTOL takes the largest term of the cloud as the
        scale of the gradient measure, under the same two bounds (float32 oracle <= 0.1 GRAD_RTOL, device <= GRAD_RTOL).
    This narrows the issue's rules for ELBO terms (not for site 1's log p and score, which are held exactly as stated there, on
    the same points, without the cancellation)."""
    lq = o.std_normal_logpdf(np.asarray(xs, dtype=np.float64))
    return np.abs(e64 + lq) + np.abs(lq)


def aggregate_ok(e64, l64, l32, g64, g32, terms=None):
    """(loss eligible, gradient eligible): condition 5 of the module docstring, from the oracles alone -- and for the loss, by
    term_scale's reasoning, that TERM_ULPS x 2^-24 x the mean term fits LOSS_RTOL |loss|: the loss of a far batch is a mean of
    cancelling ELBO terms (one sample of Banana's y1 at 30, d = 129: 15.95 left of two terms of 520, whose last place is 6e-5)"""
    loss_ok = abs(l32 - l64) <= FLOOR_SHARE * LOSS_RTOL * abs(l64) and abs(l64) >= 0.1 * float(np.abs(e64).mean())
    if terms is not None:
        loss_ok = loss_ok and TERM_ULPS * 2.0 ** -24 * float(np.abs(terms).mean()) <= LOSS_RTOL * abs(l64)
    gs = max(float(np.abs(g64).max()), 1e-300)
    return bool(loss_ok), bool(np.isfinite(g32).all() and float(np.abs(g32 - g64).max()) / gs <= FLOOR_SHARE * GRAD_RTOL)


def make_flow(nf, torch, kind, d, f64, nl=None):
    dt = torch.float64 if f64 else torch.float32
    th = torch.tensor(flow_theta(kind, d, nl), dtype=dt, device="cuda")
    if kind == "realnvp":
        return nf.Flow("realnvp", nf.MvNormal(d), 1, HDIMS, dtype=dt, device="cuda", theta=th), dt
    return nf.Flow(kind, nf.MvNormal(d), 1 if kind in ("meanfield", "fullrank") else (nl or SIMPLE_NL), dtype=dt, device="cuda", theta=th), dt


def targets_at(d):
    return tuple(t for t in TARGETS if d == 2 or t not in D2)


def flow_site(nf, kind, f64, d, nl=None, chk=None, tag="", no_tile=False):
    """Sites 2-6 at (flow kind, dtype, d): every target that exists at d, every parameter set, every cloud as supplied draws (n by
    n_of): nf.batched_elbos against o.batched_elbos under `hold`, nf.value_and_gradient against o.neg_elbo_value_and_grad where
    `aggregate_ok`; the launches by profiler name.  Only site 2 gets a per-sample check this way: behind a simple flow
    nf.batched_elbos evaluates the target with k_target (site 1), and the training entry points of sites 3-6 return no per-sample
    output, so those four sites are held by loss and gradient alone.
    Returns (chk, {target: [eligible losses, eligible gradients, cases]})."""
    import torch

    chk = chk or Checks()
    P = chk.P
    flow, dt = make_flow(nf, torch, kind, d, f64, nl)
    train = train_launch(kind, f64, d, nl, no_tile)
    counts = {}
    for target in targets_at(d):
        cnt = counts.setdefault(target, [0, 0, 0])
        for pi in range(len(PARAMS[target])):
            tgt, ot = device_target(nf, torch, target, pi, d, dt), otarget(target, pi, d)
            for ci, c in enumerate(clouds(target, pi, d)):
                n = n_of(pi, ci)
                xs = points(target, pi, d, ci)[:, :n]
                flow_name = f"target regimes: {tag}{kind} {'f64' if f64 else 'f32'}{' x' + str(nl) if nl else ''}"
                # keyed by what ran: the per-sample terms come from nf.batched_elbos -- k_target_tiled behind RealNVP / full-rank, but
                # k_simple_apply WITHOUT its target and then k_target (site 1) behind a simple flow; loss and gradient from the training launch
                group_e = f"{flow_name} (batched_elbos: {'target_tiled' if train == 'target' else 'simple_apply, then k_target'}) {target} d={d}: "
                group = f"{flow_name} (value_and_gradient: {'target_tiled' if train == 'target' else train}) {target} d={d}: "
                detail = f"{params(target, pi) if target != 'diaggauss' else 'draw ' + str(pi)} {c.name} n={n}"
                key = f"{group}({detail}) "
                e64, l64, g64 = flow_oracle(kind, d, ot, xs, np.float64, nl)
                e32, l32, g32 = flow_oracle(kind, d, ot, xs, np.float32, nl)
                if not (np.isfinite(e64).all() and np.isfinite(g64).all()):
                    chk.failed.append(key + "the float64 oracle is not finite: a defect of the case")
                    continue
                xd = _cm(torch, xs, dt)
                got = {}
                ran_b = launched(nf, flow.ctx, lambda: got.update(e=nf.batched_elbos(flow, tgt, xd)))
                ran_t = launched(nf, flow.ctx, lambda: got.update(vg=nf.value_and_gradient(nf.elbo_batch, flow, tgt, xd)))
                if train == "target":  # site 2: the tiled route converts the layout first; the flat full-rank route does not run
                    ok_b = only(ran_b, target=1) and ran_b["layout_convert"] >= 1 and not ran_b["fr_apply_flat"]
                    ok_t = only(ran_t, target=1) and ran_t["layout_convert"] >= 1 and not ran_t["fr_grad_flat"]
                else:
                    ok_b = only(ran_b, simple_apply=1, target=1)  # (the forward without its fused target, then site 1)
                    ok_t = only(ran_t, simple_apply=1) and ran_t["simple_bwd"] == 1 if train == "split" else only(ran_t, **{train: 1})
                if not (ok_b and ok_t):
                    chk.failed.append(key + f"launches: expected {train}, batched_elbos ran {ran_b}, value_and_gradient ran {ran_t}")
                hold(chk, group_e + "ELBO terms", detail, got["e"], e64, e32, f64, terms=term_scale(e64, xs))
                loss, g = got["vg"]
                lok, gok = aggregate_ok(e64, l64, l32, g64, g32.astype(np.float64), term_scale(e64, xs))
                cnt[0], cnt[1], cnt[2] = cnt[0] + lok, cnt[1] + gok, cnt[2] + 1
                if lok:
                    aggregate(chk, "scalar", group + "loss", detail, loss, l64, F64_RTOL if f64 else LOSS_RTOL, floor=None if f64 else l32)
                if gok:
                    aggregate(chk, "gradient", group + "gradient", detail, g, g64, F64_GRAD if f64 else GRAD_RTOL, floor=None if f64 else g32)
    return chk, counts


# ----------------------------------------------------------------------------------------------------------------------
# sites 7, 8: in-library draws; the flow places the cloud (module docstring)
# ----------------------------------------------------------------------------------------------------------------------
PLACE_L, PLACE_TANH = 4, 0.9              # RealNVP blocks; the largest |tanh b_s| prescribed
SEED_DRAW = 77
NSF_K, NSF_B, NSF_L, NSF_BIAS = 8, 5.0, 2, 1.0  # the K = 8 spline geometry of the fused chain kernel; output biases of scale NSF_BIAS
# d = 2: the D2 arm and the one-term s2; 33: the second register block's first feature; 64 / 32: full blocks (the fused K = 8 spline
# chain serves d <= 32: beyond it an NSF flow takes the standard-layout route, site 1)
PLACED_DIMS = {"realnvp": (2, 3, 9, 33, 64), "nsf": (2, 3, 9, 32)}
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def placed_spec(kind, d):
    return o.FlowSpec("realnvp", d, PLACE_L, HDIMS) if kind == "realnvp" else o.FlowSpec("nsf", d, NSF_L, HDIMS, NSF_K, NSF_B)


def reachable(target, pi, d, ci):
    """True where the RealNVP placement reaches cloud ci; DiagGauss' own cloud is reached with its scales clipped"""
    lim = np.exp(PLACE_L * PLACE_TANH)
    s = clouds(target, pi, d)[ci].scale
    return target == "diaggauss" or bool((s >= 1.0 / lim).all() and (s <= lim).all())


@functools.lru_cache(maxsize=None)
def placed_theta(kind, target, pi, d, ci):
    """RealNVP: Glorot hidden layers, zero output weights, output biases that carry N(0, 1) to the cloud -- each of the PLACE_L couplings
    of a coordinate takes an equal share of log scale, the coupling applied last (flat index 0 / 1) the whole centre.
    NSF: Glorot hidden layers, zero output weights, output biases NSF_BIAS N(0, 1): one fixed spline per coordinate and coupling."""
    spec = placed_spec(kind, d)
    rng = np.random.default_rng([41, FLOW_KINDS.index("realnvp") if kind == "realnvp" else 9, TARGETS.index(target), pi, d, ci])
    th = o.init_params(spec, rng)
    c = clouds(target, pi, d)[ci]
    lim = np.exp(PLACE_L * PLACE_TANH)
    for k, li in enumerate(o.layers_flat_order(spec)):
        for ni, net in enumerate(li.nets):
            w_off, b_off, nout, nin = net[-1]
            th[w_off:w_off + nout * nin] = 0.0
            if kind == "nsf":
                th[b_off:b_off + nout] = NSF_BIAS * rng.standard_normal(nout)
            elif ni == 0:
                th[b_off:b_off + nout] = np.arctanh(np.log(np.clip(c.scale[li.idx_t], 1.0 / lim, lim)) / PLACE_L)
            else:
                th[b_off:b_off + nout] = c.centre[li.idx_t] if k < 2 else 0.0
    th = _f32r(th)
    th.setflags(write=False)
    return th


ELIGIBLE_SHARE = 0.5  # of a (flow, d, target)'s cases, the losses and the gradients that must be eligible for the aggregate checks


def eligible_enough(nl, ng, nall):
    """the aggregate checks are not vacuous: at least ELIGIBLE_SHARE of the cases' losses and of their gradients pass aggregate_ok
    (measured with the oracles alone over every row of FLOW_CASES: the smallest shares are 65 % of the losses -- Banana, whose far
    clouds cancel -- and 50 % of the gradients -- DiagGauss, four cases per d)"""
    return nl >= ELIGIBLE_SHARE * nall and ng >= ELIGIBLE_SHARE * nall


def placed_site(nf, kind, target, d, chk=None):
    """Sites 7 (kind = "realnvp") and 8 ("nsf") at (target, d): every parameter set; RealNVP every reachable cloud, NSF one flow per
    parameter set.  nf_elbo_value_and_grad(xs = NULL) and one nf_elbo_step against the oracle on the regenerated draws
    (nf.device_specific_rand with the same seed; the Float32 sampler is held to o.base_sample elsewhere), under `aggregate_ok`;
    and the cross-site check: the same y (nf_flow_fwd of those draws) through site 1, sum of site 1's per-sample terms against
    the fused loss -- it shares neither the forward kernel nor the epilogue.  Launches by profiler name."""
    import ctypes as C

    import torch

    chk = chk or Checks()
    dt = torch.float32
    spec = placed_spec(kind, d)
    lib = nf.load_library()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    counts = [0, 0, 0]
    fused_name = ("affine_chain" if target == "diaggauss" else "affine_chain_tgt") if kind == "realnvp" else ("rqs_chain" if target == "diaggauss" else "rqs_chain_tgt")
    for pi in range(len(PARAMS[target])):
        tgt, ot = device_target(nf, torch, target, pi, d, dt), otarget(target, pi, d)
        cis = [ci for ci in range(len(clouds(target, pi, d))) if reachable(target, pi, d, ci)] if kind == "realnvp" else [0]
        for ci in cis:
            n = n_of(pi, ci)
            cname = clouds(target, pi, d)[ci].name if kind == "realnvp" else f"output biases x{NSF_BIAS:g}"
            group = f"target regimes: {kind} in-library draws ({fused_name}) {target} d={d}: "
            detail = f"{params(target, pi) if target != 'diaggauss' else 'draw ' + str(pi)} {cname} n={n}"
            th = placed_theta(kind, target, pi, d, ci)
            if kind == "realnvp":
                flow = nf.Flow("realnvp", nf.MvNormal(d), PLACE_L, HDIMS, dtype=dt, device="cuda", theta=torch.tensor(th, dtype=dt, device="cuda"))
            else:
                flow = nf.Flow("nsf", nf.MvNormal(d), NSF_L, HDIMS, NSF_K, NSF_B, dtype=dt, device="cuda", theta=torch.tensor(th, dtype=dt, device="cuda"))
            xs_d = nf.device_specific_rand(nf.PhiloxRNG(SEED_DRAW), flow.dist, n, dtype=dt)
            xs = xs_d.cpu().numpy().astype(np.float64)
            with np.errstate(all="ignore"):
                e64 = o.batched_elbos(spec, th, ot, xs)
                l64, g64 = o.neg_elbo_value_and_grad(spec, th, ot, xs)
                ot32 = tuple(v.astype(np.float32) if isinstance(v, np.ndarray) else (np.float32(v) if not isinstance(v, str) else v) for v in ot)
                l32, g32 = o.neg_elbo_value_and_grad(spec, th.astype(np.float32), ot32, xs.astype(np.float32))
            if not (np.isfinite(e64).all() and np.isfinite(g64).all()):
                chk.failed.append(f"{group}({detail}) the float64 oracle is not finite: a defect of the case")
                continue
            got = {}
            ran = launched(nf, flow.ctx, lambda: got.update(vg=nf.value_and_gradient(nf.elbo_batch, flow, tgt, n, rng=nf.PhiloxRNG(SEED_DRAW))))
            if not only(ran, **({} if target == "diaggauss" else {fused_name: True})) or ran[fused_name] < 1:
                chk.failed.append(f"{group}({detail}) launches: expected {fused_name} alone, ran {ran}")
            loss, g = got["vg"]
            th_a, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)
            sl, sg = C.c_double(0), C.c_double(0)
            ran_s = launched(nf, flow.ctx, lambda: nf._lib.check(lib.nf_elbo_step(flow.ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_a), vp(m), vp(v),
                                                                                  n, SEED_DRAW, 0, LR, B1, B2, EPS, C.byref(sl), C.byref(sg))))
            if not only(ran_s, **({} if target == "diaggauss" else {fused_name: True})) or ran_s[fused_name] < 1:
                chk.failed.append(f"{group}({detail}) launches of nf_elbo_step: expected {fused_name} alone, ran {ran_s}")
            lok, gok = aggregate_ok(e64, float(l64), float(l32), g64, g32.astype(np.float64), term_scale(e64, xs))
            counts[0], counts[1], counts[2] = counts[0] + lok, counts[1] + gok, counts[2] + 1
            if lok:
                aggregate(chk, "scalar", group + "loss", detail, loss, l64, LOSS_RTOL, floor=l32)
                aggregate(chk, "scalar", group + "nf_elbo_step loss", detail, sl.value, l64, LOSS_RTOL, floor=l32)
            if gok:
                aggregate(chk, "gradient", group + "gradient", detail, g, g64, GRAD_RTOL, floor=g32)
                aggregate(chk, "gradient", group + "nf_elbo_step first moment / (1 - beta1)", detail, m / (1.0 - B1), g64, GRAD_RTOL, floor=g32)
            # cross-site: the same y through k_target, its per-sample terms summed in float64, against the fused loss.  Both are Float32
            # evaluations of the same terms, each within 2^-24 x TERM_ULPS of its largest term per sample (term_scale); the bound is
            # that, taken over the mean of |terms|, plus LOSS_RTOL of the loss itself.
            ys, ladj = nf.with_logabsdet_jacobian(flow.transform, xs_d)
            lp = nf.target_logp(tgt, ys)
            lq = torch.tensor(o.std_normal_logpdf(xs), dtype=torch.float64, device="cuda")
            split = float(-(lp.double() - lq + ladj.double()).mean())
            bound = LOSS_RTOL * abs(l64) + 2.0 * TERM_ULPS * 2.0 ** -24 * float(term_scale(e64, xs).mean())
            _rec(chk.P, group + "sum of site 1's terms against the fused loss [|diff| / bound]", abs(split - loss) / bound)
            if abs(split - loss) > bound:
                chk.failed.append(f"{group}({detail}) site 1 on the same y sums to {split!r}, the fused forward to {loss!r} (bound {bound:.3e})")
    return chk, counts
