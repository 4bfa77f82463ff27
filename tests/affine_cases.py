"""RealNVP cases away from Glorot initialisation: prescribed conditioner biases and scale outputs, inputs far from the origin.

A plain module (no pytest, no torch at import), importable from a child process: tests/test_affine_cases_cpu.py holds the cases
to the conditions that keep a parity check meaningful, tests/test_gpu_affine_regimes.py runs them on the device -- in process,
and once per arithmetic switch in a child process.

Flows are FlowSpec("realnvp", d, 1, hdims): two couplings.  `theta()` starts from the reference's initialisation (Glorot weights,
zero biases) and then writes

  last layer of the s net   W_out *= gain (gain = 0: s is the same for every sample and fully prescribed; gain = 1: the sample
                            dependence of a Glorot W_out on top); b_out from a PROFILE per transformed dimension, shifted by one
                            per coupling (s = tanh(z)):
                                sat+    z = +4                    s ~ +1 (1 - s^2 = 1.3e-3)
                                sat-    z = -4                    s ~ -1
                                clamp   z = +8, -8.25, +9, -8, +8.25, -9 in turn (counted over both couplings): the three sides
                                        of nf_tanh's clamp at 8.124 -- beyond x^2 = 66 the reference returns +-1
                                linear  z = 0.3 N(0, 1)
                                zero    z = 0                     what initialisation looks like
  last layer of the t net   b_out = 2 N(0, 1)
  every hidden layer        b = 0.5 N(0, 1), with unit 0, 8, 16, ... at -3 (deep in the leaky arm), unit 1, 9, ... at +3 and
  of both nets              unit 2, 10, ... at exactly 0; the weight rows of the -3 and +3 units are HELD_ROW_SCALE x their Glorot
                            draw, so that those units are dead / always on for the whole gradient batch by construction (with full
                            Glorot rows a third to a half of them crossed 0 on some column at d >= 16)

Everything (theta, inputs, target parameters, cotangents) is rounded to float32-representable values, for the Float64 cases too,
so the float32 oracle and the device see the float64 oracle's numbers.

Inputs.
  value set     72 columns (two 32-sample tiles and a ragged tail), for forward ys / ladj: 17 columns of N(0, 1) at each of the
                scales 0.3, 1, 2 and 4 | one all-zero column | one column of +-30 | one of 1e-20 N(0, 1) | one whose rows
                alternate 1e3 and 1e-3 in magnitude
  inverse set   the float32-rounded forward image of the value set, compared against o.flow_inv (not as a round trip), without
                the +-30, 1e-20 and 1e3 / 1e-3 columns: (y - t) e^-s cancels there (y = x e^s + t with |t| >> |x e^s|, or y
                ~ 1e3 carrying an absolute rounding error of 6e-5 into an x of 1e-3) and the float32 ORACLE's inverse x is
                hundreds to thousands of times the plain tolerance off -- a floor that would license any kernel
  gradient set  72 columns of N(0, 1), 24 at each of the scales 0.3, 1 and 2, no extreme column: the gradient criterion is
                max |err| / |g|inf, and with an extreme column in the batch that column owns |g|inf and the check says nothing
                about the rest.  Columns that put a hidden pre-activation of the float64 oracle within REDRAW_MARGIN of 0 are
                redrawn (a unit that close to its kink takes the other slope in float32); that is also why there is no all-zero
                column here -- the prescribed zero-bias units would sit exactly on the kink.
  forward-KL    the float64 oracle's forward image of the gradient set, rounded to float32
  tape          the gradient set with cotangents of one sign per feature (|N(0, 1)| / n, alternating by feature) and a negative
                lbar, as a mean objective's are (tests/test_gpu_cotangent_carry.py::test_pullback_against_oracle)

The exact-zero pre-activation (`zero=True`, part of the Case).  In the FIRST Dense layer of both nets of both couplings the
units ZERO_UNITS get all-zero weight rows and a zero bias; their outgoing weights stay.  Their pre-activation is +0 for every
sample in every precision, and the reference's leakyrelu differentiates it with slope 0.01 (ifelse(x > 0, x, 0.01x)); a kernel
that takes the slope from the activation's sign bit differentiates it with 1 and returns db and dW rows 100 x the reference's.
(The hidden-64 stashing forward behind k_affine_bwd_pair still does, for its cost: tests/test_gpu_affine_regimes.py, PAIR_COST.)
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
from gradient_floors import fp32_recompute_floor, min_abs_preact as _min_abs_preact  # noqa: E402,F401

Case = namedtuple("Case", "dtype d hdims gain zero")
PROFILES = ("sat+", "sat-", "clamp", "linear", "zero")
CLAMP_Z = (8.0, -8.25, 9.0, -8.0, 8.25, -9.0)  # |z| = 8 inside nf_tanh's clamp (x^2 = 64 < 66), 8.25 and 9 beyond it
HELD_ROW_SCALE = 0.05     # weight rows of the -3 / +3 units: a Glorot row of fan-in 32 spreads the pre-activation by 1.6 on inputs of
#                           scale 2 (more behind the first coupling), which carries a bias of 3 across 0; at a twentieth those units stay
#                           in their arm for the whole gradient batch (tests/test_affine_cases_cpu.py asserts EVERY one of them does)
ZERO_UNITS = (2, 5, 12)   # first-layer units of the zero=True cases (every first hidden layer here has at least 16 units)
REDRAW_MARGIN = 1e-4      # gradient-set columns closer than this to a kink are redrawn (the CPU test requires 5e-5 of what is left)
N_VAL, N_GRAD = 72, 72
EXTREME = ("pm30", "tiny", "mixed")  # roles of the value-set columns the inverse set leaves out
FWD_EXTREME = ("zero", "pm30", "tiny", "mixed")  # ... and those the forward checks take one by one

# shape -> (dtype, d, hdims); the kernels it reaches, by geo_size / nf_deep_geo_id (nf_coupling.hip, nf_deep.hip),
# nf_wide_supported / wide_fits_mid (nf_wide.hip), l64_ok (nf_generic64.hip) and g64m_geo (nf_g64m.h).  Every shape lands where
# the table says; none had to move -- that is a reading of those five functions against (d, hdims), written out shape by shape below.
# FAMILY: what a test can observe, the profiler names (nf_prof_read) of the forward and the reverse launch.  They tell the six
# families apart, not the geometries inside one (NetGeo<1,1,1,1> from <1,2,2,1>, the deep ids, GM from GW, g64m 12 from 24,
# k_affine_bwd_pair from k_affine_bwd: one name each).
SHAPES = {
    "f32_d6_h32": ("float32", 6, (32, 32)),               # NetGeo<1,1,1,1> (3 conditioner inputs, one block everywhere)
    "f32_d64_h64": ("float32", 64, (64, 64)),             # NetGeo<1,2,2,1>, full feature blocks: stashing forward, k_affine_bwd_pair
    "f32_d63_h40x64": ("float32", 63, (40, 64)),          # NetGeo<1,2,2,1>, the form with feature masks (32 / 31 rows, 40 of 64 units)
    "f32_d16_h24": ("float32", 16, (24,)),                # nf_deep.hip id 11 (one hidden layer, one block)
    "f32_d16_h64x3": ("float32", 16, (64, 64, 64)),       # nf_deep.hip id 32
    "f32_d12_h32x4": ("float32", 12, (32, 32, 32, 32)),   # nf_deep.hip id 41
    "f32_d10_h96": ("float32", 10, (96,)),                # one hidden layer of three blocks: outside the deep envelope -> l64
    "f32_d70_h40x96": ("float32", 70, (40, 96)),          # 35 conditioner inputs = two blocks: wide, GM = NetGeo<2,4,4,2>
    "f32_d130_h136x40": ("float32", 130, (136, 40)),      # 65 inputs = three blocks, 136 units = five: wide, GW
    "f64_d8_h16": ("float64", 8, (16,)),                  # nf_g64m.h id 12
    "f64_d40_h64": ("float64", 40, (64, 64)),             # nf_g64m.h id 24
    "f64_d6_h40x3": ("float64", 6, (40, 40, 40)),         # three hidden layers in Float64: the scalar g64_* kernels
}
FAMILY = {
    "f32_d6_h32": "netgeo", "f32_d64_h64": "netgeo", "f32_d63_h40x64": "netgeo", "f32_d16_h24": "deep", "f32_d16_h64x3": "deep",
    "f32_d12_h32x4": "deep", "f32_d10_h96": "l64", "f32_d70_h40x96": "wide", "f32_d130_h136x40": "wide", "f64_d8_h16": "g64m",
    "f64_d40_h64": "g64m", "f64_d6_h40x3": "g64",
}
FAMILY_PROF = {  # family -> (forward launches: one of them runs, reverse launch)
    "netgeo": (("affine_apply", "affine_chain"), "affine_bwd"), "deep": (("deep_chain",), "deep_bwd"), "l64": (("l64_fwd",), "l64_dw"),
    "wide": (("wide_apply",), "wide_bwd"), "g64m": (("g64m_apply",), "g64m_bwd"), "g64": (("g64_apply",), "g64_bwd"),
}
NETGEO = tuple(s for s, f in FAMILY.items() if f == "netgeo")  # fused nf_elbo_step, fused target forward, stash budget
RECOMPUTES = tuple(s for s, f in FAMILY.items() if f in ("netgeo", "deep"))  # a reverse pass by invertible recompute exists
ZERO_SHAPES = ("f32_d6_h32", "f32_d64_h64", "f32_d16_h64x3", "f32_d70_h40x96", "f32_d10_h96", "f64_d8_h16")


def case(shape, gain, zero=False):
    return Case(*SHAPES[shape], gain, zero)


def shape_of(c):
    return next(k for k, v in SHAPES.items() if v == tuple(c[:3]))


def case_name(c):
    return f"{shape_of(c)} gain={c.gain}" + (" zero-units" if c.zero else "")


ALL_CASES = [case(s, g) for s in SHAPES for g in (0, 1)]
ZERO_CASES = [case(s, 1, True) for s in ZERO_SHAPES]


def spec_of(c):
    return o.FlowSpec("realnvp", c.d, 1, tuple(c.hdims))


def _f32r(a):
    """float64 array of float32-representable values"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# Seeds changed under the conditions of tests/test_affine_cases_cpu.py (measured with the oracle alone): none so far.
SEED_SALT = {}


def _seed(c):
    return 1000 * c.d + len(c.hdims) + SEED_SALT.get(shape_of(c), 0)


def profile_of(ci, t):
    """profile name of transformed dimension t of coupling ci (flat order)"""
    return PROFILES[(t + ci) % len(PROFILES)]


def theta(c):
    spec = spec_of(c)
    rng = np.random.default_rng(_seed(c))
    th = o.init_params(spec, rng)
    nclamp = 0
    for ci, li in enumerate(o.layers_flat_order(spec)):
        for ni, net in enumerate(li.nets):
            for (w_off, b_off, nout, nin) in net[:-1]:
                b = 0.5 * rng.standard_normal(nout)
                b[0::8], b[1::8], b[2::8] = -3.0, 3.0, 0.0
                th[b_off:b_off + nout] = b
                W = th[w_off:w_off + nout * nin].reshape(nin, nout)  # W[o, i] at w_off + i * nout + o: a view
                W[:, 0::8] *= HELD_ROW_SCALE
                W[:, 1::8] *= HELD_ROW_SCALE
            w_off, b_off, nout, nin = net[-1]
            if ni == 1:
                th[b_off:b_off + nout] = 2.0 * rng.standard_normal(nout)
                continue
            th[w_off:w_off + nout * nin] *= c.gain
            for t in range(nout):
                p, lin = profile_of(ci, t), 0.3 * rng.standard_normal()
                if p == "clamp":
                    z, nclamp = CLAMP_Z[nclamp % len(CLAMP_Z)], nclamp + 1
                else:
                    z = {"sat+": 4.0, "sat-": -4.0, "linear": lin, "zero": 0.0}[p]
                th[b_off + t] = z
        if c.zero:
            for net in li.nets:
                w_off, b_off, nout, nin = net[0]  # W[o, i] at w_off + i * nout + o
                for u in ZERO_UNITS:
                    th[w_off + u:w_off + nout * nin:nout] = 0.0
                    th[b_off + u] = 0.0
    return _f32r(th)


def zero_bias_index(c):
    """flat theta indices of the ZERO_UNITS' biases: 3 units x 2 nets x 2 couplings"""
    return np.array([net[0][1] + u for li in o.layers_flat_order(spec_of(c)) for net in li.nets for u in ZERO_UNITS])


def zero_weight_index(c):
    """flat theta indices of the ZERO_UNITS' (all-zero) weight rows"""
    out = []
    for li in o.layers_flat_order(spec_of(c)):
        for net in li.nets:
            w_off, _, nout, nin = net[0]
            out += [w_off + i * nout + u for u in ZERO_UNITS for i in range(nin)]
    return np.array(out)


def hidden_preacts(spec, th, xs):
    """[(coupling in flat order, net, hidden layer, z (units, n))] of the oracle's forward pass on xs"""
    _, _, states = o.flow_fwd(spec, th, xs, keep=True)
    layers = o.layers_flat_order(spec)
    out = []
    for ci, x in zip(range(len(layers) - 1, -1, -1), states):
        li = layers[ci]
        for ni, net in enumerate(li.nets):
            _, acts = o.mlp_forward(th, net, x[li.idx_c], None, keep=True)
            for l, a in enumerate(acts[1:-1]):  # a = leakyrelu(z): z = a for a > 0, a / 0.01 otherwise
                out.append((ci, ni, l, np.where(a > 0, a, a / 0.01)))
    return out


def min_abs_preact(c, th, xs):
    """per sample, the smallest |pre-activation| of any leaky-ReLU unit in the oracle's forward pass (tests/gradient_floors.py)
    -- without the ZERO_UNITS of a zero=True case, which are 0 by design"""
    return _min_abs_preact(spec_of(c), th, xs, ZERO_UNITS if c.zero else ())


def _value_set(c, rng):
    d = c.d
    cols, roles = [], []
    for s in (0.3, 1.0, 2.0, 4.0):
        cols.append(s * rng.standard_normal((d, 17)))
        roles += [f"n{s:g}"] * 17
    cols.append(np.zeros((d, 1)))
    cols.append(30.0 * np.where(rng.uniform(size=(d, 1)) < 0.5, -1.0, 1.0))
    cols.append(1e-20 * rng.standard_normal((d, 1)))
    mixed = np.where(np.arange(d)[:, None] % 2 == 0, 1e3, 1e-3) * np.where(rng.uniform(size=(d, 1)) < 0.5, -1.0, 1.0)
    cols.append(mixed)
    roles += ["zero", "pm30", "tiny", "mixed"]
    return _f32r(np.concatenate(cols, axis=1)), np.array(roles)


def _grad_set(c, th, rng):
    scale = np.repeat([0.3, 1.0, 2.0], N_GRAD // 3)[None, :]
    xs = _f32r(rng.standard_normal((c.d, N_GRAD)) * scale)
    for _ in range(20):
        near = min_abs_preact(c, th, xs) < REDRAW_MARGIN
        if not near.any():
            return xs, scale[0]
        xs[:, near] = _f32r(rng.standard_normal((c.d, int(near.sum()))) * scale[:, near])
    raise AssertionError("gradient set: columns near a kink after 20 redraws")


Built = namedtuple("Built", "case spec th xs_val roles_val ys_inv xs_grad scale_grad ys_fkl ybar lbar mu var")


@functools.lru_cache(maxsize=None)
def build(c):
    spec, th = spec_of(c), theta(c)
    rng = np.random.default_rng(_seed(c) + 1)
    xs_val, roles_val = _value_set(c, rng)
    with np.errstate(all="ignore"):
        ys_inv = _f32r(o.flow_fwd(spec, th, xs_val[:, ~np.isin(roles_val, EXTREME)])[0])
    xs_grad, scale_grad = _grad_set(c, th, rng)
    ys_fkl = _f32r(o.flow_fwd(spec, th, xs_grad)[0])
    mu, var = _f32r(rng.standard_normal(c.d)), _f32r(rng.uniform(size=c.d) + 0.5)
    sign = np.where(np.arange(c.d) % 2 == 0, 1.0, -1.0)[:, None]
    ybar = _f32r(sign * np.abs(rng.standard_normal((c.d, N_GRAD))) / N_GRAD)
    lbar = _f32r(-(0.5 + rng.uniform(size=N_GRAD)) / N_GRAD)
    for a in (th, xs_val, ys_inv, xs_grad, ys_fkl, ybar, lbar, mu, var):
        a.setflags(write=False)
    return Built(c, spec, th, xs_val, roles_val, ys_inv, xs_grad, scale_grad, ys_fkl, ybar, lbar, mu, var)


def _oracle(b, dt):
    th, mu, var = b.th.astype(dt), b.mu.astype(dt), b.var.astype(dt)
    tgt = ("diaggauss", mu, var)
    r = {}
    r["ys"], r["ladj"] = o.flow_fwd(b.spec, th, b.xs_val.astype(dt))
    r["x_inv"], r["ladj_inv"] = o.flow_inv(b.spec, th, b.ys_inv.astype(dt))
    r["elbo_loss"], r["elbo_grad"] = o.neg_elbo_value_and_grad(b.spec, th, tgt, b.xs_grad.astype(dt))
    r["fkl_loss"], r["fkl_grad"] = o.neg_loglik_value_and_grad(b.spec, th, b.ys_fkl.astype(dt))
    _, _, states = o.flow_fwd(b.spec, th, b.xs_grad.astype(dt), keep=True)
    r["tape_xbar"], r["tape_grad"] = o.flow_bwd(b.spec, th, states, b.ybar.astype(dt), b.lbar.astype(dt))
    return r


@functools.lru_cache(maxsize=None)
def reference(c):
    """{"f64": ..., "f32": ...}: the oracle in float64 and, op by op, in IEEE float32 on the same inputs (the fp32 floor)"""
    b = build(c)
    with np.errstate(all="ignore"):
        return {"f64": _oracle(b, np.float64), "f32": _oracle(b, np.float32)}


# ----------------------------------------------------------------------------------------------------------------------
# the device checks of one case (tests/test_gpu_affine_regimes.py: in process, and in a child process per switch)
# ----------------------------------------------------------------------------------------------------------------------
ALL_PARTS = ("fwd", "inv", "layer", "elbo", "elbo_rng", "tape", "step", "fkl")


def parts_of(shape, layer=True):
    return tuple(p for p in ALL_PARTS if (p != "step" or shape in NETGEO) and (p != "layer" or layer))


class Checks:
    """tests/parity.py's criteria, every figure recorded and every failure kept, so that one miss does not hide the rest"""

    def __init__(self):
        import parity

        self.P = parity
        self.failed = []

    def __call__(self, fn, *args, **kw):
        try:
            getattr(self.P, fn)(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e))

    def exact(self, key, ok):
        self.P.record(key + " [exact: 1 holds]", 1.0 if ok else 0.0)
        if not ok:
            self.failed.append(key + ": not exact")


def _cm(torch, a, dt):
    """numpy (d, N) -> column-major torch (d, N)"""
    return torch.tensor(np.ascontiguousarray(a.T), dtype=dt, device="cuda").t()


def make_flow(nf, c, torch):
    b = build(c)
    dt = torch.float64 if c.dtype == "float64" else torch.float32
    flow = nf.Flow("realnvp", nf.MvNormal(c.d), 1, tuple(c.hdims), 0, 0.0, dtype=dt, device="cuda", theta=torch.tensor(b.th, dtype=dt, device="cuda"))
    tgt = nf.DiagGaussTarget(torch.tensor(b.mu, dtype=dt, device="cuda"), torch.tensor(b.var, dtype=dt, device="cuda"))
    return flow, tgt, dt


def launched(nf, flow, run):
    """{profiler name: launches} of FAMILY_PROF's names while `run()` executes"""
    import ctypes as C

    import torch

    lib, ctx = nf.load_library(), flow.ctx
    nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
    try:
        run()
        torch.cuda.synchronize()
        ran = {}
        for name in sorted({n for fwd, bwd in FAMILY_PROF.values() for n in fwd + (bwd,)}):
            a, k = C.c_double(0.0), C.c_int64(0)
            lib.nf_prof_read(ctx.ptr, name.encode(), C.byref(a), C.byref(k))
            ran[name] = int(k.value)
    finally:
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
    return ran


def dispatch(nf, c):
    """launch counts of one forward and one ELBO value-and-gradient (supplied draws) of case c"""
    import torch

    b = build(c)
    flow, tgt, dt = make_flow(nf, c, torch)

    def run():
        nf.with_logabsdet_jacobian(flow.transform, _cm(torch, b.xs_val, dt))
        nf.value_and_gradient(nf.elbo_batch, flow, tgt, _cm(torch, b.xs_grad, dt))

    return launched(nf, flow, run)


def family_ok(ran, family):
    """the family's forward and reverse launches ran, and no other family's"""
    fwd, bwd = FAMILY_PROF[family]
    # g64_apply / g64_bwd are the standard-layout route's scopes around every coupling: l64 and g64m launch inside them
    allowed = fwd + (bwd,) + (FAMILY_PROF["g64"][0] + (FAMILY_PROF["g64"][1],) if family in ("l64", "g64m") else ())
    return any(ran[n] > 0 for n in fwd) and ran[bwd] > 0 and not any(v for n, v in ran.items() if n not in allowed)


def device_checks(nf, c, parts=ALL_PARTS, chk=None, tag=""):
    """Run `parts` of case c on the device against the oracle; returns the Checks (figures in parity.MEASURED under
    'affine regimes: ...', failures in .failed)."""
    import ctypes as C

    import torch

    chk = chk or Checks()
    P = chk.P
    b, r = build(c), reference(c)
    r64, r32 = r["f64"], r["f32"]
    f64 = c.dtype == "float64"
    key = f"affine regimes: {tag}{case_name(c)}: "
    ew = dict(rtol=P.F64_RTOL, atol=1e-12) if f64 else dict(rtol=P.Y_RTOL, atol=P.Y_ATOL)
    lr = P.F64_RTOL if f64 else P.LOSS_RTOL
    gr = P.F64_GRAD if f64 else P.GRAD_RTOL
    fl = (lambda name: None) if f64 else (lambda name: r32[name])  # Float64: no floor
    flow, tgt, dt = make_flow(nf, c, torch)
    otgt = ("diaggauss", b.mu, b.var)
    layers = o.layers_flat_order(b.spec)
    n = b.xs_grad.shape[1]
    lib, ctx = nf.load_library(), flow.ctx
    xs_val, xs_grad = _cm(torch, b.xs_val, dt), _cm(torch, b.xs_grad, dt)

    def chain_by_layer():
        """nf_layer_apply of each coupling, the last in flat order first: (y, ladj, conditioner rows untouched)"""
        y, l, same = xs_val, torch.zeros(xs_val.shape[1], dtype=dt, device="cuda"), True
        for k in reversed(range(len(layers))):
            y2, lk = nf.with_logabsdet_jacobian(nf.layer(flow, k), y)
            rows = torch.tensor(layers[k].idx_c, device="cuda")
            same = same and torch.equal(y2[rows].contiguous().view(torch.int64 if f64 else torch.int32),
                                        y[rows].contiguous().view(torch.int64 if f64 else torch.int32))
            y, l = y2, l + lk
        return y, l, same

    if "fwd" in parts:
        ys, ladj = nf.with_logabsdet_jacobian(flow.transform, xs_val)
        # parity.elementwise adds CFLOOR x the float32 oracle's WORST error on the array to every element's tolerance: the 1e3 / 1e-3
        # column's floor would license errors of 1e-3 ... 0.5 on the moderate columns.  So the moderate columns go through the
        # criterion with the floor of their own columns, and so does every extreme column of ys (d elements each).  ladj has ONE
        # element per column, and a one-element floor is a single draw of float32 rounding (over 120 such checks the device and the
        # float32 oracle both read 0.03 x the tolerance in the median, 1.15 and 0.56 at most): the four extreme ladj go together.
        extreme = np.isin(b.roles_val, FWD_EXTREME)
        ysn, ladjn = ys.cpu().numpy(), ladj.cpu().numpy()
        for gname, m in [("", ~extreme)] + [(f" ({role} column)", b.roles_val == role) for role in FWD_EXTREME]:
            chk("elementwise", key + "ys" + gname, ysn[:, m], r64["ys"][:, m], floor=None if f64 else r32["ys"][:, m], **ew)
        for gname, m in (("", ~extreme), (" (extreme columns)", extreme)):
            chk("elementwise", key + "ladj" + gname, ladjn[m], r64["ladj"][m], floor=None if f64 else r32["ladj"][m], **ew)
        chk.exact(key + "forward: each coupling returns its conditioner rows bit-identical", chain_by_layer()[2])
    if "inv" in parts:
        xr, lb = nf.with_logabsdet_jacobian(nf.inverse(flow.transform), _cm(torch, b.ys_inv, dt))
        chk("elementwise", key + "inverse x", xr, r64["x_inv"], floor=fl("x_inv"), **ew)
        chk("elementwise", key + "inverse ladj", lb, r64["ladj_inv"], floor=fl("ladj_inv"), **ew)
    if "layer" in parts:
        ys, ladj = nf.with_logabsdet_jacobian(flow.transform, xs_val)
        y2, l2, _ = chain_by_layer()
        for name, whole, chained in (("ys", ys, y2), ("ladj", ladj, l2)):  # the distance, for the record, before the criterion
            diff = (whole.double() - chained.double()).abs() / (ew["atol"] + ew["rtol"] * whole.double().abs())
            P.record(key + f"nf_layer_apply chained against the whole map: {name} [elementwise diff / (atol + rtol|whole|)]", float(diff.max()))
        chk.exact(key + "nf_layer_apply chained equals the whole map: ys", torch.equal(ys, y2))
        chk.exact(key + "nf_layer_apply chained equals the whole map: ladj", torch.equal(ladj, l2))
    if any(p in parts for p in ("elbo", "elbo_default", "elbo_stashed", "elbo_recompute")):
        # elbo: the default pass and, on the NetGeo shapes, the stashed and the recompute pass; elbo_default / _stashed / _recompute: that one
        netgeo = shape_of(c) in NETGEO
        budgets = ()
        if "elbo" in parts or "elbo_default" in parts:
            budgets += (("", None),)
        if ("elbo" in parts or "elbo_stashed" in parts) and netgeo:
            budgets += ((" (stashed pass)", 1 << 32),)
        if ("elbo" in parts or "elbo_recompute" in parts) and netgeo:
            budgets += ((" (recompute pass)", 0),)
        try:
            for name, budget in budgets:
                if budget is not None:
                    nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, budget))
                loss, g = nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs_grad)
                chk("scalar", key + "ELBO loss" + name, loss, r64["elbo_loss"], lr)
                chk("gradient", key + "ELBO grad" + name, g, r64["elbo_grad"], gr, floor=fl("elbo_grad"))
                if c.zero:
                    zero_bias_report(chk, key + "ELBO grad" + name, c, g, r64["elbo_grad"])
        finally:
            if any(bud is not None for _, bud in budgets):
                nf._lib.check(lib.nf_ctx_set_stash_budget(ctx.ptr, -1))
    if "elbo_rng" in parts:  # in-library draws: the fused forward (k_affine_chain / k_affine_chain_tgt on the NetGeo shapes)
        x2 = nf.device_specific_rand(nf.PhiloxRNG(3), flow.dist, n, dtype=dt).cpu().numpy().astype(np.float64)
        targets = [("diaggauss", tgt, otgt)]
        if shape_of(c) in NETGEO:  # the fused target forward
            targets.append(("banana", nf.BananaTarget(c.d, 0.1, 4.0), ("banana", 0.1, 4.0)))
        for tname, dtgt, ot in targets:
            l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, dtgt, n, rng=nf.PhiloxRNG(3))
            lr2, gr2 = o.neg_elbo_value_and_grad(b.spec, b.th, ot, x2)
            g32 = None if f64 else o.neg_elbo_value_and_grad(b.spec, *P.f32(b.th, ot, x2))[1]
            chk("scalar", key + f"ELBO loss (in-library draws, {tname})", l2, lr2, lr)
            chk("gradient", key + f"ELBO grad (in-library draws, {tname})", g2, gr2, gr, floor=g32)
            if c.zero:
                zero_bias_report(chk, key + f"ELBO grad (in-library draws, {tname})", c, g2, gr2)
    if "tape" in parts:  # nf_flow_fwd_keep + nf_flow_bwd_kept
        _, pullback = nf.flows.rrule_with_logabsdet_jacobian(flow.transform, xs_grad)
        xbar, g = pullback(_cm(torch, b.ybar, dt), torch.tensor(b.lbar, dtype=dt, device="cuda"))
        chk("gradient", key + "pullback gtheta", g, r64["tape_grad"], gr, floor=fl("tape_grad"))
        chk("gradient", key + "pullback xbar", xbar, r64["tape_xbar"], gr, floor=fl("tape_xbar"))
    if "step" in parts:  # nf_elbo_step (draw, forward, reverse, Adam, norm in one call) against the split calls
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        th_a, th_b = flow.theta.clone(), flow.theta.clone()
        ma, va, mb, vb = (torch.zeros_like(th_a) for _ in range(4))
        out, gn = torch.empty(flow.P + 1, dtype=dt, device="cuda"), torch.empty(1, dtype=dt, device="cuda")
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_a), vp(ma), vp(va), n, 77, 0, 1e-3, 0.9, 0.999,
                                       1e-8, C.byref(loss), C.byref(gnorm)))
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, 77, 0, 0, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, 1 if f64 else 0, vp(th_b), vp(out), vp(mb), vp(vb), flow.P, 1e-3, 0.9, 0.999, 1e-8, 1, vp(gn)))
        torch.cuda.synchronize()
        chk("scalar", key + "nf_elbo_step loss against the split calls", loss.value, float(out[flow.P]), 1e-6)
        chk("scalar", key + "nf_elbo_step |g| against the split calls", gnorm.value, float(gn), 1e-6)
        # Adam's first moment after one step is (1 - beta1) g: the two forms run the same kernels and differ at most in the
        # order of the slab sums, so a tenth of the parity tolerance is generous (tests/spline_cases.py)
        chk("gradient", key + "nf_elbo_step first moment against the split calls", ma, mb, 0.1 * gr)
    if "fkl" in parts:
        l3, g3 = nf.loglikelihood_value_and_gradient(flow, _cm(torch, b.ys_fkl, dt))
        chk("scalar", key + "forward-KL loss", l3, r64["fkl_loss"], 10 * lr)
        chk("gradient", key + "forward-KL grad", g3, r64["fkl_grad"], gr, floor=fl("fkl_grad"))
    return chk


def zero_bias_report(chk, key, c, g, gref):
    """the ZERO_UNITS' bias entries on their own: worst |got / ref| ratio's distance from 1 (a sign-bit slope reads 99)"""
    idx = zero_bias_index(c)
    got = g.detach().cpu().numpy().astype(np.float64)[idx] if hasattr(g, "detach") else np.asarray(g, dtype=np.float64)[idx]
    chk.P.record(key + ": zero-unit bias entries [max |got / ref - 1|]", float(np.abs(got / gref[idx] - 1.0).max()))
