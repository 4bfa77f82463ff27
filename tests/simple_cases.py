"""Planar and radial cases away from the 0.3 x randn initialisation: prescribed w'u, |w|, b (planar) and alpha, beta-hat, z0 (radial).

A plain module (no pytest, no torch at import), importable from a child process: tests/test_simple_cases_cpu.py holds the cases
to the conditions that keep a parity check meaningful, tests/test_gpu_simple_regimes.py runs them on the device -- in process,
and once per environment switch in a child process.

Flows are FlowSpec("planar" | "radial", d, nl).  Flat layer k = 0 is the outermost (applied last); the first-applied layer is the
last in flat order.  Everything (theta, inputs, target parameters, cotangents) is rounded to float32-representable values, for
the Float64 cases too, so the float32 oracle and the device see the float64 oracle's numbers.

Planar, per flat layer k, three settings cycled independently:
  |w|     from SW = (1, 0.3, 3): with N(0, I) inputs w'z + b covers the linear, the moderate and the saturated tanh
  b       from B = (0, 2, -2, 0.5)
  m = w'u from M = (-3, 0.75, 0, -0.75, 0.25, -0.125, 1.5, -0.25, 0.125, -1.5, 3, 0.5): c = w'u_hat = softplus(m) - 1 from -0.95
          to 2.05.  u = perp + m w / |w|^2 with perp = 0.5 / sqrt(d) randn made orthogonal to w.
  |m| <= 3 in every chain that is inverted or differentiated: at full randn parameters the float32 ORACLE's own inverse is 2e4 x
  the element-wise tolerance off at d = 64 x 16 and its forward 1160 x at d = 200 x 30 -- a floor that would license any kernel.

Radial, per layer j COUNTED IN THE ORDER OF APPLICATION (j = nl - 1 - k of flat layer k):
  theta[0] from P0 = (0, -4, 3, 1, -1.5): alpha = softplus from 0.018 to 3.05
  theta[1] from P1 = (0, -5, 4, -2, 1, 8), ENTERED AT ITS LAST ELEMENT (8, 0, -5, 4, -2, 1, 8, ...): softplus from 0.0067 to 8, beta-hat
           = softplus(theta[1]) - alpha from just above -alpha to about 8.  Entered at 0 the cycle reaches 8 only at k = 5, and the
           shapes of three and four layers could not realise beta-hat > 5 (a condition of the CPU test); entered at 8 the first
           three layers are (0, 8), (-4, 0), (3, -5): alpha < 0.05, alpha > 3, beta-hat + alpha < 0.01 and beta-hat > 5 all occur.
           Counted by flat index the first-applied layer of a three-layer flow is (3, -5): beta-hat + alpha = 0.0067, and on the
           near-centre columns (r ~ 1e-3) 1 + beta-hat h = (alpha + beta-hat + r) / (alpha + r) cancels -- the float32 ORACLE's ELBO
           gradient was 1.4e-5 of |g|inf off (d = 2 x 3; cap 1e-5).  Counted in the order of application the first-applied layer is
           always (0, 8).
  z0       randn x 0.5 on odd j, x 0.05 on even j

Edge cases (`edge=True`: forward checks only, the same shapes with nl = 4):
  planar   m = (-12, 12, -30, 30) IN THE ORDER OF APPLICATION: 1 + c from 6e-6 down to 9e-14, c up to 29.  The centre column puts t = 0
           on the m = -12 layer, ladj = log(1 + c) = -12.  Counted by flat index the layers with |u_hat| = 30 and 12 came first and the
           nearly singular ones, which return log(t^2), saw states of magnitude 30: one float32 ulp on theta and the inputs moved ladj
           by up to 18.6 x the plain tolerance on a moderate column and 3.2 x on the all-zero column (float64 oracle alone,
           ulp_response below) -- errors that scale as 1 / |w'z + b|, heavy-tailed, where the largest of 68 draws of one float32
           code is not within 3 x of another's and a one-element floor is a single lucky or unlucky draw (the float32 oracle read
           0.38 x on that all-zero column, and 7.45 x on the centre column of d = 130).  In the order of application the response
           is at most 2.4 x and 0.5 x.  The device keeps softplus(w'u) and evaluates
           log(sp sech^2 + t^2); the float32 oracle's log1p(c sech^2) cancels there.  Both figures are recorded.
  radial   (theta[0], theta[1]) = (-12, -12), (8, 12), (-12, 12), (8, -12)

Inputs.
  value set     72 columns: 17 columns of N(0, 1) at each of the scales 0.3, 1, 2 and 4 | one all-zero column | one of +-30 | one of
                1e-20 N(0, 1) | one "centre" column: radial, exactly z0 of the first-applied layer (r = 0); planar, -b w / |w|^2 of the
                first-applied layer (t = 0)
  inverse set   the float32-rounded float64-oracle image of the value set without the +-30 and 1e-20 columns, compared against
                o.flow_inv (not as a round trip)
  gradient set  72 columns, 24 at each of the scales 0.3, 1 and 2; radial: the last four of the scale-0.3 block sit at z0 + 1e-3 randn
                of the first-applied layer.  No column at exactly r = 0: the reference's AD does not define the gradient there.
  forward-KL    the float32-rounded oracle image of the gradient set without the near-centre columns, less the columns whose
                single-column gradient, float32 oracle against float64 oracle, differs by more than FKL_DROP of the batch's |g|inf
                (the rule of test_general_mvnormal_base for splines)
  tape          the gradient set with cotangents of one sign per feature (|N(0, 1)| / n, alternating by feature) and a negative lbar
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
from affine_cases import Checks, _cm  # noqa: E402,F401

Case = namedtuple("Case", "kind shape edge")
KINDS = ("planar", "radial")
SW = (1.0, 0.3, 3.0)
B = (0.0, 2.0, -2.0, 0.5)
M = (-3.0, 0.75, 0.0, -0.75, 0.25, -0.125, 1.5, -0.25, 0.125, -1.5, 3.0, 0.5)
EDGE_M = (-12.0, 12.0, -30.0, 30.0)
P0 = (0.0, -4.0, 3.0, 1.0, -1.5)
P1 = (0.0, -5.0, 4.0, -2.0, 1.0, 8.0)
P1_ENTRY = 5  # the cycle is entered at its last element (module docstring)
EDGE_R = ((-12.0, -12.0), (8.0, 12.0), (-12.0, 12.0), (8.0, -12.0))
EDGE_NL = 4
N_VAL, N_GRAD, N_NEAR = 72, 72, 4
EXTREME = ("pm30", "tiny")                        # roles of the value-set columns the inverse set leaves out
FWD_EXTREME = ("zero", "pm30", "tiny", "centre")  # ... and those the forward checks take one by one
INV_EXTREME = ("zero", "centre")
FKL_DROP = 1e-5

# shape -> (dtype, d, nl).  What each reaches, read off nf_simple.hip's host side:
#   dpl_for(d)      = ceil(d / 16) rounded up to a power of two (16 lanes per sample)
#   vec_ok<T>       vector width vw = 4 (float, DPL >= 4), 2 (float DPL 2; double, DPL >= 2), 1 (DPL 1): vector rows iff vw > 1 and d % vw == 0
#   planar_mfma_ok  float32, 2 <= d <= 64, nl <= 16 -> k_planar_step, PlanarGeo<DB = 1 + (d > 32), 6 (nl <= 10) | 8>
#   radial_lane_ok  float32, 8 <= d <= 64, nl <= 16 -> k_radial_step, RadialGeo<DB, 10 (nl <= 10) | 16>
#   step_nlmax      budget = (64 float | 32 double) / DPL layers held in registers -> 12 / 10 / 4 / 0; step_bound(nl) = 4 | 10 | 12
#   nf_simple_step_supported: a tile kernel, or nl <= step_nlmax (and the caches fit LDS); otherwise the split sequence
#                   simple_apply (stashing) + simple_bwd + simple_finalize
# The smallest shape per path: one row for every features-per-lane instantiation, row form and training kernel.
SHAPES = {
    "f32_d2x3": ("float32", 2, 3),        # DPL 1 (vw 1: element-wise).  planar: PlanarGeo<1,6>; radial (d < 8): k_simple_step<float,1,.,4> (budget 64, bound 4)
    "f32_d9x11": ("float32", 9, 11),      # DPL 1.  more than ten layers: PlanarGeo<1,8>, RadialGeo<1,16>
    "f32_d31x10": ("float32", 31, 10),    # DPL 2 (need 2), vw 2, 31 odd: element-wise rows.  one feature block, <= 10 layers: <1,6>, <1,10>
    "f32_d33x10": ("float32", 33, 10),    # DPL 4 (need 3), vw 4, 33 % 4 = 1: element-wise rows.  d > 32: two feature blocks, the second holds one row
    "f32_d64x16": ("float32", 64, 16),    # DPL 4, vector rows.  two full blocks, 16 layers: PlanarGeo<2,8>, RadialGeo<2,16>
    "f32_d100x4": ("float32", 100, 4),    # DPL 8 (need 7), vw 4, 100 % 4 = 0: vector rows.  d > 64: k_simple_step<float,8,.,4> (budget 8 -> 4 layers)
    "f32_d130x4": ("float32", 130, 4),    # DPL 16 (need 9), 130 % 4 = 2: element-wise rows.  k_simple_step<float,16,.,4>, AT its budget 64 / 16 = 4
    "f32_d200x30": ("float32", 200, 30),  # DPL 16 (need 13), vector rows.  30 > 4 layers: simple_apply (stash) + simple_bwd + simple_finalize
    "f64_d2x10": ("float64", 2, 10),      # DPL 1.  k_simple_step<double,1,.,10> (budget 32 -> 12, bound 10)
    "f64_d5x12": ("float64", 5, 12),      # DPL 1.  bound 12, the cap of step_nlmax
    "f64_d20x3": ("float64", 20, 3),      # DPL 2, vw 2, vector rows (pairs).  budget 16 -> 12, bound 4
    "f64_d33x4": ("float64", 33, 4),      # DPL 4, vw 2, 33 odd: element-wise rows.  budget 8 -> 4, bound 4
    "f64_d100x4": ("float64", 100, 4),    # DPL 8, vector rows.  budget 32 / 8 = 4, bound 4
    "f64_d64x10": ("float64", 64, 10),    # DPL 4, vector rows.  10 > budget 8 -> 4: the split sequence
}
# profiler name (nf_prof_read) of the ELBO value-and-gradient's main launch, per kind; "split" = simple_apply + simple_bwd
_TILE = ("f32_d9x11", "f32_d31x10", "f32_d33x10", "f32_d64x16")
_SPLIT = ("f32_d200x30", "f64_d64x10")
TRAIN = {
    ("planar", s): "split" if s in _SPLIT else "planar_step" if s in _TILE + ("f32_d2x3",) else "simple_step" for s in SHAPES
}
TRAIN.update({("radial", s): "split" if s in _SPLIT else "radial_step" if s in _TILE else "simple_step" for s in SHAPES})
# the same under NF_PLANAR_NO_MFMA / NF_RADIAL_NO_LANE, for the shapes of the switch rows: without a tile kernel d = 64 x 16 has DPL 4, a
# budget of 16 layers that step_nlmax rounds down to 12, and 16 layers exceed it.  d = 64 x 12 stands next to it for what the row was
# after: k_simple_step<float, 4, ., 12> with vector rows, AT step_nlmax.  It is a shape of the switch rows only (by default it lands
# on the tile kernels of d = 64 x 16), held to the same CPU conditions as the table's shapes.
SWITCH_SHAPES = {"f32_d64x12": ("float32", 64, 12)}
SWITCH_TRAIN = {"f32_d9x11": "simple_step", "f32_d33x10": "simple_step", "f32_d64x16": "split", "f32_d64x12": "simple_step"}
TRAIN.update({("planar", "f32_d64x12"): "planar_step", ("radial", "f32_d64x12"): "radial_step"})
ALL_SHAPES = {**SHAPES, **SWITCH_SHAPES}
PROF_NAMES = ("simple_apply", "simple_bwd", "simple_finalize", "simple_step", "planar_step", "radial_step", "simple_epilogue")


def case(kind, shape, edge=False):
    return Case(kind, shape, edge)


CHAIN_CASES = [case(k, s) for k in KINDS for s in SHAPES]
SWITCH_ONLY_CASES = [case(k, s) for k in KINDS for s in SWITCH_SHAPES]
EDGE_CASES = [case(k, s, True) for k in KINDS for s in SHAPES]


def dtype_of(c):
    return ALL_SHAPES[c.shape][0]


def d_of(c):
    return ALL_SHAPES[c.shape][1]


def nl_of(c):
    return EDGE_NL if c.edge else ALL_SHAPES[c.shape][2]


def case_name(c):
    return f"{c.kind} {c.shape}" + (" edge x4" if c.edge else "")


def case_id(c):
    return case_name(c).replace(" ", "_")


def spec_of(c):
    return o.FlowSpec(c.kind, d_of(c), nl_of(c))


def step_supported(c):
    return TRAIN[(c.kind, c.shape)] != "split"


def _f32r(a):
    """float64 array of float32-representable values"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# Seeds changed under the conditions of tests/test_simple_cases_cpu.py (measured with the oracle alone), by case name:
#   planar f32_d64x16   salt 0: float32-oracle forward-KL floor 3.9e-5 of |g|inf on the full set, 4 of 72 columns over FKL_DROP (cap: 3)
#   planar f32_d200x30  salt 0: float32-oracle inverse x 3.46 x and inverse ladj 4.62 x the plain tolerance on the moderate columns (cap: 3)
#   planar f32_d9x11 edge x4  salt 0: one float32 ulp on theta moves the ladj of the all-zero and the 1e-20 column by 0.64 x the plain tolerance (cap: 0.5)
SEED_SALT = {"planar f32_d64x16": 1, "planar f32_d200x30": 2, "planar f32_d9x11 edge x4": 1}


def _seed(c):
    return 1000 * d_of(c) + nl_of(c) + (0 if c.kind == "planar" else 500) + (250 if c.edge else 0) + SEED_SALT.get(case_name(c), 0)


def profile_of(c, k):
    """what flat layer k is prescribed: planar (|w|, b, m), radial (theta[0], theta[1], z0 scale)"""
    if c.kind == "planar":
        # edge: m in the order of application, the first-applied layer has m = -12 (module docstring)
        return SW[k % len(SW)], B[k % len(B)], (EDGE_M[(nl_of(c) - 1 - k) % len(EDGE_M)] if c.edge else M[k % len(M)])
    j = nl_of(c) - 1 - k  # radial layers are counted in the order they are applied (module docstring)
    p0, p1 = EDGE_R[j % len(EDGE_R)] if c.edge else (P0[j % len(P0)], P1[(j + P1_ENTRY) % len(P1)])
    return p0, p1, (0.5 if j % 2 else 0.05)


def theta(c):
    spec, d = spec_of(c), d_of(c)
    rng = np.random.default_rng(_seed(c))
    th = np.zeros(o.param_count(spec))
    for k, li in enumerate(o.layers_flat_order(spec)):
        if c.kind == "planar":
            sw, b, m = profile_of(c, k)
            w = rng.standard_normal(d)
            w = _f32r(w * sw / np.linalg.norm(w))
            perp = rng.standard_normal(d) * 0.5 / np.sqrt(d)
            perp -= (perp @ w) / (w @ w) * w
            th[li.offset:li.offset + d] = w
            th[li.offset + d:li.offset + 2 * d] = perp + m * w / (w @ w)
            th[li.offset + 2 * d] = b
        else:
            p0, p1, zs = profile_of(c, k)
            th[li.offset], th[li.offset + 1] = p0, p1
            th[li.offset + 2:li.offset + 2 + d] = rng.standard_normal(d) * zs
    return _f32r(th)


def layer_params(c, th):
    """per flat layer: planar (w, u, b), radial (alpha, beta-hat, z0)"""
    d, out = d_of(c), []
    for li in o.layers_flat_order(spec_of(c)):
        p = th[li.offset:li.offset + li.nparams]
        if c.kind == "planar":
            out.append((p[:d], p[d:2 * d], p[2 * d]))
        else:
            alpha = o.softplus(p[0])
            out.append((alpha, o.softplus(p[1]) - alpha, p[2:2 + d]))
    return out


def centre_of(c, th):
    """the input at which the first-applied layer sits at its centre: radial z0 (r = 0), planar -b w / |w|^2 (w'z + b = 0)"""
    p = layer_params(c, th)[-1]
    if c.kind == "radial":
        return p[2].copy()
    w, _, b = p
    return -b * w / (w @ w)


def _value_set(c, th, rng):
    d = d_of(c)
    cols, roles = [], []
    for s in (0.3, 1.0, 2.0, 4.0):
        cols.append(s * rng.standard_normal((d, 17)))
        roles += [f"n{s:g}"] * 17
    cols.append(np.zeros((d, 1)))
    cols.append(30.0 * np.where(rng.uniform(size=(d, 1)) < 0.5, -1.0, 1.0))
    cols.append(1e-20 * rng.standard_normal((d, 1)))
    cols.append(centre_of(c, th)[:, None])
    roles += ["zero", "pm30", "tiny", "centre"]
    return _f32r(np.concatenate(cols, axis=1)), np.array(roles)


def _grad_set(c, th, rng):
    d = d_of(c)
    scale = np.repeat([0.3, 1.0, 2.0], N_GRAD // 3)
    xs = rng.standard_normal((d, N_GRAD)) * scale[None, :]
    near = np.zeros(N_GRAD, dtype=bool)
    if c.kind == "radial":
        near[N_GRAD // 3 - N_NEAR:N_GRAD // 3] = True
        xs[:, near] = centre_of(c, th)[:, None] + 1e-3 * rng.standard_normal((d, N_NEAR))
    return _f32r(xs), scale, near


def per_column_fkl_grads(spec, th, ys):
    """(n, P): column j's share of o.neg_loglik_value_and_grad(spec, th, ys)[1], by the oracle's own steps -- the batched inverse and
    the batched implicit-function solve of _layer_inv_bwd, which are per column anyway, and the layer's reverse pass column by column
    where the oracle sums over the batch"""
    n = ys.shape[1]
    z, _ = o.flow_inv(spec, th, ys)
    a, cc = z / n, np.full(n, -1.0 / n, dtype=ys.dtype)
    G = np.zeros((n, th.shape[0]), dtype=th.dtype)
    w = z
    for li in reversed(o.layers_flat_order(spec)):
        vbar = o._layer_inv_bwd(spec, th, li, w, a, cc, np.zeros_like(th))
        for j in range(n):
            o._layer_bwd(spec, th, li, w[:, j:j + 1], -vbar[:, j:j + 1], -cc[j:j + 1], G[j])
        a = vbar
        w, _ = o._layer_fwd(spec, th, li, w)
    return G


def _fkl_set(c, spec, th, ys):
    """ys less the columns the drop rule removes; (kept ys, number dropped, float32-oracle floor of the full set / |g|inf)"""
    f = np.float32
    with np.errstate(all="ignore"):
        G64 = per_column_fkl_grads(spec, th, ys)
        G32 = per_column_fkl_grads(spec, th.astype(f), ys.astype(f)).astype(np.float64)
    g64 = G64.sum(axis=0)
    gs = float(np.abs(g64).max())
    keep = np.abs(G32 - G64).max(axis=1) / gs <= FKL_DROP
    return np.ascontiguousarray(ys[:, keep]), int((~keep).sum()), float(np.abs(G32.sum(axis=0) - g64).max() / gs)


Built = namedtuple("Built", "case spec th xs_val roles_val ys_inv roles_inv xs_grad scale_grad near_grad ys_fkl n_fkl_full fkl_dropped "
                            "fkl_floor_full ybar lbar mu var")


@functools.lru_cache(maxsize=None)
def build(c):
    spec, th, d = spec_of(c), theta(c), d_of(c)
    rng = np.random.default_rng(_seed(c) + 1)
    xs_val, roles_val = _value_set(c, th, rng)
    if c.edge:
        for a in (th, xs_val):
            a.setflags(write=False)
        return Built(c, spec, th, xs_val, roles_val, *([None] * 13))
    inv_cols = ~np.isin(roles_val, EXTREME)
    with np.errstate(all="ignore"):
        ys_inv = _f32r(o.flow_fwd(spec, th, xs_val[:, inv_cols])[0])
    xs_grad, scale_grad, near_grad = _grad_set(c, th, rng)
    ys_full = _f32r(o.flow_fwd(spec, th, xs_grad[:, ~near_grad])[0])
    ys_fkl, dropped, floor_full = _fkl_set(c, spec, th, ys_full)
    mu, var = _f32r(rng.standard_normal(d)), _f32r(rng.uniform(size=d) + 0.5)
    sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)[:, None]
    ybar = _f32r(sign * np.abs(rng.standard_normal((d, N_GRAD))) / N_GRAD)
    lbar = _f32r(-(0.5 + rng.uniform(size=N_GRAD)) / N_GRAD)
    for a in (th, xs_val, ys_inv, xs_grad, ys_fkl, ybar, lbar, mu, var):
        a.setflags(write=False)
    return Built(c, spec, th, xs_val, roles_val, ys_inv, roles_val[inv_cols], xs_grad, scale_grad, near_grad, ys_fkl, ys_full.shape[1], dropped,
                 floor_full, ybar, lbar, mu, var)


def _oracle(b, dt):
    th = b.th.astype(dt)
    r = {}
    r["ys"], r["ladj"] = o.flow_fwd(b.spec, th, b.xs_val.astype(dt))
    if b.case.edge:
        return r
    tgt = ("diaggauss", b.mu.astype(dt), b.var.astype(dt))
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


def ulp_response(c, draws=8):
    """per value-set column: the largest |change of the float64 oracle's ladj| / (Y_ATOL + Y_RTOL |ladj|) when theta and the inputs
    move by one float32 ulp (relative 2^-24 U(-1, 1), `draws` times) -- what ANY float32 evaluation is off by at the least"""
    b, ref = build(c), reference(c)["f64"]["ladj"]
    rng = np.random.default_rng(12345)
    worst = np.zeros_like(ref)
    with np.errstate(all="ignore"):
        for _ in range(draws):
            th = b.th * (1.0 + 2.0 ** -24 * rng.uniform(-1, 1, b.th.shape))
            xs = b.xs_val * (1.0 + 2.0 ** -24 * rng.uniform(-1, 1, b.xs_val.shape))
            worst = np.maximum(worst, np.abs(o.flow_fwd(b.spec, th, xs)[1] - ref) / (1e-6 + 1e-5 * np.abs(ref)))
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# the device checks of one case (tests/test_gpu_simple_regimes.py: in process, and in a child process per switch)
# ----------------------------------------------------------------------------------------------------------------------
ALL_PARTS = ("fwd", "inv", "layer", "rand", "elbo", "tape", "step", "fkl")
SEED_RNG, SEED_STEP, SEED_RAND = 3, 77, 21
DRAW_ATOL = {"float32": 3e-6, "float64": 1e-13}  # the base sampler against o.base_sample, as test_gpu_parity.py holds it


def parts_of(c, layer=True):
    if c.edge:
        return ("fwd", "layer") if layer else ("fwd",)
    return tuple(p for p in ALL_PARTS if (p != "step" or step_supported(c)) and (p != "layer" or layer))


def targets_of(nf, c, b, torch, dt):
    """[(name, device target, oracle target)]: the diagonal Gaussian on every shape, Banana and Funnel where d <= 64 (the
    cross-feature terms of target_term, the DIAG = false instantiations of the tile kernels), WarpedGauss and Cross at d = 2"""
    d = d_of(c)
    out = [("diaggauss", nf.DiagGaussTarget(torch.tensor(b.mu, dtype=dt, device="cuda"), torch.tensor(b.var, dtype=dt, device="cuda")),
            ("diaggauss", b.mu, b.var))]
    if d <= 64:
        out.append(("banana", nf.BananaTarget(d, 0.3, 4.0), ("banana", 0.3, 4.0)))
        out.append(("funnel", nf.FunnelTarget(d, -1.0, 1.5), ("funnel", -1.0, 1.5)))
    if d == 2:
        out.append(("warped", nf.WarpedGaussTarget(1.0, 0.12), ("warped", 1.0, 0.12)))
        out.append(("cross", nf.CrossTarget(2.0, 0.15), ("cross", 2.0, 0.15)))
    return out


def make_flow(nf, c, torch):
    b = build(c)
    dt = torch.float64 if dtype_of(c) == "float64" else torch.float32
    flow = nf.Flow(c.kind, nf.MvNormal(d_of(c)), nl_of(c), dtype=dt, device="cuda", theta=torch.tensor(b.th, dtype=dt, device="cuda"))
    return flow, dt


def launched(nf, flow, run):
    """{profiler name: launches} of PROF_NAMES while `run()` executes"""
    import ctypes as C

    import torch

    lib, ctx = nf.load_library(), flow.ctx
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


def dispatch(nf, c):
    """launch counts of one forward, and of one ELBO value-and-gradient (supplied draws), of case c"""
    import torch

    b = build(c)
    flow, dt = make_flow(nf, c, torch)
    tgt = targets_of(nf, c, b, torch, dt)[0][1]
    xs_val, xs_grad = _cm(torch, b.xs_val, dt), _cm(torch, b.xs_grad, dt)
    fwd = launched(nf, flow, lambda: nf.with_logabsdet_jacobian(flow.transform, xs_val))
    vg = launched(nf, flow, lambda: nf.value_and_gradient(nf.elbo_batch, flow, tgt, xs_grad))
    return {"fwd": fwd, "elbo": vg}


def expected_launches(train):
    """what dispatch() must read for a shape whose training path is `train` (a profiler name, or "split"), and nothing else"""
    zero = dict.fromkeys(PROF_NAMES, 0)
    fwd = dict(zero, simple_apply=1)
    if train == "split":
        vg = dict(zero, simple_apply=1, simple_bwd=1, simple_finalize=1)
    else:
        vg = dict(zero, simple_finalize=1)
        vg[train] = 1
    return {"fwd": fwd, "elbo": vg}


def device_checks(nf, c, parts=ALL_PARTS, chk=None, tag=""):
    """Run `parts` of case c on the device against the oracle; returns the Checks (figures in parity.MEASURED under
    'simple regimes: ...', failures in .failed)."""
    import ctypes as C

    import torch

    chk = chk or Checks()
    P = chk.P
    b, r = build(c), reference(c)
    r64, r32 = r["f64"], r["f32"]
    f64 = dtype_of(c) == "float64"
    key = f"simple regimes: {tag}{case_name(c)}: "
    ew = dict(rtol=P.F64_RTOL, atol=1e-12) if f64 else dict(rtol=P.Y_RTOL, atol=P.Y_ATOL)
    lr = P.F64_RTOL if f64 else P.LOSS_RTOL
    gr = P.F64_GRAD if f64 else P.GRAD_RTOL
    fl = (lambda name: None) if f64 else (lambda name: r32[name])  # Float64: no floor
    flow, dt = make_flow(nf, c, torch)
    bits = torch.int64 if f64 else torch.int32
    nl, d = nl_of(c), d_of(c)
    lib, ctx = nf.load_library(), flow.ctx
    xs_val = _cm(torch, b.xs_val, dt)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def same(a, bb):
        return torch.equal(a.contiguous().view(bits), bb.contiguous().view(bits))

    def by_role(name, got, ref, floor, roles, extreme):
        """parity.elementwise adds CFLOOR x the float32 oracle's WORST error on the array to every element's tolerance, so the
        moderate columns go through the criterion with the floor of their own columns and every extreme column of a (d, n) array
        on its own (d elements each).  A per-sample array has ONE element per column and a one-element floor is a single draw of
        float32 rounding: tests/test_simple_cases_cpu.py requires of the extreme columns that one float32 ulp on their inputs moves ladj
        by at most half the plain tolerance, and they go one role at a time as well."""
        got = got.detach().cpu().numpy()
        ext = np.isin(roles, extreme)
        groups = [("", ~ext)] + [(f" ({role} column)", roles == role) for role in extreme]
        for gname, m in groups:
            chk("elementwise", key + name + gname, got[..., m], ref[..., m], floor=None if floor is None else floor[..., m], **ew)

    if "fwd" in parts:
        ys, ladj = nf.with_logabsdet_jacobian(flow.transform, xs_val)
        by_role("ys", ys, r64["ys"], fl("ys"), b.roles_val, FWD_EXTREME)
        by_role("ladj", ladj, r64["ladj"], fl("ladj"), b.roles_val, FWD_EXTREME)
    if "inv" in parts:
        xr, lb = nf.with_logabsdet_jacobian(nf.inverse(flow.transform), _cm(torch, b.ys_inv, dt))
        by_role("inverse x", xr, r64["x_inv"], fl("x_inv"), b.roles_inv, INV_EXTREME)
        by_role("inverse ladj", lb, r64["ladj_inv"], fl("ladj_inv"), b.roles_inv, INV_EXTREME)
    if "layer" in parts:  # one kernel runs both forms, so any difference is a finding
        runs = [("", flow.transform, xs_val, reversed(range(nl)), False)]
        if not c.edge:
            runs.append((" (inverse)", nf.inverse(flow.transform), _cm(torch, b.ys_inv, dt), range(nl), True))
        for dname, whole_t, x_in, order, inv in runs:
            whole, lw = nf.with_logabsdet_jacobian(whole_t, x_in)
            y, l = x_in, torch.zeros(x_in.shape[1], dtype=dt, device="cuda")
            for k in order:
                t = nf.layer(flow, k)
                y, lk = nf.with_logabsdet_jacobian(nf.inverse(t) if inv else t, y)
                l = l + lk
            for name, a, bb in (("ys", whole, y), ("ladj", lw, l)):  # the distance, for the record, before the criterion
                diff = (a.double() - bb.double()).abs() / (ew["atol"] + ew["rtol"] * a.double().abs())
                diff = diff[torch.isfinite(diff)]
                P.record(key + f"nf_layer_apply chained against the whole map{dname}: {name} [elementwise diff / (atol + rtol|whole|)]",
                         float(diff.max()) if diff.numel() else 0.0)
                chk.exact(key + f"nf_layer_apply chained equals the whole map{dname}: {name}", same(a, bb))
    if "rand" in parts:
        n = N_GRAD
        ys = nf.rand(flow, n, nf.PhiloxRNG(SEED_RAND))
        xs = nf.device_specific_rand(nf.PhiloxRNG(SEED_RAND), flow.dist, n, dtype=dt)
        chk.exact(key + "nf_flow_rand equals nf_flow_fwd of nf_base_sample_logpdf's draws", same(ys, flow.transform(xs)))
        x_ref = o.base_sample(d, n, seed=SEED_RAND, sample_offset=0, stream=0, precision="f64" if f64 else "f32")
        y_ref = o.flow_fwd(b.spec, b.th, x_ref)[0]
        # the draws on their own, at the sampler's stated bound (test_base_sampler_matches_spec_and_is_shard_invariant: 3e-6 absolute
        # in Float32, Box-Muller round-off; 1e-13 in Float64) -- nothing of the device's draws enters the floor below
        draw_err = float(np.abs(xs.cpu().numpy().astype(np.float64) - x_ref).max())
        draw_tol = DRAW_ATOL["float64" if f64 else "float32"]
        P.record(key + "nf_base_sample_logpdf's draws against o.base_sample [max abs diff / sampler's bound]", draw_err / draw_tol)
        if not draw_err <= draw_tol:
            chk.failed.append(key + f"nf_base_sample_logpdf's draws are {draw_err:.3e} from o.base_sample's (bound {draw_tol:g})")
        # Float32: the floor is the float32 oracle on the float32-rounded ORACLE draws
        y32 = None if f64 else o.flow_fwd(b.spec, *P.f32(b.th, x_ref))[0]
        chk("elementwise", key + "nf_flow_rand against the oracle's image of the oracle's draws", ys, y_ref, floor=y32, **ew)
    if "elbo" in parts:
        n = N_GRAD
        xs_grad = _cm(torch, b.xs_grad, dt)
        tgts = targets_of(nf, c, b, torch, dt)
        loss, g = nf.value_and_gradient(nf.elbo_batch, flow, tgts[0][1], xs_grad)
        chk("scalar", key + "ELBO loss (gradient set)", loss, r64["elbo_loss"], lr, floor=fl("elbo_loss"))
        chk("gradient", key + "ELBO grad (gradient set)", g, r64["elbo_grad"], gr, floor=fl("elbo_grad"))
        x2 = nf.device_specific_rand(nf.PhiloxRNG(SEED_RNG), flow.dist, n, dtype=dt)  # the draws the in-library form regenerates
        x2n = x2.cpu().numpy().astype(np.float64)
        for tname, dtgt, ot in tgts:
            lo, go = o.neg_elbo_value_and_grad(b.spec, b.th, ot, x2n)
            l32, g32 = (None, None) if f64 else o.neg_elbo_value_and_grad(b.spec, *P.f32(b.th, ot, x2n))
            got = {}
            for form, arg in (("in-library draws", n), ("the same draws supplied", x2)):
                l2, g2 = nf.value_and_gradient(nf.elbo_batch, flow, dtgt, arg, rng=nf.PhiloxRNG(SEED_RNG))
                chk("scalar", key + f"ELBO loss ({form}, {tname})", l2, lo, lr, floor=l32)
                chk("gradient", key + f"ELBO grad ({form}, {tname})", g2, go, gr, floor=g32)
                got[form] = g2
            chk.exact(key + f"ELBO grad ({tname}): the two draw forms agree bit for bit", same(*got.values()))
    if "tape" in parts:  # nf_flow_fwd_keep + nf_flow_bwd_kept; then once more with xbar_out aliasing ybar, which the header allows
        n = N_GRAD
        xs_grad = _cm(torch, b.xs_grad, dt).t().contiguous()  # (n, d) row-major = d x n column-major
        nbytes = int(lib.nf_tape_bytes(ctx.ptr, C.byref(flow.desc), n))
        nf._lib.check(min(nbytes, 0))
        tape = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device="cuda")
        y, ladj = torch.empty_like(xs_grad), torch.empty(n, dtype=dt, device="cuda")
        nf._lib.check(lib.nf_flow_fwd_keep(ctx.ptr, C.byref(flow.desc), vp(flow.theta), vp(xs_grad), n, vp(y), vp(ladj), vp(tape), nbytes))
        ybar = _cm(torch, b.ybar, dt).t().contiguous()
        lbar = torch.tensor(b.lbar, dtype=dt, device="cuda")
        xbar, g = torch.empty_like(ybar), torch.empty(flow.P, dtype=dt, device="cuda")
        nf._lib.check(lib.nf_flow_bwd_kept(ctx.ptr, C.byref(flow.desc), vp(flow.theta), vp(tape), nbytes, vp(ybar), vp(lbar), n, vp(xbar), vp(g)))
        inplace, g2 = ybar.clone(), torch.empty_like(g)
        nf._lib.check(lib.nf_flow_bwd_kept(ctx.ptr, C.byref(flow.desc), vp(flow.theta), vp(tape), nbytes, vp(inplace), vp(lbar), n, vp(inplace), vp(g2)))
        torch.cuda.synchronize()
        chk("gradient", key + "pullback gtheta", g, r64["tape_grad"], gr, floor=fl("tape_grad"))
        chk("gradient", key + "pullback xbar", xbar.t(), r64["tape_xbar"], gr, floor=fl("tape_xbar"))
        chk.exact(key + "pullback with xbar_out aliasing ybar: gtheta bit for bit", same(g, g2))
        chk.exact(key + "pullback with xbar_out aliasing ybar: xbar bit for bit", same(xbar, inplace))
    if "step" in parts:  # nf_elbo_step (draw, chain, target, reverse, Adam, norm in one call) against the split calls
        n = N_GRAD
        tgt = targets_of(nf, c, b, torch, dt)[0][1]
        th_a, th_b = flow.theta.clone(), flow.theta.clone()
        ma, va, mb, vb = (torch.zeros_like(th_a) for _ in range(4))
        out, gn = torch.empty(flow.P + 1, dtype=dt, device="cuda"), torch.empty(1, dtype=dt, device="cuda")
        loss, gnorm = C.c_double(0), C.c_double(0)
        nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_a), vp(ma), vp(va), n, SEED_STEP, 0, 1e-3, 0.9, 0.999,
                                       1e-8, C.byref(loss), C.byref(gnorm)))
        nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th_b), None, n, n, SEED_STEP, 0, 0, vp(out)))
        nf._lib.check(lib.nf_adam_update(ctx.ptr, 1 if f64 else 0, vp(th_b), vp(out), vp(mb), vp(vb), flow.P, 1e-3, 0.9, 0.999, 1e-8, 1, vp(gn)))
        torch.cuda.synchronize()
        chk("scalar", key + "nf_elbo_step loss against the split calls", loss.value, float(out[flow.P]), 1e-6)
        chk("scalar", key + "nf_elbo_step |g| against the split calls", gnorm.value, float(gn), 1e-6)
        chk("gradient", key + "nf_elbo_step first moment against the split calls", ma, mb, 0.1 * gr)
    if "fkl" in parts:
        l3, g3 = nf.loglikelihood_value_and_gradient(flow, _cm(torch, b.ys_fkl, dt))
        chk("scalar", key + "forward-KL loss", l3, r64["fkl_loss"], 10 * lr, floor=fl("fkl_loss"))
        chk("gradient", key + "forward-KL grad", g3, r64["fkl_grad"], gr, floor=fl("fkl_grad"))
    return chk
