"""The planar / radial cases of tests/simple_cases.py, held to the conditions that keep the GPU tests from hiding a failure (oracle only).

tests/test_gpu_simple_regimes.py accepts CFLOOR x the float32 oracle's own error on top of the plain tolerances.  That is only a test
while the float32 oracle is itself close to the float64 one: the planar map at full randn parameters is not (its float32 oracle is
42 x the element-wise tolerance off at d = 33 x 10, 1160 x at d = 200 x 30, its inverse 2e4 x at d = 64 x 16), which is why the cases
prescribe w'u, |w| and b per layer and keep |w'u| <= 3 in every chain that is inverted or differentiated.  The caps below are
conditions on the CASES; if a seed breaks one, the seed changes (simple_cases.SEED_SALT), not the cap.  Every test prints what it
measured.

Two things changed under these conditions that are not seeds (simple_cases' docstring has the figures): the radial theta[1] cycle is
entered at its last element (8, 0, -5, 4, -2, 1), because entered at 0 it reaches 8 only at the sixth layer and the shapes of three
and four layers cannot realise beta-hat > 5; and the radial layers are counted in the order they are applied, so that the
first-applied layer, which the near-centre gradient columns sit on, is (0, 8) in every shape and not the nearly singular (3, -5).
"""
import numpy as np
import pytest

import nf_oracle as o
import parity as P
import simple_cases as S

MODERATE_FLOOR_CAP = 3.0                  # float32-oracle error / (Y_ATOL + Y_RTOL |ref|) on the moderate columns, every element
GRAD_FLOOR_CAP = 1e-5                     # ELBO / pullback: float32-oracle gradient error / |g|inf
FKL_FLOOR_CAP = P.GRAD_RTOL / P.CFLOOR    # forward-KL: under it, parity.gradient's bound IS GRAD_RTOL
FKL_DROP_CAP = 0.05

CHAIN = S.CHAIN_CASES + S.SWITCH_ONLY_CASES  # the switch rows' own shape is held to every condition of the table's
IDS = [S.case_id(c) for c in CHAIN]
EDGE_IDS = [S.case_id(c) for c in S.EDGE_CASES]


def _ratio(got, ref):
    return np.abs(got.astype(np.float64) - ref) / (P.Y_ATOL + P.Y_RTOL * np.abs(ref))


@pytest.mark.parametrize("c", CHAIN, ids=IDS)
def test_oracle_outputs_are_finite_and_the_float32_floors_are_capped(c):
    b, r = S.build(c), S.reference(c)
    for prec in ("f64", "f32"):
        for name, a in r[prec].items():
            assert np.all(np.isfinite(a)), (prec, name)
    r64, r32 = r["f64"], r["f32"]
    for name, roles, extreme in (("ys", b.roles_val, S.FWD_EXTREME), ("ladj", b.roles_val, S.FWD_EXTREME),
                                 ("x_inv", b.roles_inv, S.INV_EXTREME), ("ladj_inv", b.roles_inv, S.INV_EXTREME)):
        rt = _ratio(r32[name], r64[name])
        mod = ~np.isin(roles, extreme)
        print(f"{S.case_name(c)}: {name} float32-oracle floor {float(rt[..., mod].max()):.2f} x the plain tolerance on the moderate columns, "
              f"{float(rt[..., ~mod].max()):.2f} on the extreme ones")
        assert rt[..., mod].max() <= MODERATE_FLOOR_CAP, (name, float(rt[..., mod].max()))
    for name in ("elbo_grad", "tape_grad", "tape_xbar"):
        ref = r64[name]
        ferr = float(np.abs(r32[name].astype(np.float64) - ref).max() / np.abs(ref).max())
        print(f"{S.case_name(c)}: {name} float32-oracle floor {ferr:.2e} of |g|inf")
        assert ferr <= GRAD_FLOOR_CAP, (name, ferr)
    ref = r64["fkl_grad"]
    ferr = float(np.abs(r32["fkl_grad"].astype(np.float64) - ref).max() / np.abs(ref).max())
    print(f"{S.case_name(c)}: fkl_grad float32-oracle floor {b.fkl_floor_full:.2e} of |g|inf on the full set, {ferr:.2e} after the drop rule "
          f"({b.fkl_dropped} of {b.n_fkl_full} columns dropped)")
    assert ferr <= FKL_FLOOR_CAP, ferr
    assert b.fkl_dropped <= FKL_DROP_CAP * b.n_fkl_full, (b.fkl_dropped, b.n_fkl_full)
    assert b.ys_fkl.shape == (S.d_of(c), b.n_fkl_full - b.fkl_dropped)


@pytest.mark.parametrize("c", CHAIN, ids=IDS)
def test_input_sets_have_their_columns(c):
    b = S.build(c)
    d = S.d_of(c)
    assert b.xs_val.shape == (d, S.N_VAL) and list(b.roles_val[-4:]) == ["zero", "pm30", "tiny", "centre"]
    assert [int((b.roles_val == f"n{s:g}").sum()) for s in (0.3, 1.0, 2.0, 4.0)] == [17] * 4
    assert b.ys_inv.shape == (d, S.N_VAL - len(S.EXTREME)) and not np.isin(b.roles_inv, S.EXTREME).any()
    assert np.all(b.xs_val[:, b.roles_val == "zero"] == 0.0) and np.all(np.abs(b.xs_val[:, b.roles_val == "pm30"]) == 30.0)
    assert 0 < np.abs(b.xs_val[:, b.roles_val == "tiny"]).max() < 1e-19
    assert b.xs_grad.shape == (d, S.N_GRAD) and [int((b.scale_grad == s).sum()) for s in (0.3, 1.0, 2.0)] == [24] * 3
    assert b.n_fkl_full == S.N_GRAD - int(b.near_grad.sum())
    # cotangents: one sign per feature, a negative lbar
    assert np.all(np.sign(b.ybar) == np.where(np.arange(d) % 2 == 0, 1.0, -1.0)[:, None]) and np.all(b.lbar < 0)
    # float32-representable throughout: the float32 oracle and the device see the float64 oracle's numbers
    for a in (b.th, b.xs_val, b.ys_inv, b.xs_grad, b.ys_fkl, b.ybar, b.lbar, b.mu, b.var):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    # the centre column sits exactly at the first-applied layer's centre, in float32 as in float64
    centre = b.xs_val[:, b.roles_val == "centre"]
    p = S.layer_params(c, b.th)[-1]
    if c.kind == "radial":
        assert np.array_equal(centre[:, 0], p[2])
        assert int(b.near_grad.sum()) == S.N_NEAR
        r_first = np.sqrt(((b.xs_grad - p[2][:, None]) ** 2).sum(axis=0))
        print(f"{S.case_name(c)}: first-applied layer's r on the gradient set: {r_first[b.near_grad].min():.2e} ... {r_first[b.near_grad].max():.2e} "
              f"(near-centre columns), at least {r_first[~b.near_grad].min():.2e} elsewhere")
        assert r_first.min() > 0 and r_first[b.near_grad].max() < 1e-3 * 6 * np.sqrt(d)
        # no column at exactly r = 0 in ANY layer: the reference's AD does not define the gradient there
        _, _, states = o.flow_fwd(b.spec, b.th, b.xs_grad, keep=True)
        for (alpha, bhat, z0), x in zip(reversed(S.layer_params(c, b.th)), states):
            assert np.sqrt(((x - z0[:, None]) ** 2).sum(axis=0)).min() > 0
    else:
        w, _, bb = p
        print(f"{S.case_name(c)}: first-applied layer's w'z + b on the centre column: {float(w @ centre[:, 0] + bb):.2e}")
        assert abs(w @ centre[:, 0] + bb) < 1e-6 and not b.near_grad.any()


PLANAR = [c for c in CHAIN if c.kind == "planar"]
RADIAL = [c for c in CHAIN if c.kind == "radial"]


@pytest.mark.parametrize("c", [c for c in CHAIN if c.shape in ("f32_d2x3", "f64_d5x12", "f32_d33x10", "f32_d64x12")], ids=S.case_id)
def test_per_column_forward_kl_gradients_sum_to_the_oracles(c):
    """The drop rule ranks columns by simple_cases.per_column_fkl_grads, the oracle's forward-KL reverse pass taken column by column
    through its internals: the columns must sum to o.neg_loglik_value_and_grad's gradient, or the rule selects by something else."""
    b = S.build(c)
    ys = b.ys_fkl[:, :12]
    g = o.neg_loglik_value_and_grad(b.spec, b.th, ys)[1]
    G = S.per_column_fkl_grads(b.spec, b.th, ys)
    err = float(np.abs(G.sum(axis=0) - g).max() / np.abs(g).max())
    print(f"{S.case_name(c)}: |sum of the per-column gradients - the oracle's| = {err:.1e} of |g|inf")
    assert G.shape == (ys.shape[1], b.th.shape[0]) and err <= 1e-12


@pytest.mark.parametrize("c", PLANAR, ids=[S.case_id(c) for c in PLANAR])
def test_planar_layers_realise_their_profile_and_span_the_tanh_regimes(c):
    b = S.build(c)
    params = S.layer_params(c, b.th)
    worst = 0.0
    for k, (w, u, bb) in enumerate(params):
        sw, bp, m = S.profile_of(c, k)
        worst = max(worst, abs(w @ u - m))
        assert abs(w @ u) <= 3.0 + 1e-6, (k, w @ u)
        assert abs(w @ u - m) <= 1e-6, (k, w @ u, m)
        assert abs(np.linalg.norm(w) - sw) <= 1e-6 * sw and bb == bp
    # the whole profile is used where the chain is long enough
    assert {S.profile_of(c, k)[0] for k in range(len(params))} == set(S.SW)
    # the value set's moderate columns reach the linear and the saturated tanh
    mod = ~np.isin(b.roles_val, S.FWD_EXTREME)
    _, _, states = o.flow_fwd(b.spec, b.th, b.xs_val[:, mod], keep=True)
    a = np.array([np.abs(w @ x + bb) for (w, _, bb), x in zip(reversed(params), states)])
    print(f"{S.case_name(c)}: |w'u - profile| <= {worst:.1e}; |w'z + b| on the moderate columns from {a.min():.2e} to {a.max():.1f}")
    assert a.min() < 0.1 and a.max() > 6.0


@pytest.mark.parametrize("c", RADIAL, ids=[S.case_id(c) for c in RADIAL])
def test_radial_layers_reach_small_and_large_alpha_and_beta_hat(c):
    b = S.build(c)
    params = S.layer_params(c, b.th)
    alpha = np.array([p[0] for p in params])
    bhat = np.array([p[1] for p in params])
    print(f"{S.case_name(c)}: alpha {alpha.min():.4f} ... {alpha.max():.3f}; beta-hat + alpha at least {(bhat + alpha).min():.4f}; beta-hat up to {bhat.max():.2f}")
    assert alpha.min() < 0.05 and alpha.max() > 3.0 and (bhat + alpha).min() < 0.01 and bhat.max() > 5.0
    assert np.all(bhat + alpha > 0)  # the layer is invertible
    for k, li in enumerate(o.layers_flat_order(b.spec)):
        p0, p1, zs = S.profile_of(c, k)
        assert b.th[li.offset] == p0 and b.th[li.offset + 1] == p1


@pytest.mark.parametrize("c", S.EDGE_CASES, ids=EDGE_IDS)
def test_edge_cases_are_finite_in_float64_and_realise_their_extremes(c):
    """Forward only.  The float32 oracle's own ladj cancels at 1 + c ~ 0 (log1p(c sech^2)): its floor is printed, not capped -- the
    device check records both figures, and where the device beats the float32 oracle the table shows it."""
    b, r = S.build(c), S.reference(c)
    assert S.nl_of(c) == S.EDGE_NL and b.xs_val.shape == (S.d_of(c), S.N_VAL)
    assert np.all(np.isfinite(r["f64"]["ys"])) and np.all(np.isfinite(r["f64"]["ladj"]))
    mod = ~np.isin(b.roles_val, S.FWD_EXTREME)
    fy, fl = _ratio(r["f32"]["ys"], r["f64"]["ys"]), _ratio(r["f32"]["ladj"], r["f64"]["ladj"])
    print(f"{S.case_name(c)}: float32-oracle floor on the moderate columns: ys {np.nanmax(fy[:, mod]):.2f}, ladj {np.nanmax(fl[mod]):.2f} x the plain tolerance")
    params = S.layer_params(c, b.th)
    if c.kind == "planar":
        ms = np.array([w @ u for w, u, _ in reversed(params)])  # in the order of application
        # LOOSER than the chain cases' 1e-6: the profile to 1e-6 |m| / 3, i.e. 4e-6 at m = +-12 and 1e-5 at m = +-30 -- u is rounded
        # to float32 and m = 30 carries ten times the rounding of m = 3.  The chain cases (|m| <= 3) are held to 1e-6 itself.
        assert np.all(np.abs(ms - np.array(S.EDGE_M)) <= 1e-6 * np.abs(np.array(S.EDGE_M)) / 3.0), ms
        onepc = o.softplus(ms)  # 1 + c
        print(f"{S.case_name(c)}: 1 + c from {onepc.min():.1e} to {onepc.max():.1f}")
        assert onepc.min() < 1e-12 and 1e-6 < sorted(onepc)[1] < 1e-5 and onepc.max() > 29.0
    else:
        assert [(b.th[li.offset], b.th[li.offset + 1]) for li in reversed(o.layers_flat_order(b.spec))] == list(S.EDGE_R)  # in the order of application
        assert all(p[0] + p[1] > 0 for p in params)


EXTREME_ULP_CAP = 0.5  # x the plain tolerance
MODERATE_ULP_CAP = 3.0  # the cap of the float32-oracle floor on the chain cases' moderate columns


@pytest.mark.parametrize("c", CHAIN + S.EDGE_CASES, ids=IDS + EDGE_IDS)
def test_extreme_columns_are_not_decided_by_one_ulp_of_their_inputs(c):
    """The extreme columns' ladj is ONE element per column, so its float32-oracle floor is a single draw of float32 rounding and the
    device check on it is, in effect, the plain tolerance.  That is only a test where float32 can reach the plain tolerance at all:
    moving theta and the inputs by one float32 ulp (eight draws, float64 oracle) must move each extreme column's ladj by at most half
    of it.  The moderate columns (68 elements, a floor that is a maximum over many draws) are held to what the chain cases'
    float32-oracle floor is held to, 3 x: beyond it the error of any float32 code is an amplified rounding that scales as
    1 / |w'z + b| on a nearly singular layer, and the largest of 68 such draws of one code says little about another's.  With the
    planar edge layers counted by flat index this read up to 18.6 x (d = 2) and 3.2 x on an extreme column (d = 9), which is why
    they are counted in the order of application."""
    b = S.build(c)
    w = S.ulp_response(c)
    ext = np.isin(b.roles_val, S.FWD_EXTREME)
    print(f"{S.case_name(c)}: one ulp on the inputs moves ladj by {np.round(w[ext], 2)} x the plain tolerance on the extreme columns, "
          f"up to {w[~ext].max():.2f} x on the moderate ones")
    assert w[ext].max() <= EXTREME_ULP_CAP, (list(b.roles_val[ext]), w[ext])
    assert w[~ext].max() <= MODERATE_ULP_CAP, float(w[~ext].max())


# ---- the shape table against a model of nf_simple.hip's host side -----------------------------------------------------------------
def _dpl_for(d):
    need, dpl = (d + 15) // 16, 1
    while dpl < need:
        dpl *= 2
    return dpl


def _vec_ok(d, es):
    dpl = _dpl_for(d)
    vw = 16 // es if dpl * es >= 16 else dpl
    return vw > 1 and d % vw == 0


def _train_path(kind, dtype, d, nl, tile=True):
    f32 = dtype == "float32"
    if tile and kind == "planar" and f32 and 2 <= d <= 64 and 1 <= nl <= 16:
        return "planar_step", (1 + (d > 32), 6 if nl <= 10 else 8)
    if tile and kind == "radial" and f32 and 8 <= d <= 64 and 1 <= nl <= 16:
        return "radial_step", (1 + (d > 32), 10 if nl <= 10 else 16)
    budget = (64 if f32 else 32) // _dpl_for(d)
    nlmax = 12 if budget >= 12 else 10 if budget >= 10 else 4 if budget >= 4 else 0
    if nl > nlmax:
        return "split", None
    return "simple_step", (_dpl_for(d), 4 if nl <= 4 else 10 if nl <= 10 else 12)


EXPECT = {  # shape -> (DPL, vector rows, planar path, radial path)
    "f32_d2x3": (1, False, ("planar_step", (1, 6)), ("simple_step", (1, 4))),
    "f32_d9x11": (1, False, ("planar_step", (1, 8)), ("radial_step", (1, 16))),
    "f32_d31x10": (2, False, ("planar_step", (1, 6)), ("radial_step", (1, 10))),
    "f32_d33x10": (4, False, ("planar_step", (2, 6)), ("radial_step", (2, 10))),
    "f32_d64x16": (4, True, ("planar_step", (2, 8)), ("radial_step", (2, 16))),
    "f32_d100x4": (8, True, ("simple_step", (8, 4)), ("simple_step", (8, 4))),
    "f32_d130x4": (16, False, ("simple_step", (16, 4)), ("simple_step", (16, 4))),
    "f32_d200x30": (16, True, ("split", None), ("split", None)),
    "f64_d2x10": (1, False, ("simple_step", (1, 10)), ("simple_step", (1, 10))),
    "f64_d5x12": (1, False, ("simple_step", (1, 12)), ("simple_step", (1, 12))),
    "f64_d20x3": (2, True, ("simple_step", (2, 4)), ("simple_step", (2, 4))),
    "f64_d33x4": (4, False, ("simple_step", (4, 4)), ("simple_step", (4, 4))),
    "f64_d100x4": (8, True, ("simple_step", (8, 4)), ("simple_step", (8, 4))),
    "f64_d64x10": (4, True, ("split", None), ("split", None)),
}


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_shapes_reach_the_paths_the_table_names(shape):
    """dpl_for, vec_ok, planar_mfma_ok, radial_lane_ok, step_bound, step_nlmax and nf_simple_step_supported, modelled here line by line:
    each shape reaches the DPL, the row form and the training kernel its row names, every DPL occurs in both element types that have it,
    and f32 d130 x 4 sits AT its layer budget."""
    dtype, d, nl = S.SHAPES[shape]
    es = 4 if dtype == "float32" else 8
    dpl, vec, planar, radial = EXPECT[shape]
    assert (_dpl_for(d), _vec_ok(d, es)) == (dpl, vec)
    assert _train_path("planar", dtype, d, nl) == planar and _train_path("radial", dtype, d, nl) == radial
    assert S.TRAIN[("planar", shape)] == planar[0] and S.TRAIN[("radial", shape)] == radial[0]
    # the edge cases (nl = 4) keep the shape's DPL and row form: only the forward kernel runs there
    assert S.nl_of(S.case("planar", shape, True)) == 4


def test_the_shape_table_covers_every_apply_instantiation_and_row_form():
    f32 = {(EXPECT[s][0], EXPECT[s][1]) for s in S.SHAPES if s.startswith("f32")}
    f64 = {(EXPECT[s][0], EXPECT[s][1]) for s in S.SHAPES if s.startswith("f64")}
    assert {dpl for dpl, _ in f32} == {1, 2, 4, 8, 16} and {dpl for dpl, _ in f64} == {1, 2, 4, 8}
    assert {(4, True), (4, False), (16, True), (16, False)} <= f32 and {(4, True), (4, False)} <= f64
    # f32 d130 x 4: 4 layers == the budget of 64 / 16 registers
    assert _train_path("planar", "float32", 130, 5)[0] == "split" and _train_path("planar", "float32", 130, 4)[0] == "simple_step"
    assert {S.expected_launches(t)["elbo"][t if t != "split" else "simple_bwd"] for t in ("split", "simple_step", "planar_step", "radial_step")} == {1}


def test_switch_rows_land_where_the_host_code_sends_them():
    """NF_PLANAR_NO_MFMA / NF_RADIAL_NO_LANE: d = 33 x 10 and d = 9 x 11 run k_simple_step, d = 64 x 16 is beyond step_nlmax (12) and splits"""
    for kind in S.KINDS:
        assert _train_path(kind, "float32", 33, 10, tile=False) == ("simple_step", (4, 10))
        assert _train_path(kind, "float32", 9, 11, tile=False) == ("simple_step", (1, 12))
        assert _train_path(kind, "float32", 64, 16, tile=False) == ("split", None)
        assert _train_path(kind, "float32", 64, 12, tile=False) == ("simple_step", (4, 12)) and _vec_ok(64, 4)
        assert _train_path(kind, "float32", 64, 13, tile=False) == ("split", None)  # 12 is the last fused depth
    for shape, train in S.SWITCH_TRAIN.items():
        assert _train_path("planar", *S.ALL_SHAPES[shape], tile=False)[0] == train
    for c in S.SWITCH_ONLY_CASES:  # by default the switch rows' own shape is served by the tile kernels, as simple_cases.TRAIN says
        assert _train_path(c.kind, *S.ALL_SHAPES[c.shape])[0] == S.TRAIN[(c.kind, c.shape)] == c.kind + "_step"
