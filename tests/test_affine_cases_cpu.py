"""The RealNVP cases of tests/affine_cases.py, held to the conditions that keep the GPU tests from hiding a failure (oracle only).

tests/test_gpu_affine_regimes.py accepts CFLOOR x the float32 oracle's own error on top of the plain element-wise tolerance and
holds every gradient to the plain GRAD_RTOL.  Both are only tests while the float32 oracle is itself close to the float64 one
and no single column or near-kink unit decides the outcome.  So the caps below are conditions on the INPUTS; if a seed or a
column breaks one, the seed or the column changes (affine_cases.SEED_SALT), not the cap.  Every test prints what it measured.

The -3 and +3 units.  With full Glorot rows they do not keep one sign over the batch: a row of fan-in 32 (d = 64) has |w| ~ 0.14 per
entry, inputs of scale 2 -- and the second coupling sees the first one's outputs, |y| up to ~ 10 -- spread the pre-activation by 1.6
and more around a bias of 3, and a third to a half of those units crossed 0 on some column whatever the seed.  So the CASE changed,
not the condition: their weight rows are affine_cases.HELD_ROW_SCALE x the Glorot draw, and test_profiles_reach_their_regimes
asserts that EVERY -3 unit stays in the leaky arm and EVERY +3 unit stays on for the whole gradient batch, in every hidden layer of
both nets of both couplings.

One condition could not be written the way it was first stated, for a reason that is arithmetic, not a seed: "the zero units' bias
entries are at least 100 GRAD_RTOL |g|inf".  Such an entry is 0.01 x the unit's summed cotangent, so it reaches 1e-2 |g|inf only if
that cotangent sum alone equals the largest entry of the whole gradient, and the outgoing weights stay as drawn.  What the check needs
is that the sign-bit rule cannot pass: it returns 100 x the entry, an error of 99 |entry|.  The test requires of EVERY one of the
twelve bias entries that this error alone is at least 2 GRAD_RTOL |g|inf, and of the units' weight rows (all-zero weights, non-zero
gradient: the larger part of what the sign-bit rule gets wrong) that their largest entry's error is at least the bound first stated,
100 GRAD_RTOL |g|inf; it prints both ranges.
"""
import numpy as np
import pytest

import affine_cases as A
import nf_oracle as o
import parity as P

FLOOR_CAP = 64.0                       # tests/test_spline_cases_cpu.py's: float32-oracle error / (Y_ATOL + Y_RTOL |ref|), every element
GRAD_FLOOR_CAP = P.GRAD_RTOL / P.CFLOOR  # float32-oracle gradient error / |g|inf: under it, parity.gradient's bound IS GRAD_RTOL
KINK_MARGIN = 5e-5                     # tests/test_gpu_cotangent_carry.py's 1e-5, widened for a fan-in of 136
EXTREME_FORWARD_COLUMNS = ("zero", "pm30", "tiny", "mixed")

CASES = A.ALL_CASES + A.ZERO_CASES
IDS = [A.case_name(c).replace(" ", "_") for c in CASES]


def _ratio(got, ref):
    return np.abs(got.astype(np.float64) - ref) / (P.Y_ATOL + P.Y_RTOL * np.abs(ref))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_outputs_are_finite_and_the_float32_floors_are_capped(c):
    b, r = A.build(c), A.reference(c)
    for prec in ("f64", "f32"):
        for name, a in r[prec].items():
            assert np.all(np.isfinite(a)), (prec, name)
    r64, r32 = r["f64"], r["f32"]
    mod = ~np.isin(b.roles_val, EXTREME_FORWARD_COLUMNS)
    for name in ("ys", "ladj", "x_inv", "ladj_inv"):
        rt = _ratio(r32[name], r64[name])
        extra = f" (moderate columns {float(rt[..., mod].max()):.2f})" if name in ("ys", "ladj") else ""
        print(f"{A.case_name(c)}: {name} float32-oracle floor {float(rt.max()):.2f} x the plain tolerance{extra}")
        assert rt.max() <= FLOOR_CAP, (name, float(rt.max()))
    for name in ("elbo_grad", "fkl_grad", "tape_grad", "tape_xbar"):
        ref = r64[name]
        ferr = float(np.abs(r32[name].astype(np.float64) - ref).max() / np.abs(ref).max())
        print(f"{A.case_name(c)}: {name} float32-oracle floor {ferr:.2e} of |g|inf")
        assert ferr <= GRAD_FLOOR_CAP, (name, ferr)


REC_CASES = [c for c in CASES if A.shape_of(c) in A.RECOMPUTES]


@pytest.mark.parametrize("c", REC_CASES, ids=[A.case_name(c).replace(" ", "_") for c in REC_CASES])
def test_the_reconstruct_by_inversion_floor_is_capped(c):
    """The shapes whose reverse pass can rebuild the layer inputs by inverting the chain (nf_deep.hip always, the NetGeo kernels under
    nf_ctx_set_stash_budget(0)): the float32 oracle doing the same, with the forward output moved in its last bit six ways, stays
    under the cap, so that pass too is held to the plain GRAD_RTOL."""
    b, r = A.build(c), A.reference(c)
    g = r["f64"]["elbo_grad"]
    tgt = ("diaggauss", b.mu, b.var)
    errs = [float(np.abs(A.fp32_recompute_floor(b.spec, b.th, tgt, b.xs_grad, s) - g).max() / np.abs(g).max()) for s in [None] + list(range(6))]
    print(f"{A.case_name(c)}: reconstruct-by-inversion floor {errs[0]:.2e} of |g|inf, worst of six jitters {max(errs):.2e}")
    assert max(errs) <= GRAD_FLOOR_CAP, errs


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gradient_sets_stay_off_the_kinks_and_no_column_dominates(c):
    b, r = A.build(c), A.reference(c)
    n = b.xs_grad.shape[1]
    assert b.xs_grad.shape == (c.d, A.N_GRAD) and b.ys_fkl.shape == b.xs_grad.shape
    near = A.min_abs_preact(c, b.th, b.xs_grad)
    pre, _ = o.flow_inv(b.spec, b.th, b.ys_fkl)  # the pre-image of the forward-KL data, after their rounding to float32
    near_fkl = A.min_abs_preact(c, b.th, pre)
    print(f"{A.case_name(c)}: smallest |hidden pre-activation| {near.min():.2e} (gradient set), {near_fkl.min():.2e} (forward-KL pre-image)")
    assert near.min() >= KINK_MARGIN and near_fkl.min() >= KINK_MARGIN
    # no extreme column: the three scales only, nothing beyond 5 sigma of the widest
    assert np.abs(b.xs_grad).max() <= 10.0 and sorted(set(b.scale_grad)) == [0.3, 1.0, 2.0]
    tgt = ("diaggauss", b.mu, b.var)
    ginf = float(np.abs(r["f64"]["elbo_grad"]).max())
    col = max(float(np.abs(o.neg_elbo_value_and_grad(b.spec, b.th, tgt, b.xs_grad[:, j:j + 1])[1]).max()) for j in range(n))
    print(f"{A.case_name(c)}: n |g|inf / largest single-column gradient = {n * ginf / col:.2f}")
    assert col / n <= 0.5 * ginf, (col / n, ginf)


def _s_rows(b, xs):
    """per coupling (flat order): pre-tanh z and s = tanh(z) of the oracle's forward pass on xs, (transformed dimensions, n)"""
    _, _, states = o.flow_fwd(b.spec, b.th, xs, keep=True)
    layers = o.layers_flat_order(b.spec)
    out = {}
    for ci, x in zip(range(len(layers) - 1, -1, -1), states):
        li = layers[ci]
        out[ci] = (o.mlp_forward(b.th, li.nets[0], x[li.idx_c], None), o.mlp_forward(b.th, li.nets[0], x[li.idx_c], "tanh"), li)
    return out


@pytest.mark.parametrize("c", A.ALL_CASES, ids=[A.case_name(c).replace(" ", "_") for c in A.ALL_CASES])
def test_profiles_reach_their_regimes(c):
    b = A.build(c)
    assert b.xs_val.shape == (c.d, A.N_VAL) and b.ys_inv.shape == (c.d, A.N_VAL - len(A.EXTREME))
    with np.errstate(all="ignore"):
        rows = _s_rows(b, b.xs_val)
    nt = sum(len(li.idx_t) for _, _, li in rows.values())
    used = {A.profile_of(ci, t) for ci, (_, _, li) in rows.items() for t in range(len(li.idx_t))}
    if min(len(li.idx_t) for _, _, li in rows.values()) >= 5:
        assert used == set(A.PROFILES), used
    clamp_seen = []
    for ci in sorted(rows):
        z, s, li = rows[ci]
        _, b_off, nout, _ = li.nets[0][-1]
        zb = b.th[b_off:b_off + nout]
        for t in range(nout):
            p = A.profile_of(ci, t)
            if c.gain == 0:  # fully prescribed: the same for every sample, tanh of the profile
                assert np.all(z[t] == zb[t]) and np.all(s[t] == np.tanh(zb[t])), (ci, t, p)
                if p in ("sat+", "sat-"):
                    assert np.all(np.abs(s[t]) > 0.99) and np.all(np.sign(s[t]) == (1 if p == "sat+" else -1))
            else:  # sample-dependent on top (measured before the tanh: a row may saturate for the whole batch at gain = 1 too)
                assert np.ptp(z[t][np.isfinite(z[t])]) > 1e-3, (ci, t, p)
            if p == "clamp":
                clamp_seen.append(float(zb[t]))
                assert (zb[t] ** 2 < 66.0) == (abs(zb[t]) == 8.0) and abs(zb[t]) in (8.0, 8.25, 9.0)
            if p == "zero":
                assert zb[t] == 0.0
    # both sides of nf_tanh's clamp in every shape with two clamp dimensions (d >= 6 has them), in turn
    assert clamp_seen == [A.CLAMP_Z[k % len(A.CLAMP_Z)] for k in range(len(clamp_seen))]
    assert len(clamp_seen) >= 2 and min(v * v for v in clamp_seen) < 66.0 < max(v * v for v in clamp_seen), clamp_seen
    # hidden biases: -3, +3, 0 on every 8th unit; EVERY -3 / +3 unit keeps its sign over the whole gradient batch
    held = np.zeros(2, dtype=int)
    total = np.zeros(2, dtype=int)
    for li in o.layers_flat_order(b.spec):
        for net in li.nets:
            for (_, b_off, nout, _) in net[:-1]:
                hb = b.th[b_off:b_off + nout]
                assert np.all(hb[0::8] == -3.0) and np.all(hb[1::8] == 3.0) and np.all(hb[2::8] == 0.0)
    for _, _, _, z in A.hidden_preacts(b.spec, b.th, b.xs_grad):
        held += ((z[0::8] < 0).all(axis=1).sum(), (z[1::8] > 0).all(axis=1).sum())
        total += (len(z[0::8]), len(z[1::8]))
    print(f"{A.case_name(c)}: {nt} transformed dimensions, clamp z {clamp_seen}; units that keep their sign over the gradient batch: "
          f"{held[0]} of {total[0]} at -3, {held[1]} of {total[1]} at +3")
    assert held[0] == total[0] and held[1] == total[1], (held, total)
    # float32-representable throughout: the float32 oracle and the device see the float64 oracle's numbers
    for a in (b.th, b.xs_val, b.ys_inv, b.xs_grad, b.ys_fkl, b.ybar, b.lbar, b.mu, b.var):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


def test_profiles_shift_by_one_per_coupling_and_gain_zero_differs_only_in_w_out():
    assert A.profile_of(1, 0) == A.profile_of(0, 1)
    for shape in A.SHAPES:
        t0, t1 = A.theta(A.case(shape, 0)), A.theta(A.case(shape, 1))
        diff = np.flatnonzero(t0 != t1)
        w_out = np.concatenate([np.arange(li.nets[0][-1][0], li.nets[0][-1][1]) for li in o.layers_flat_order(A.spec_of(A.case(shape, 0)))])
        assert np.all(np.isin(diff, w_out)) and np.all(t0[w_out] == 0.0)


@pytest.mark.parametrize("c", A.ZERO_CASES, ids=[A.case_name(c).replace(" ", "_") for c in A.ZERO_CASES])
def test_zero_units_sit_exactly_on_the_kink_and_their_gradient_cannot_be_missed(c):
    b, r = A.build(c), A.reference(c)
    for prec, dt in (("f64", np.float64), ("f32", np.float32)):
        for _, _, l, z in A.hidden_preacts(b.spec, b.th.astype(dt), b.xs_grad.astype(dt)):
            if l == 0:  # +0 for every sample, in every precision (not -0: the sign bit is clear)
                zz = z[list(A.ZERO_UNITS)]
                assert np.all(zz == 0.0) and not np.any(np.signbit(zz)), prec
    # their outgoing weights stay: the reference differentiates these units with slope 0.01 and the entries are not 0
    g = r["f64"]["elbo_grad"]
    idx = A.zero_bias_index(c)
    assert len(idx) == 12
    ginf = float(np.abs(g).max())
    err_if_slope_1 = 99.0 * np.abs(g[idx])  # what a kernel that differentiates +0 with slope 1 is off by, entry by entry
    print(f"{A.case_name(c)}: zero-unit bias entries {np.abs(g[idx]).min() / ginf:.2e} ... {np.abs(g[idx]).max() / ginf:.2e} of |g|inf; "
          f"a slope of 1 there is off by {err_if_slope_1.min() / (P.GRAD_RTOL * ginf):.1f} ... {err_if_slope_1.max() / (P.GRAD_RTOL * ginf):.1f} x GRAD_RTOL |g|inf")
    assert err_if_slope_1.min() >= 2.0 * P.GRAD_RTOL * ginf
    werr = 99.0 * np.abs(g[A.zero_weight_index(c)])  # the same for the units' weight rows: zero weights, non-zero gradient
    print(f"{A.case_name(c)}: zero-unit weight-row entries up to {werr.max() / 99.0 / ginf:.2e} of |g|inf; a slope of 1 there is off by up to "
          f"{werr.max() / (P.GRAD_RTOL * ginf):.0f} x GRAD_RTOL |g|inf")
    assert werr.max() >= 100.0 * P.GRAD_RTOL * ginf
