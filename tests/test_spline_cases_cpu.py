"""The spline cases of tests/spline_cases.py, held to the conditions that keep the GPU tests from hiding a failure (oracle only).

tests/test_gpu_spline_regimes.py accepts CFLOOR x the float32 oracle's own error on top of the plain tolerance.  That is only a
test while the float32 oracle is itself close to the float64 one: an ill-conditioned spline (a near-zero-width bin, a sample on a
knot in a gradient) would license any kernel.  So the caps below are conditions on the INPUTS; if a seed or profile breaks one,
the seed or the profile changes, not the cap.
"""
import numpy as np
import pytest

import nf_oracle as o
import parity as P
import spline_cases as S

FLOOR_CAP = 64.0      # float32-oracle error / (Y_ATOL + Y_RTOL |ref|), every element of y, ladj, inverse x, inverse ladj
GRAD_FLOOR_CAP = 3e-3  # float32-oracle gradient error / |g|inf

IDS = [S.case_name(c).replace(" ", "_") for c in S.ALL_CASES]


@pytest.mark.parametrize("c", S.ALL_CASES, ids=IDS)
def test_oracle_outputs_are_finite_and_the_float32_floor_is_capped(c):
    r = S.reference(c)
    for prec in ("f64", "f32"):
        for name, a in r[prec].items():
            assert np.all(np.isfinite(a)), (prec, name)
    r64, r32 = r["f64"], r["f32"]
    for name in ("ys", "ladj", "x_inv", "ladj_inv"):
        ref = r64[name]
        ratio = float((np.abs(r32[name].astype(np.float64) - ref) / (P.Y_ATOL + P.Y_RTOL * np.abs(ref))).max())
        print(f"{S.case_name(c)}: {name} float32-oracle floor {ratio:.2f} x the plain tolerance")
        assert ratio <= FLOOR_CAP, (name, ratio)
    for name in ("elbo_grad", "fkl_grad"):
        ref = r64[name]
        ferr = float(np.abs(r32[name].astype(np.float64) - ref).max() / np.abs(ref).max())
        print(f"{S.case_name(c)}: {name} float32-oracle floor {ferr:.2e} of |g|inf")
        assert ferr <= GRAD_FLOOR_CAP, (name, ferr)


F32_CASES = [c for c in S.ALL_CASES if c.dtype == "float32"]  # the cases whose GPU checks take a float32-oracle floor


@pytest.mark.parametrize("c", F32_CASES, ids=[S.case_name(c).replace(" ", "_") for c in F32_CASES])
def test_the_ladj_floor_does_not_rest_on_cancellation_between_couplings(c):
    """The floor handed to tests/parity.py is ONE float32 evaluation of the chain.  ladj is a sum over the couplings, and the second
    coupling's conditioner sees the first one's rounding error, so the float32 oracle's errors can cancel on a sensitive column (a
    column whose log-derivatives themselves cancel to ~ 0, where the tolerance is its absolute part) and the floor then licenses less
    than float32 arithmetic needs -- a correct kernel fails the rms criterion on such a case, on one column.  Condition on the
    inputs: the float32 oracle's error of EACH coupling, fed the float64 oracle's state, summed over the couplings without sign,
    must itself pass the rms criterion the GPU test applies with the chain's floor, max(1, CFLOOR x the floor's rms)."""
    b, r = S.build(c), S.reference(c)
    layers = o.layers_flat_order(b.spec)
    for name, x, order, f in (("ladj", b.xs_val, layers[::-1], o._layer_fwd), ("ladj_inv", b.ys_grid, layers, o._layer_inv)):
        ref = r["f64"][name]
        base = P.Y_ATOL + P.Y_RTOL * np.abs(ref)
        frms = float(np.sqrt(np.mean((np.abs(r["f32"][name].astype(np.float64) - ref) / base) ** 2)))
        tot = np.zeros(x.shape[1])
        for li in order:
            y64, l64 = f(b.spec, b.th, li, x)
            tot += np.abs(f(b.spec, b.th.astype(np.float32), li, x.astype(np.float32))[1].astype(np.float64) - l64)
            x = y64.astype(np.float32).astype(np.float64)
        rms = float(np.sqrt(np.mean((tot / base) ** 2)))
        print(f"{S.case_name(c)}: {name} float32 floor rms {frms:.2f}, per coupling without cancellation {rms:.2f}")
        assert rms <= max(1.0, P.CFLOOR * frms), (name, rms, frms)


def _bins(p, v):
    """bin index of v in the knots p (K + 1,), -1 outside [p0, pK)"""
    k = np.searchsorted(p, v, side="right") - 1
    return np.where((v >= p[0]) & (v < p[-1]), k, -1)


@pytest.mark.parametrize("c", S.ALL_CASES, ids=IDS)
def test_value_sets_cover_every_bin_and_the_box_edges(c):
    b = S.build(c)
    pX, _, li_f = S.knots(c, 1)
    _, pY, li_i = S.knots(c, 0)
    assert b.xs_val.shape[1] == 4 * c.K + 8 and b.ys_grid.shape[1] == 4 * c.K + 8
    for x, p, li in ((b.xs_val, pX, li_f), (b.ys_grid, pY, li_i)):
        for t, row in enumerate(li.idx_t):
            k = _bins(p[:, t], x[row])
            assert np.all(np.bincount(k[k >= 0], minlength=c.K) >= 3), (row, np.bincount(k[k >= 0], minlength=c.K))
            assert (k < 0).sum() >= 4 and (x[row] == -c.B).sum() == 1 and (x[row] == c.B).sum() == 1
    # float32-representable throughout: the float32 oracle and the device see the float64 oracle's numbers
    for a in (b.th, b.xs_val, b.ys_grid, b.xs_grad, b.xs_fkl, b.ys_fkl, b.mu, b.var):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("c", S.ALL_CASES, ids=IDS)
def test_gradient_sets_stay_off_the_knots(c):
    """Measured in float64, in units of the bin's width: no gradient-set sample within 1e-4 of a knot -- except the
    columns placed on purpose at 1 - 2^-16 of each bin (15e-6 of its width from the right knot), which must be
    strictly inside their bin and at least 2^-17 of its width from the knot: four times the tape's clamp distance
    (2^-19), so the bin and xi they are differentiated at are still theirs."""
    b = S.build(c)
    pX, _, li = S.knots(c, 1)
    assert b.xs_grad.shape[1] == 5 * c.K + 4
    clamp = b.roles_grad == "clamp"
    assert clamp.sum() == c.K
    for t, row in enumerate(li.idx_t):
        p, x = pX[:, t], b.xs_grad[row]
        k = _bins(p, x)
        ins = k >= 0
        assert np.all(ins[clamp]) and np.array_equal(k[clamp], np.arange(c.K))
        dx = np.diff(p)[k[ins]]
        dist = np.minimum(x[ins] - p[k[ins]], p[k[ins] + 1] - x[ins]) / dx
        assert np.all(dist[~clamp[ins]] >= 1e-4), dist[~clamp[ins]].min()
        assert np.all(dist[clamp[ins]] >= 2.0 ** -17), dist[clamp[ins]].min()
    # the forward-KL data are the image of the same set with those columns at 1 - 2^-10: no pre-image within 1e-4 of a knot
    assert np.array_equal(b.xs_fkl[:, ~clamp], b.xs_grad[:, ~clamp])
    if c.gain:  # (the knots of gain = 1 move with the sample: the float32-oracle cap on the gradient is what holds those)
        return
    xr, _ = o.flow_inv(b.spec, b.th, b.ys_fkl)  # ... and rounding the image to float32 moved none of them across or near one
    for t, row in enumerate(li.idx_t):
        p, x = pX[:, t], xr[row]
        k = _bins(p, x)
        assert np.array_equal(k, _bins(p, b.xs_fkl[row]))
        ins = k >= 0
        assert np.all(np.minimum(x[ins] - p[k[ins]], p[k[ins] + 1] - x[ins]) / np.diff(p)[k[ins]] >= 1e-4)


def test_profiles_are_all_used_and_shift_by_one_per_coupling():
    for shape in S.SHAPES:
        c = S.case(shape, 0)
        nt = [(c.d + 1) // 2, c.d // 2]
        used = {S.profile_of(ci, t) for ci in range(2) for t in range(nt[ci])}
        assert used == set(S.PROFILES) if c.d >= 9 else used >= set(S.PROFILES[:3]), (shape, used)
    assert S.profile_of(1, 0) == S.profile_of(0, 1)
    # gain = 0: the raw parameters are the prescribed ones for every sample; gain = 1: they vary with the sample
    c0, c1 = S.case("f32_d5_h32_K10", 0), S.case("f32_d5_h32_K10", 1)
    for c, varies in ((c0, False), (c1, True)):
        b = S.build(c)
        li = o.layers_flat_order(b.spec)[1]
        raw = o.mlp_forward(b.th, li.nets[0], b.xs_val[li.idx_c], None)
        assert bool(np.ptp(raw, axis=1).max() > 1e-3) == varies
