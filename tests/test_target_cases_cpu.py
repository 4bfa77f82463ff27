"""The conditions tests/target_cases.py must meet for tests/test_gpu_target_regimes.py to mean something -- asserted from the two
oracles (float64, and the same algorithm op by op in float32) alone, no device.

  1-3  every cloud is plain or norm-wise conditioned: the float32 oracle's max |err| / |ref|inf is <= 0.1 GRAD_RTOL on log p and
       on the score of EVERY cloud (so the gradient measure is asserted everywhere, and a cloud that is not plain is still held)
  4    at least two thirds of each target's clouds are plain, and every (target, parameter set) has a plain cloud at every d
  5    the aggregate checks' eligibility rule leaves something to check: per flow family and target, at least half of the losses and
       of the gradients are eligible (measured on the cheap shapes; the device test counts them at every shape)
  6    every float64 and float32 oracle value is finite
  7    the oracle's scores equal central finite differences of the oracle's own log p in float64, at every parameter set and
       cloud (d = 2, 3, 9): the clouds leave the regime the oracle was validated in (tests/test_oracle.py: N(0, 1) points)
and the cases' own bookkeeping: every n of NS occurs for every (target, d), the dimensions straddle the boundaries the module
names.  The counts of plain and norm-wise clouds per target are printed (pytest -s); DESIGN section 5 quotes them.
"""
import numpy as np
import pytest

import target_cases as T

o = T.o
FD_MEDIAN_REL = 1e-5  # the finite-difference tolerance relative to the score, at the median element of a target's clouds


def test_every_cloud_is_finite_and_conditioned():
    summary = {}
    for target in T.TARGETS:
        rows = T.all_clouds(target)
        plain = 0
        worst_lp = worst_g = 0.0
        per_set = {}
        for pi, d, ci in rows:
            R = T.reference(target, pi, d, ci)
            name = f"{target} set {pi} d={d} {T.clouds(target, pi, d)[ci].name}"
            for a in (R.lp64, R.g64, R.lp32, R.g32):
                assert np.isfinite(a).all(), name
            assert R.floor_lp <= T.FLOOR_SHARE * T.GRAD_RTOL, (name, "log p", R.floor_lp)
            assert R.floor_g <= T.FLOOR_SHARE * T.GRAD_RTOL, (name, "score", R.floor_g)
            worst_lp, worst_g = max(worst_lp, R.floor_lp), max(worst_g, R.floor_g)
            plain += R.plain
            per_set.setdefault((pi, d), []).append(R.plain)
        summary[target] = (len(rows), plain, len(rows) - plain)
        print(f"target cases: {target}: {len(rows)} clouds, {plain} plain, {len(rows) - plain} norm-wise only; float32 oracle by the gradient measure: "
              f"log p <= {worst_lp:.2e}, score <= {worst_g:.2e}")
        assert 3 * plain >= 2 * len(rows), (target, plain, len(rows))
        for (pi, d), flags in per_set.items():
            assert any(flags), f"{target} set {pi} d={d}: no plain cloud"
    assert set(summary) == set(T.TARGETS)


def test_plain_clouds_leave_conditioned_elements_to_hold():
    """a plain cloud's mask keeps >= 95 % of each array, at every prefix n a conditioned element remains for most clouds -- and
    lane 0 alone (n = 1) is checked element-wise on at least two thirds of each target's plain clouds"""
    for target in T.TARGETS:
        first = total = 0
        for pi, d, ci in T.all_clouds(target):
            R = T.reference(target, pi, d, ci)
            if not R.plain:
                continue
            assert R.cond_lp.mean() >= T.PLAIN_SHARE and R.cond_g.mean() >= T.PLAIN_SHARE
            total += 1
            first += bool(R.cond_lp[0] and R.cond_g[:, 0].all())
        assert 3 * first >= 2 * total, (target, first, total)


def _fd_scale(target, pi, y):
    """the local length scale of log p per sample: 1, but r near WarpedGauss' origin (log r) and sigma on Cross' ridges"""
    if target == "warped":
        return np.minimum(1.0, np.hypot(y[0], y[1]))[None, :]
    if target == "cross":
        return np.full((1, y.shape[1]), min(1.0, T.params(target, pi)[1]))
    return np.ones((1, y.shape[1]))


@pytest.mark.parametrize("target", T.TARGETS)
def test_oracle_scores_against_finite_differences_of_its_logp(target):
    """Central differences in float64 with h_i = 1e-6 max(|y_i|, l), l the local length scale (_fd_scale).  The quotient's own error:
    rounding, <= 64 eps max|log p(y +- h)| / 2h (64: log p is a sum of up to a few dozen terms that may cancel), and truncation,
    estimated by Richardson from the step 2h: |fd(2h) - fd(h)| x 4 / 3 (the h^2 term is a third of that difference; 4x for
    the h^4 term and the estimate's own noise).  TOLERANCE = rounding + truncation + 1e-9 |score|: a score off by a factor, a
    sign or a missing term keeps fd(h) = fd(2h) and fails by orders of magnitude."""
    eps = 2.0 ** -52
    worst, rel = 0.0, []
    for pi, d, ci in T.all_clouds(target, None if target in T.D2 else T.FD_DIMS):
        y = np.array(T.points(target, pi, d, ci))
        ot = T.otarget(target, pi, d)
        g = o.target_grad(ot, y)
        scale = _fd_scale(target, pi, y)
        for i in range(d):
            h = 1e-6 * np.maximum(np.abs(y[i]), scale[0])
            fds, mag = [], 0.0
            for k in (1.0, 2.0):
                yp, ym = y.copy(), y.copy()
                yp[i] += k * h
                ym[i] -= k * h
                step = yp[i] - ym[i]  # the step as represented
                lp, lm = o.target_logp(ot, yp), o.target_logp(ot, ym)
                fds.append((lp - lm) / step)
                if k == 1.0:
                    mag = np.maximum(np.abs(lp), np.abs(lm))
            tol = 64 * eps * mag / (2 * h) + 4.0 / 3.0 * np.abs(fds[1] - fds[0]) + 1e-9 * np.abs(g[i])
            err = np.abs(fds[0] - g[i])
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (target, pi, d, T.clouds(target, pi, d)[ci].name, i, float((err / tol).max()), float(np.abs(g[i]).max()))
            # ... and the tolerance is a small part of the score (elements that cancel to nothing aside; where exp(-y0) = 2e-9 the score
            # of a Funnel coordinate is 1e-5 and the rounding term alone a hundredth of it: hence the median over the target's clouds)
            big = np.abs(g[i]) >= 1e-3 * np.abs(g[i]).max()
            rel.append(tol[big] / np.abs(g[i])[big])
    loose = float(np.median(np.concatenate(rel)))
    assert loose <= FD_MEDIAN_REL, (target, loose)
    print(f"target cases: {target}: oracle score against finite differences, worst |fd - g| / tolerance = {worst:.3f}; median tolerance / |score| = {loose:.2e}")


@pytest.mark.parametrize("kind,dims", [("realnvp", (2, 3)), ("fullrank", (2, 3)), ("meanfield", (2, 9)), ("planar", (2, 9)), ("radial", (2, 9))])
def test_aggregate_checks_have_eligible_cases(kind, dims):
    """condition 5 from the oracles on the near-identity flows: per target, at least one loss and one gradient pass the rule, the
    per-sample ELBO terms of every case are finite, and each is plain or norm-wise conditioned"""
    for d in dims:
        for target in T.targets_at(d):
            nl = ng = nall = nterm = 0
            for pi in range(len(T.PARAMS[target])):
                ot = T.otarget(target, pi, d)
                for ci, c in enumerate(T.clouds(target, pi, d)):
                    xs = T.points(target, pi, d, ci)[:, :T.n_of(pi, ci)]
                    e64, l64, g64 = T.flow_oracle(kind, d, ot, xs, np.float64)
                    e32, l32, g32 = T.flow_oracle(kind, d, ot, xs, np.float32)
                    name = f"{kind} {target} set {pi} d={d} {c.name}"
                    assert np.isfinite(e64).all() and np.isfinite(g64).all() and np.isfinite(e32).all(), name
                    cond, share, floor = T.classify(e64, e32)
                    share = float((cond & (T.TERM_ULPS * 2.0 ** -24 * T.term_scale(e64, xs) <= T.tol32(e64))).mean())  # (hold's rule for ELBO terms)
                    by_terms = float(np.abs(e32 - e64).max() / T.term_scale(e64, xs).max())  # (target_cases.term_scale: log q0 cancels log p)
                    assert share >= T.PLAIN_SHARE or min(floor, by_terms) <= T.FLOOR_SHARE * T.GRAD_RTOL, (name, share, floor, by_terms)
                    nterm += not (share >= T.PLAIN_SHARE or floor <= T.FLOOR_SHARE * T.GRAD_RTOL)
                    lok, gok = T.aggregate_ok(e64, l64, l32, g64, g32.astype(np.float64), T.term_scale(e64, xs))
                    nl, ng, nall = nl + lok, ng + gok, nall + 1
            print(f"target cases: {kind} d={d} {target}: {nl} losses and {ng} gradients of {nall} cases eligible for the aggregate checks; "
                  f"{nterm} held by the scale of their terms")
            assert T.eligible_enough(nl, ng, nall), (kind, d, target, nl, ng, nall)


@pytest.mark.parametrize("target,d", [("funnel", 9), ("banana", 3), ("cross", 2), ("warped", 2), ("diaggauss", 9), ("funnel", 64)])
def test_the_placed_flow_carries_the_draws_to_its_cloud(target, d):
    """sites 7, 8: the oracle's image of N(0, 1) draws under target_cases.placed_theta has the cloud's centre and scale per coordinate
    (2 000 draws: the mean within 5 standard errors + 1e-3 of the scale, the standard deviation within 10 %) -- this pins the
    convention that the couplings of flat index 0 and 1 are applied last and carry the whole centre"""
    lim = np.exp(T.PLACE_L * T.PLACE_TANH)
    xs = o.base_sample(d, 2000, seed=5, precision="f32")
    for pi in range(len(T.PARAMS[target])):
        for ci, c in enumerate(T.clouds(target, pi, d)):
            if not T.reachable(target, pi, d, ci):
                continue
            y = o.flow_fwd(T.placed_spec("realnvp", d), T.placed_theta("realnvp", target, pi, d, ci), xs)[0]
            scale = np.clip(c.scale, 1.0 / lim, lim)
            assert (np.abs(y.mean(axis=1) - c.centre) <= scale * (5.0 / np.sqrt(2000) + 1e-3)).all(), (target, pi, d, c.name)
            assert (np.abs(y.std(axis=1) / scale - 1.0) <= 0.1).all(), (target, pi, d, c.name)


def test_bookkeeping():
    for target in T.TARGETS:
        for pi in range(len(T.PARAMS[target])):
            ncl = len(T.clouds(target, pi, 2))
            assert {T.n_of(pi, ci) for ci in range(ncl)} == set(T.NS) or ncl < 3, (target, pi)
    # each boundary the module names has its two sides in DIMS
    for lo in (7, 8, 16, 32, 64, 128):
        assert lo in T.DIMS and lo + 1 in T.DIMS
    assert {2, 3} <= set(T.DIMS) and any(d % 2 for d in T.DIMS)
    assert [T.dpl_for(d) for d in (16, 17, 32, 33, 64, 65, 128, 129)] == [1, 2, 2, 4, 4, 8, 8, 16]
    # the training launch on each side of the boundaries (asserted against the profiler on the device)
    assert [T.train_launch("planar", False, d) for d in (2, 64, 65, 129)] == ["planar_step", "planar_step", "simple_step", "simple_step"]
    assert [T.train_launch("radial", False, d) for d in (7, 8, 64, 65)] == ["simple_step", "radial_step", "radial_step", "simple_step"]
    assert [T.train_launch("planar", True, d) for d in (65, 129)] == ["simple_step", "split"]
    assert T.train_launch("planar", False, 33, no_tile=True) == "simple_step"
    for kind, f64, nl, dims in T.FLOW_CASES:  # the rows meant for site 3 split, the others do not (Float64 d = 129 aside)
        if nl in (5, 13, 17):
            assert all(T.train_launch(kind, f64, d, nl) == "split" for d in dims), (kind, f64, nl)
        else:
            assert all(T.train_launch(kind, f64, d, nl) != "split" or (f64 and d == 129) for d in dims), (kind, f64, nl)
    # every flow case's d is one of DIMS
    for _, _, _, dims in T.FLOW_CASES:
        assert set(dims) <= set(T.DIMS)
