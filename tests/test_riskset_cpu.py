"""CPU checks of the risk-set regression target (NF_TARGET_RISKSET, kind 33: Cox partial likelihood, conditional logit): the
constant (header, Python mirror, Julia extension) with the ABI, the symbol list and the target descriptor unchanged,
nf_target_check's conventions as nf_target_logp reports them BEFORE any device work (a stand-in context is enough), the refusals
of the flows that evaluate their target in their own kernels, the host packing of RiskSetTarget / CoxRegressionTarget /
ConditionalLogitTarget (sort order, tie mass, padding, permutation, constructor errors), the numpy forms against central
differences, the recurrences against the definition, a two-alternative conditional logit against logistic regression, a hand-written
Cox example, the weight-0 row, the float32 floor of the GPU tests' inputs, and the new kernels' resources."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import glm_forms as gf
import parity as P
import riskset_forms as rf
from __graft_entry__ import ROOT, build, load_package

KIND = 33
MAXR = 8192


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def _t(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


def make_target(nf, geometry, p, dtype=torch.float64, **kw):
    X, seg, m, w, off, lin = rf.arrays(geometry, p)
    kw = {"prior_sigma": rf.SIGMA, **kw}
    return nf.RiskSetTarget(_t(X, dtype), seg, m, w, off, lin, **kw)


def test_the_constant_matches_the_header_the_mirror_and_the_julia_extension(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M)}
    for _ in range(2):  # the kinds written relative to the one before them, in order
        for name, base, inc in re.findall(r"^#define (NF_TARGET_\w+) \((NF_TARGET_\w+) \+ (\d+)\)\s*$", hdr, re.M):
            if base in defs:
                defs[name] = defs[base] + int(inc)
    assert "NF_TARGET_RISKSET" in defs, "the header does not define NF_TARGET_RISKSET"
    assert re.search(r"^#define NF_TARGET_RISKSET \(NF_TARGET_ORDINAL_LOGIT \+ 1\)\s*$", hdr, re.M)
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    m = re.search(r"const NF_TARGET_RISKSET = Int32\((\d+)\)", jl)
    assert m and int(m.group(1)) == KIND
    assert defs["NF_TARGET_RISKSET"] == nf._lib.NF_TARGET_RISKSET == KIND == max(defs.values())
    assert len(set(defs.values())) == len(defs)  # no two kinds share a value
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    assert int(re.search(r"^#define NF_RISKSET_MAXR (\d+)", hdr, re.M).group(1)) == nf._lib.NF_RISKSET_MAXR == MAXR
    assert nf.load_library().nf_abi_version() == 4
    assert len(nf.SYMBOLS) == 49
    assert [f[0] for f in nf._lib.Target._fields_] == ["kind", "p0", "p1", "s0", "s1"]


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) and NF_ERR_UNSUPPORTED (-2) for every violated convention without touching the context (N = 0: nothing is
    launched, and a good target's answer is no error)"""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf, buf2 = (C.c_double * 64)(), (C.c_double * 64)()
    p, x = C.cast(buf, C.c_void_p).value, C.cast(buf2, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=8, n=0, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)

    for dtype in (0, 1):
        assert logp(Target(KIND, 0, x, 64.0, 2.0), dtype=dtype) == -1               # p0 = NULL
        assert logp(Target(KIND, p, 0, 64.0, 2.0), dtype=dtype) == -1               # p1 = NULL
        assert logp(Target(KIND, p, p, 64.0, 2.0), dtype=dtype) == -1               # X and the row buffer are one buffer
        for s0 in (0.0, -32.0, 8.0, 33.0, 48.0, 32.5, 2147483648.0, 4294967296.0, math.nan, math.inf):
            assert logp(Target(KIND, p, x, s0, 2.0), dtype=dtype) == -1, s0         # not a positive multiple of 32 that fits an int
        for s1 in (0.0, -1.0, -math.inf, math.nan):
            assert logp(Target(KIND, p, x, 64.0, s1), dtype=dtype) == -1, s1        # the prior sigma is > 0
        assert logp(Target(KIND, p, x, 64.0, 2.0), d=0, dtype=dtype) == -1
        assert logp(Target(KIND, p, x, 33.0, 2.0), d=257, dtype=dtype) == -1        # an argument error first
        assert logp(Target(KIND, p, x, 64.0, 2.0), d=257, dtype=dtype) == -2        # d > 256
        assert logp(Target(KIND, p, x, 64.0, 2.0), d=257, n=4, dtype=dtype) == -2
        assert logp(Target(KIND, p, x, MAXR + 32.0, 2.0), dtype=dtype) == -2        # more rows than the kernels' carries hold
        assert logp(Target(KIND, p, x, 2147483616.0, 2.0), dtype=dtype) == -2
        assert logp(Target(KIND, p, x, 64.0, 2.0), dtype=dtype) >= 0                # past the check
        assert logp(Target(KIND, p, x, 32.0, math.inf), d=1, dtype=dtype) >= 0      # the smallest; the flat prior
        assert logp(Target(KIND, p, x, float(MAXR), 0.5), d=256, dtype=dtype) >= 0  # both caps
    assert logp(Target(34, p, x, 64.0, 2.0)) == -1  # no such kind


def _five(lib, ctx, p, val, desc, tgt):
    return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
            lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
            lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
            lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
            lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with the
    risk-set kind as the target and as the Hamiltonian score; a non-centring layer does not take it -- the stand-in context is never
    used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf, buf2 = (C.c_double * 256)(), (C.c_double * 256)()
    p, x = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    tg = Target(KIND, p.value, x.value, 32.0, 2.0)
    for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1), ("planar", 1)):
        desc = FlowDesc()
        desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
        assert _five(lib, ctx, p, val, desc, tg) == [-2] * 5, kind
    hd = FlowDesc()
    hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 6, 2, 3
    hd.score = C.cast(C.pointer(diag), C.c_void_p)
    assert _five(lib, ctx, p, val, hd, tg) == [-2] * 5
    hd.score = C.cast(C.pointer(tg), C.c_void_p)
    assert _five(lib, ctx, p, val, hd, diag) == [-2] * 5
    with pytest.raises(nf.NFHipError):
        nf.noncentred(object(), make_target(nf, "mass_on_last_live_row", 3))


def test_realnvp_fullrank_and_preconditioned_get_past_every_refusal(nf):
    """the ELBO entry points get past every refusal that comes before device work and stop at the stand-in context's device ordinal (a
    positive HIP error code); the graph form is never an argument error"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    keep = (C.c_char * 4096)()
    C.cast(keep, C.POINTER(C.c_int32))[0] = 1 << 20  # no such device
    ctx = C.cast(keep, C.c_void_p)
    buf, buf2 = (C.c_double * 256)(), (C.c_double * 256)()
    p, x = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    val = C.c_double(0.0)
    for kind in ("realnvp", "fullrank", "preconditioned"):
        for dtype in (0, 1):
            inner = FlowDesc()
            inner.kind, inner.dtype, inner.d, inner.nlayers, inner.n_hidden = NF_KIND["realnvp"], dtype, 7, 2, 2
            inner.hdims[0] = inner.hdims[1] = 32
            desc = inner
            if kind != "realnvp":
                desc = FlowDesc()
                desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 7, 1
                if kind == "preconditioned":
                    desc.nsegments = 1
                    desc.segments = C.cast(C.pointer(inner), C.c_void_p)
            got = _five(lib, ctx, p, val, desc, Target(KIND, p.value, x.value, 64.0, 2.0))
            assert all(c > 0 for c in got[:4]) and (got[4] > 0 or got[4] == -2), (kind, dtype, got)


# ---- host packing -------------------------------------------------------------------------------------------------------------------
def test_riskset_packing_pads_only_the_tail_with_dropped_rows(nf):
    for geometry, p in (("strata_2_to_5", 7), ("mass_on_last_live_row", 3), ("boundary_at_a_block_edge", 4)):
        X, seg, m, w, off, lin = rf.arrays(geometry, p)
        rows = X.shape[0]
        tgt = nf.RiskSetTarget(_t(X), seg, m, w, off, lin, const=0.25, prior_sigma=rf.SIGMA)
        Xd, p0 = rf.target_arrays(tgt)
        R = rf.padded(rows)
        assert tgt.rows == rows and tgt.padded_rows == R == Xd.shape[0] and 0 <= R - rows <= 31 and tgt.d == tgt.p == p
        assert tgt.c.kind == KIND and tgt.c.s0 == R and tgt.c.s1 == rf.SIGMA and tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr()
        o_, lw, m_, s_, l_, par = rf.split_p0(p0, R, p)
        assert np.array_equal(Xd[:rows], X) and not Xd[rows:].any() and np.array_equal(o_[:rows], off) and not o_[rows:].any()
        assert np.array_equal(lw[:rows], np.log(np.where(w > 0, w, 1.0)) + np.where(w > 0, 0.0, -np.inf)) and (lw[rows:] == -np.inf).all()
        assert np.array_equal(m_[:rows], m) and not m_[rows:].any() and s_[0] == 1.0 and np.array_equal(s_[1:rows], seg[1:]) and not s_[rows:].any()
        want = 0.25 - 0.5 * p * math.log(2 * math.pi * rf.SIGMA**2)
        assert np.array_equal(l_, lin) and par[0] == 1 / rf.SIGMA**2 and abs(par[1] - want) <= 1e-14 * abs(want)
        Xw, pw = rf.pack(X, seg, m, w, off, lin, const=0.25)
        assert np.array_equal(Xd, Xw) and np.allclose(p0, pw, rtol=1e-15, atol=0)
    flat = nf.RiskSetTarget(_t(X), seg, m)  # the defaults: weight 1, no offset, no lin, the flat prior
    pf = rf.split_p0(rf.target_arrays(flat)[1], R, p)
    assert not pf[1][:rows].any() and not pf[0].any() and not pf[4].any() and list(pf[5]) == [0.0, 0.0] and flat.c.s1 == math.inf
    t32 = make_target(nf, "strata_2_to_5", 7, torch.float32)
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32
    assert np.array_equal(t32.unpack(_t(np.arange(7.0))).numpy(), np.arange(7.0))


def test_riskset_constructor_errors(nf):
    X, seg, m, w, off, lin = rf.arrays("boundary_inside_a_block", 4)
    X = _t(X)
    T = nf.RiskSetTarget
    neg, bad_w, nan_m = m.copy(), w.copy(), m.copy()
    neg[3], bad_w[5], nan_m[2] = -1.0, -0.5, math.nan
    w0 = w.copy()
    w0[45:50] = 0.0
    m_empty = m.copy()
    m_empty[47] = 1.0  # rows 45..49 open the second segment with weight 0: no risk set yet
    Xnan, offinf = X.clone(), off.copy()
    live = int(np.nonzero(w > 0)[0][0])
    Xnan[live, 1], offinf[live] = math.nan, math.inf
    for make in (lambda: T(X, seg, neg, w), lambda: T(X, seg, m, bad_w), lambda: T(X, seg, nan_m, w), lambda: T(X, seg, m_empty, w0),
                 lambda: T(Xnan, seg, m, w), lambda: T(X, seg, m, w, offinf), lambda: T(X, seg, m, w, off, lin * math.inf)):
        with pytest.raises(ValueError):
            make()
    for make in (lambda: T(X[0], seg, m), lambda: T(X.to(torch.float16), seg, m), lambda: T(X, seg[:-1], m), lambda: T(X, seg, m, w[:-1]),
                 lambda: T(X, seg, m, w, off, lin[:-1]), lambda: T(X, seg, m, prior_sigma=0.0), lambda: T(X, seg, m, prior_sigma=math.nan),
                 lambda: T(X, seg, m, const=math.inf), lambda: T(torch.ones(40, 257, dtype=torch.float64), np.zeros(40), np.zeros(40)),
                 lambda: T(torch.ones(MAXR + 1, 1, dtype=torch.float64), np.zeros(MAXR + 1), np.zeros(MAXR + 1))):
        with pytest.raises(nf.NFHipError):
            make()
    dead = int(np.nonzero(w == 0)[0][0])
    Xd, od = X.clone(), off.copy()
    Xd[dead, 0], od[dead] = math.inf, math.nan  # a dropped row may hold anything: stored as 0
    t = T(Xd, seg, m, w, od)
    assert bool(torch.isfinite(t.A).all()) and float(t.A[dead, 0]) == 0.0 and float(t.p0[dead]) == 0.0
    T(torch.ones(40, 256, dtype=torch.float64), np.zeros(40), np.ones(40))
    T(torch.ones(MAXR, 1, dtype=torch.float64), np.zeros(MAXR), np.zeros(MAXR))


def _cox_data(rows=41, p=3, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, p)).astype(np.float32).astype(np.float64)
    time = rng.integers(1, 9, rows).astype(np.float64)  # many ties
    event = (rng.random(rows) < 0.6).astype(np.float64)
    strata = rng.integers(0, 3, rows)
    wt = rng.choice([1.0, 2.0, 0.5, 0.0], rows)
    off = (0.3 * rng.standard_normal(rows)).astype(np.float32).astype(np.float64)
    return X, time, event, strata, wt, off


def breslow_partial_likelihood(y, X, time, event, strata, wt, off):
    """sum_i wt_i delta_i (eta_i - log sum_{j: same stratum, t_j >= t_i} wt_j exp(eta_j)), written from the textbook"""
    eta = X @ y + off[:, None]
    out = np.zeros(y.shape[1])
    for i in np.nonzero((event == 1) & (wt > 0))[0]:
        risk = (strata == strata[i]) & (time >= time[i]) & (wt > 0)
        out += wt[i] * (eta[i] - np.log((wt[risk, None] * np.exp(eta[risk])).sum(0)))
    return out


def test_cox_packing_sorts_by_stratum_then_time_descending_with_the_tie_mass_on_the_last_row(nf):
    X, time, event, strata, wt, off = _cox_data()
    rows, p = X.shape
    tgt = nf.CoxRegressionTarget(_t(X), time, event, strata, wt, off, prior_sigma=rf.SIGMA)
    order = tgt.order.numpy()
    assert sorted(order) == list(range(rows)) and np.array_equal(order, np.lexsort((-time, strata)))
    ts, ss, es, ws = time[order], strata[order], event[order], wt[order]
    assert (np.diff(ss) >= 0).all() and all((np.diff(ts[ss == s]) <= 0).all() for s in set(ss))  # time descending inside a stratum
    Xd, p0 = rf.target_arrays(tgt)
    R = rf.padded(rows)
    o_, lw, m_, s_, l_, par = rf.split_p0(p0, R, p)
    assert R - rows <= 31 and np.array_equal(Xd[:rows], X[order]) and np.array_equal(o_[:rows], off[order])  # the permutation round trip
    back = np.empty(rows, dtype=int)
    back[order] = np.arange(rows)
    assert np.array_equal(Xd[back], X)
    assert np.array_equal(s_[:rows], np.r_[1.0, (ss[1:] != ss[:-1]).astype(float)])
    with np.errstate(divide="ignore"):
        assert np.array_equal(lw[:rows], np.log(ws))
    seen_tie_with_censored = False
    for s in set(ss):
        for t in set(ts[ss == s]):
            grp = np.nonzero((ss == s) & (ts == t))[0]
            assert np.array_equal(grp, np.arange(grp[0], grp[-1] + 1))  # equal times are contiguous, censored rows inside the group
            assert not m_[grp[:-1]].any() and m_[grp[-1]] == (ws[grp] * es[grp]).sum()  # the whole mass on the group's last row
            seen_tie_with_censored |= len(grp) > 2 and 0 < es[grp].sum() < len(grp)
    assert seen_tie_with_censored
    we = wt * event
    assert np.allclose(l_, we @ X, rtol=1e-14, atol=1e-14)
    want = (we * off).sum() - 0.5 * p * math.log(2 * math.pi * rf.SIGMA**2)
    assert abs(par[1] - want) <= 1e-13 * max(1.0, abs(want)) and tgt.ties == "breslow"
    # the form on this packing is the textbook Breslow partial likelihood plus the prior
    ys = 0.7 * np.random.default_rng(3).standard_normal((p, 5))
    got = rf.definition(ys, Xd, p0)[0]
    prior = -0.5 * (ys * ys).sum(0) / rf.SIGMA**2 - 0.5 * p * math.log(2 * math.pi * rf.SIGMA**2)
    assert np.allclose(got, breslow_partial_likelihood(ys, X, time, event, strata, wt, off) + prior, rtol=1e-12, atol=0)
    hz = tgt.predict(_t(ys), _t(X[:4])).numpy()
    assert hz.shape == (4, 5) and np.allclose(hz, np.exp(X[:4] @ ys), rtol=1e-14)
    for bad in (lambda: nf.CoxRegressionTarget(_t(X), time, event, ties="efron"),):
        with pytest.raises(NotImplementedError):
            bad()
    for bad in (lambda: nf.CoxRegressionTarget(_t(X), time, event + 0.5), lambda: nf.CoxRegressionTarget(_t(X), time * math.nan, event),
                lambda: nf.CoxRegressionTarget(_t(X), time, event, weights=-wt - 1)):
        with pytest.raises(ValueError):
            bad()


def test_cox_with_distinct_times_and_one_stratum_is_the_textbook_partial_likelihood(nf):
    """five subjects, times 5 > 4 > 3 > 2 > 1 after sorting, events at times 4, 2 and 1: written out by hand"""
    X = np.array([[0.5], [-1.0], [2.0], [0.25], [-0.5]])
    time = np.array([2.0, 5.0, 1.0, 4.0, 3.0])
    event = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    tgt = nf.CoxRegressionTarget(_t(X), time, event)
    assert list(tgt.order.numpy()) == [1, 3, 4, 0, 2] and tgt.padded_rows == 32
    Xd, p0 = rf.target_arrays(tgt)
    for b in (-0.8, 0.0, 0.3, 1.7):
        e = np.exp(b * X[:, 0])
        # the event at time 4 (subject 3): at risk 1, 3;  at time 2 (subject 0): 1, 3, 4, 0;  at time 1 (subject 2): all five
        want = (b * 0.25 - math.log(e[1] + e[3])) + (b * 0.5 - math.log(e[1] + e[3] + e[4] + e[0])) + (b * 2.0 - math.log(e.sum()))
        sm = lambda idx: (X[idx, 0] * e[idx]).sum() / e[idx].sum()
        dwant = (0.25 - sm([1, 3])) + (0.5 - sm([1, 3, 4, 0])) + (2.0 - sm([0, 1, 2, 3, 4]))
        for form in (rf.definition, rf.logp_score):
            lp, g = form(np.array([[b]]), Xd, p0)
            assert abs(lp[0] - want) <= 1e-14 * max(1.0, abs(want)) and abs(g[0, 0] - dwant) <= 1e-14 * max(1.0, abs(dwant)), (b, form)


def _clogit_data(sets=23, p=4, seed=4):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 6, sets)
    cs = np.repeat(np.arange(sets), sizes)
    rows = cs.size
    X = rng.standard_normal((rows, p)).astype(np.float32).astype(np.float64)
    chosen = np.zeros(rows)
    for s in range(sets):
        chosen[rng.choice(np.nonzero(cs == s)[0])] = 1.0
    perm = rng.permutation(rows)  # the caller's rows in any order
    return X[perm], cs[perm], chosen[perm], np.repeat(rng.choice([1.0, 2.0, 0.5], sets), sizes)[perm]


def test_conditional_logit_packing_and_predict(nf):
    X, cs, chosen, wt = _clogit_data()
    rows, p = X.shape
    tgt = nf.ConditionalLogitTarget(_t(X), cs, chosen, wt, prior_sigma=rf.SIGMA)
    order = tgt.order.numpy()
    assert np.array_equal(order, np.argsort(cs, kind="stable"))
    Xd, p0 = rf.target_arrays(tgt)
    R = rf.padded(rows)
    o_, lw, m_, s_, l_, par = rf.split_p0(p0, R, p)
    ss = cs[order]
    last = np.r_[ss[1:] != ss[:-1], True]
    assert np.array_equal(Xd[:rows], X[order]) and not lw[:rows].any() and (lw[rows:] == -np.inf).all() and R - rows <= 31
    assert np.array_equal(s_[:rows], np.r_[1.0, (ss[1:] != ss[:-1]).astype(float)]) and np.array_equal(m_[:rows], np.where(last, wt[order], 0.0))
    assert np.allclose(l_, (wt * chosen) @ X, rtol=1e-14, atol=1e-14)
    ys = 0.7 * np.random.default_rng(3).standard_normal((p, 5))
    pr = tgt.predict(_t(ys), _t(X), cs).numpy()
    assert pr.shape == (rows, 5) and all(np.allclose(pr[cs == s].sum(0), 1.0, rtol=0, atol=1e-14) for s in set(cs))
    lik = (wt[:, None] * chosen[:, None] * np.log(pr)).sum(0)
    prior = -0.5 * (ys * ys).sum(0) / rf.SIGMA**2 - 0.5 * p * math.log(2 * math.pi * rf.SIGMA**2)
    assert np.allclose(rf.definition(ys, Xd, p0)[0], lik + prior, rtol=1e-12, atol=0)
    assert np.allclose(tgt.predict(_t(ys[:, 1]), _t(X), cs).numpy(), pr[:, 1], rtol=0, atol=1e-14)
    two = chosen.copy()
    two[np.nonzero(cs == 3)[0]] = 1.0
    uneven = wt.copy()
    uneven[np.nonzero(cs == 5)[0][0]] += 1.0
    for bad in (lambda: nf.ConditionalLogitTarget(_t(X), cs, two), lambda: nf.ConditionalLogitTarget(_t(X), cs, 0 * chosen),
                lambda: nf.ConditionalLogitTarget(_t(X), cs, chosen, uneven), lambda: nf.ConditionalLogitTarget(_t(X), cs, chosen, -wt)):
        with pytest.raises(ValueError):
            bad()


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    t = make_target(nf, "strata_2_to_5", 8, torch.float32)
    assert t.d == 8 and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
    X, time, event, strata, wt, off = _cox_data()
    assert isinstance(nf.CoxRegressionTarget(_t(X), time, event), ob._LINPRED)
    check_target(t, torch.float32, "cpu", 8)
    for args in ((torch.float64, "cpu", 8), (torch.float32, "cuda:0", 8), (torch.float32, "cpu", 7)):
        with pytest.raises(nf.NFHipError):
            check_target(t, *args)

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d, inner=None):
            self.kind, self.theta, self.inner = kind, torch.zeros(1), inner
            self.dist = type("D", (), {"d": d})()

    for kind in ("planar", "radial", "meanfield"):
        assert ob._builtin(F(kind, 8), t) is False   # the closure route, with the device score
    assert ob._builtin(F("hamiltonian", 16), t) is False
    for kind in ("realnvp", "nsf", "composite", "fullrank"):
        assert ob._builtin(F(kind, 8), t) is True    # the library route
    assert ob._builtin(F("preconditioned", 8, F("realnvp", 8)), t) is True
    with pytest.raises(nf.NFHipError):
        ob._builtin(F("planar", 7), t)


# ---- the numpy forms ----------------------------------------------------------------------------------------------------------------
FORM_CASES = [("one_segment", 7), ("strata_2_to_5", 7), ("dead_rows_at_segment_start", 7), ("boundary_at_a_round_edge", 33), ("one_row_segment", 1)]


def _packed(geometry, p):
    return rf.pack(*rf.arrays(geometry, p))


@pytest.mark.parametrize("regime", list(rf.REGIMES))
@pytest.mark.parametrize("case", FORM_CASES, ids=lambda c: "%s_d%d" % c)
def test_the_form_is_the_derivative_of_its_value(case, regime):
    """central differences in float64, every coordinate: the value's differences agree with the score to 1e-6 of max(1, |score|) (the
    step is 1e-5 relative to 1 + |y_i|: truncation 1e-10 |f'''|, round-off 1e-16 |f| / 1e-5) -- both forms"""
    Xp, p0 = _packed(*case)
    y0 = rf.sample_ys(case[1], 1, regime)
    for form in (rf.definition, rf.logp_score):
        sc = form(y0, Xp, p0)[1][:, 0]
        worst = 0.0
        for i in range(y0.shape[0]):
            e = np.zeros_like(y0)
            e[i] = 1e-5 * (1 + abs(y0[i, 0]))
            fd = (form(y0 + e, Xp, p0)[0][0] - form(y0 - e, Xp, p0)[0][0]) / (2 * e[i, 0])
            worst = max(worst, abs(fd - sc[i]) / max(1.0, abs(sc[i])))
        print(f"riskset central differences {case} {regime} {form.__name__}: {worst:.2e}")
        assert worst <= 1e-6, (case, regime, form.__name__, worst)


@pytest.mark.parametrize("regime", list(rf.REGIMES))
@pytest.mark.parametrize("case", rf.CASES, ids=lambda c: "%s_d%d" % c)
def test_the_recurrences_equal_the_definition(case, regime):
    """float64: the two recurrences against explicit risk sets, 1e-12 of |log p|inf and of |g|inf"""
    Xp, p0 = _packed(*case)
    ys = rf.sample_ys(case[1], 5, regime)
    (l, g), (lr, gr) = rf.definition(ys, Xp, p0), rf.logp_score(ys, Xp, p0)
    el, eg = np.abs(lr - l).max() / np.abs(l).max(), np.abs(gr - g).max() / np.abs(g).max()
    print(f"riskset recurrences vs definition {case} {regime}: {el:.2e} {eg:.2e}")
    assert np.isfinite(l).all() and np.isfinite(g).all() and el <= 1e-12 and eg <= 1e-12, (case, regime, el, eg)


def test_a_two_alternative_conditional_logit_is_logistic_regression_on_the_differences(nf):
    """sets of two: P(chosen) = sigmoid((x_chosen - x_other) . y), so log p is glm_forms' logit regression on the feature differences
    with the sets' weights -- value and score, flat prior and N(0, sigma^2)"""
    rng = np.random.default_rng(8)
    sets, p = 37, 3
    X = rng.standard_normal((2 * sets, p)).astype(np.float32).astype(np.float64)
    cs = np.repeat(np.arange(sets), 2)
    first = rng.integers(0, 2, sets)
    chosen = np.zeros(2 * sets)
    chosen[2 * np.arange(sets) + first] = 1.0
    wt = np.repeat(rng.choice([1.0, 2.0, 0.5], sets), 2)
    A = X[2 * np.arange(sets) + first] - X[2 * np.arange(sets) + 1 - first]
    glm_p0 = np.concatenate([np.zeros(p), np.zeros(sets), wt[::2], [0.0, 0.0]])
    ys = rng.standard_normal((p, 7))
    for sigma in (math.inf, 2.0):
        tgt = nf.ConditionalLogitTarget(_t(X), cs, chosen, wt, prior_sigma=sigma)
        Xd, p0 = rf.target_arrays(tgt)
        want = gf.logp_score("logit", ys, A, glm_p0, sigma)
        for form in (rf.definition, rf.logp_score):
            got = form(ys, Xd, p0)
            assert np.allclose(got[0], want[0], rtol=1e-13, atol=0) and np.abs(got[1] - want[1]).max() <= 1e-13 * np.abs(want[1]).max(), sigma


def test_a_zero_weight_row_of_huge_features_leaves_the_form_alone():
    X, seg, m, w, off, lin = rf.arrays("dead_rows_at_segment_start", 7)
    ys = rf.sample_ys(7, 5, "spread")
    dead = np.nonzero(w == 0)[0]
    assert dead.size >= 9
    Xb, ob = X.copy(), off.copy()
    Xb[dead], ob[dead] = 1e30, 50.0
    for form in (rf.definition, rf.logp_score):
        want, got = form(ys, *rf.pack(X, seg, m, w, off, lin)), form(ys, *rf.pack(Xb, seg, m, w, ob, lin))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    l32, s32 = rf.logp_score(ys.astype(np.float32), *rf.pack(Xb, seg, m, w, ob, lin))
    assert np.isfinite(l32).all() and np.isfinite(s32).all()


# ---- the float32 floor of the GPU tests' inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(rf.REGIMES))
@pytest.mark.parametrize("case", rf.CASES, ids=lambda c: "%s_d%d" % c)
def test_the_float32_form_alone_stays_inside_the_tolerances(nf, case, regime):
    """the float32 recurrences against the float64 definition on the GPU tests' inputs, read back from the Float32 target the
    constructor folds (what the device reads): at most 0.5x the element-wise tolerance on log p and 0.5x GRAD_RTOL on the score, so the
    floor is not expected to decide a nf_target_logp check.  (Float32's unit round-off is 6e-8; a row's c is a chain of at most 288
    logaddexp, each within a few units of round-off of |c| <= 70, and log p sums at most 288 of them: well below 1e-5 relative.  The
    fraction is a bound on how much of the tolerance the format itself may use, not a measurement.)"""
    tgt = make_target(nf, *case, torch.float32)
    Xd, p0 = rf.target_arrays(tgt)
    Xw, pw = _packed(*case)
    assert np.array_equal(Xd, Xw) and np.allclose(p0, pw, rtol=1e-7, atol=0)
    for n in rf.N_SIZES:
        ys = rf.sample_ys(case[1], n, regime)
        l64, s64 = rf.definition(ys, Xd, p0)
        l32, s32 = rf.logp_score(ys.astype(np.float32), Xd, p0)
        assert l32.dtype == s32.dtype == np.float32 and np.isfinite(l64).all() and np.isfinite(s64).all() and np.isfinite(s32).all()
        lr = float((np.abs(l32 - l64) / (P.Y_ATOL + P.Y_RTOL * np.abs(l64))).max())
        gr = float(np.abs(s32 - s64).max() / np.abs(s64).max()) / P.GRAD_RTOL
        print(f"riskset floor {case} {regime} N={n}: logp {lr:.4f}x, score {gr:.5f}x")
        assert lr <= 0.5 and gr <= 0.5, (case, regime, n, lr, gr)


# ---- the float64 loop train_flow is compared with -----------------------------------------------------------------------------------
TRAIN = (("strata_2_to_5", 8), 64, 9, 0.05, 6)  # case, draws, seed, Adam's rate, steps


def train_target(nf, device="cpu"):
    X, seg, m, w, off, lin = rf.arrays(*TRAIN[0])
    return nf.RiskSetTarget(torch.tensor(X, dtype=torch.float64, device=device), seg, m, w, off, lin, prior_sigma=rf.SIGMA)


def fullrank_numpy_losses(Xd, p0, n, seed, lr, iters, fixed=None):
    """Full-rank Gaussian VI on the risk-set posterior as a float64 numpy loop from theta = [0 ; I] (tests/fullrank_ref.py's layout):
    draws of stream i, the definition's score, oracle Adam.  Returns the losses, theta, and -ELBO on the fixed draws before and after."""
    import fullrank_ref as fr
    import nf_oracle as o

    d = Xd.shape[1]
    ref = lambda y: rf.definition(y, Xd, p0)
    th = fr.join(np.zeros(d), np.eye(d))
    before = fr.neg_elbo_value_and_grad(th, fixed, ref)[0] if fixed is not None else None
    m, v = np.zeros_like(th), np.zeros_like(th)
    losses = []
    for i in range(iters):
        xs = o.base_sample(d, n, seed, 0, i, precision="f64")
        loss, g = fr.neg_elbo_value_and_grad(th, xs, ref)
        losses.append(float(loss))
        o.adam_update(th, g, m, v, i + 1, lr=lr)  # in place
    after = fr.neg_elbo_value_and_grad(th, fixed, ref)[0] if fixed is not None else None
    return losses, th, before, after


def test_the_numpy_training_loop_descends(nf):
    """the float64 loop alone lowers -ELBO on a fixed draw set, so the GPU comparison does not rest on luck"""
    import nf_oracle as o

    _, n, seed, lr, iters = TRAIN
    Xd, p0 = rf.target_arrays(train_target(nf))
    fixed = o.base_sample(Xd.shape[1], 256, 1234, 0, 0, precision="f64")
    losses, th, before, after = fullrank_numpy_losses(Xd, p0, n, seed, lr, iters, fixed)
    print("riskset fullrank numpy loop", losses, before, after)
    assert all(np.isfinite(losses)) and np.isfinite(th).all() and after < before


# ---- resources and sources -----------------------------------------------------------------------------------------------------------
def test_riskset_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_target_riskset_tiled<", 4), ("void k_target_riskset<", 2)):  # DB in {1, 2, 4, 8}; {float, double}
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        for name, agpr, vgpr, sgpr, scratch, lds in hit:
            assert scratch == 0, (name, scratch)
            assert vgpr <= 512, (name, vgpr)    # 256 threads per workgroup: one wave per SIMD may use the whole register file
            assert lds <= 16384, (name, lds)    # static LDS: the published pairs and the reductions (tile, images and carries are dynamic)
            if re.search(r"tiled<[12]>\(", name[:80]):
                assert vgpr <= 256, (name, vgpr)  # DB <= 2: two workgroups per CU


def test_the_new_source_is_built_and_has_no_build_time_variants():
    from __graft_entry__ import SOURCES

    assert "nf_riskset.hip" in SOURCES
    src = open(os.path.join(ROOT, "normalizingflows.jl_amd", "csrc", "nf_riskset.hip")).read()
    assert not re.search(r"^\s*#\s*if(def|ndef)?\b.*\bNF_", src, re.M)
    assert 'ProfScope ps(ctx, "target_riskset")' in src
    assert "atomic" not in src.replace("no atomics", "")
